"""GPU parity of the per-channel symbol path (sdrhip_detectorbank_create / sdrhip_bitsbank_create and their
set_channel calls): every row of a mixed bank against (1) a one-parameter handle (channels = 1) run on that row alone with the
same call sequence and (2) the numpy restatement tests/fsk_restatement.py — both pinned to the compiled reference by the g18
fixtures. Bit for bit over every row, every byte and every count: there is no tolerance. The module name makes
tests/conftest.py run every process() call inside the red-zoned device arena; the BitStream bank runs on device buffers of
its own whose bytes behind every row's count must keep their fill pattern.

"After call 3" of a set_channel is read as: between the calls of index 3 and 4 of the ragged sequence (259 samples in — no
multiple of 18 or 242, so a wrong phase origin shows)."""
import ctypes as C

import numpy as np
import pytest

import fsk_restatement as fr
import libsdr_amd as sa

pytestmark = pytest.mark.gpu

FS = 22050.0
LENS = [0, 1, 17, 241, 255, 256, 257, 700, 1]
BIG = 4096                 # the BitStream bank's extra call
SWITCH = 4                 # set_channel happens before the call of this index
TOTAL = sum(LENS) + BIG
AX25, RTTY = (1200.0, 1200.0, 2200.0), (90.90, 930.0, 1100.0)   # baud, mark, space


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def _fsk(baud, f0, f1, L):
    lm, ls = sa.design_fsk_lut(FS, baud, f0), sa.design_fsk_lut(FS, baud, f1)
    assert lm.shape == ls.shape == (L, 2) and fr.corr_len(FS, baud) == L
    return ("fsk", lm, ls)


def _det_channels():
    """The issue's table, in its deliberately unsorted order; max_corr_len = 300."""
    return [_fsk(*AX25, 18), ("ask", False), _fsk(*RTTY, 242), ("ask", True), _fsk(22050.0, 1200.0, 2200.0, 1),
            _fsk(11025.0, 1200.0, 2200.0, 2), _fsk(73.5, 1200.0, 2200.0, 300), _fsk(*AX25, 18)]


def _audio(n=TOTAL):
    """8 rows: keyed tones plus noise, different per row (rows 0 and 7 share their parameters, not their input); row 5 is all
    zero (f == 0 -> symbol 0) and row 6 holds only +/-32767."""
    r = np.random.default_rng(20240518)
    x = np.zeros((8, n), np.int16)
    for c, (baud, f0, f1) in enumerate([AX25, (512.0, 600.0, 600.0), RTTY, AX25, AX25, AX25, AX25, AX25]):
        per = max(int(FS / baud), 1)
        key = np.repeat(r.integers(0, 2, n // per + 2), per)[:n]
        ph = 2 * np.pi * np.cumsum(np.where(key, f1, f0) / FS) + r.uniform(0, 6)
        v = r.uniform(3000, 14000) * np.sin(ph) * (key if c in (1, 3) else 1) + r.normal(0, 1500, n)
        x[c] = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    x[5] = 0
    x[6] = np.where(r.integers(0, 2, n) > 0, 32767, -32767)
    return x


def _calls(x, lens):
    out, at = [], 0
    for n in lens:
        out.append(x[..., at:at + n])
        at += n
    return out


# ---- one row, by the two references: a schedule is [(first call index, config), ...] — a fresh node from that call on ------
def _ref_det_node(cfg):
    if cfg[0] == "ask":
        return lambda x: fr.ask_detect(x, cfg[1])
    node = fr.FSKDetector(cfg[1], cfg[2], channels=1)
    return lambda x: node.process(x[None])[0]


def _gpu_det_node(ctx, cfg, max_in):
    if cfg[0] == "ask":
        node = sa.ASKDetector(ctx, invert=cfg[1], channels=1, max_in=max_in)
    else:
        node = sa.SymbolDetector(ctx, sa.DET_FSK, cfg[1], cfg[2], channels=1, max_in=max_in)
    return lambda x: node.process(x)[0]


def _ref_bits_node(cfg):
    node = fr.BitStream(FS, cfg[0], cfg[1], channels=1)
    return lambda s: node.process(s[None])[0]


def _gpu_bits_node(ctx, cfg, max_in):
    node = sa.BitStream(ctx, FS, cfg[0], cfg[1], channels=1, max_in=max_in)
    return lambda s: node.process(s)[0]


def _row(make, schedule, calls):
    out, node = [], None
    for k, x in enumerate(calls):
        for at, cfg in schedule:
            if at == k:
                node = make(cfg)
        out.append(np.asarray(node(x)))
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype == np.uint8 and np.array_equal(g, w), (what, "call", k, g.shape, w.shape)


# ---- detector bank -----------------------------------------------------------------------------------------------------------
def _det_schedules(switch):
    chans = _det_channels()
    sched = [[(0, cfg)] for cfg in chans]
    if switch:
        sched[2].append((SWITCH, _fsk(*AX25, 18)))       # L = 242 -> 18: the parameters of rows 0 and 7
        sched[1].append((SWITCH, _fsk(*RTTY, 242)))      # ASK -> FSK, L = 242
        sched[7].append((SWITCH, chans[7]))              # its own parameters again: still a restart (row 0 has the same, unbroken)
    return chans, sched


@pytest.fixture(scope="module")
def audio():
    x = _audio()
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("switch", [False, True], ids=["steady", "set_channel"])
def test_detector_bank(ctx, audio, switch):
    chans, sched = _det_schedules(switch)
    calls = _calls(audio[:, :sum(LENS)], LENS)
    bank = sa.SymbolDetectorBank(ctx, chans, max_in=max(LENS), max_corr_len=300)
    assert bank.kernel_names == ["detectorbank_kernel"]
    got = []
    for k, x in enumerate(calls):
        for c in range(8):
            for at, cfg in sched[c][1:]:
                if at == k:
                    bank.set_channel(c, cfg)
        s = bank.process(x)
        assert s.shape == x.shape and s.dtype == np.uint8
        got.append(s)
    for c in range(8):
        row = [g[c] for g in got]
        rcalls = [x[c] for x in calls]
        want = _row(_ref_det_node, sched[c], rcalls)
        _same(row, want, ("restatement", c))
        _same(row, _row(lambda cfg: _gpu_det_node(ctx, cfg, max(LENS)), sched[c], rcalls), ("one-parameter handle", c))
    whole = np.concatenate(got, axis=1)
    assert not whole[5].any()                                   # the all-zero row: f == 0 -> 0
    assert whole[0].any() and whole[7].any() and not np.array_equal(whole[0], whole[7])
    assert whole[3].any() and whole[6].any()


def test_detector_bank_reset_and_empty_calls(ctx, audio):
    """reset: every channel a fresh node whatever the sample count before; an empty call moves nothing."""
    chans, sched = _det_schedules(False)
    bank = sa.SymbolDetectorBank(ctx, chans, max_in=700, max_corr_len=300)
    bank.process(audio[:, 1000:1259])
    bank.reset()
    calls = _calls(audio[:, :558], [301, 0, 257])
    got = [bank.process(x) for x in calls]
    for c in range(8):
        _same([g[c] for g in got], _row(_ref_det_node, sched[c], [x[c] for x in calls]), ("after reset", c))


# ---- BitStream bank ----------------------------------------------------------------------------------------------------------
N, T = sa.BITS_NORMAL, sa.BITS_TRANSITION
BIT_ROWS = [(1200.0, N), (1200.0, T), (90.90, N), (512.0, N), (2400.0, T), (FS / 3, N)]
BIT_LENS = LENS + [BIG]


@pytest.fixture(scope="module")
def symbols(ctx, audio):
    """Rows 0 - 2: the detector bank's OWN output rows 0, 7 and 2 over the BitStream bank's call sequence (equal to the
    restatement's, which is checked here too); rows 3 - 5: seeded symbol rows whose flips run slightly faster than the row's
    baud rate, which drives the PLL towards its upper limit (row 5: Fs / baud nearly an integer, where a call emits more bits
    than 1 + n / corr_len)."""
    chans = _det_channels()
    bank = sa.SymbolDetectorBank(ctx, chans, max_in=BIG, max_corr_len=300)
    own = np.concatenate([bank.process(x) for x in _calls(audio, BIT_LENS)], axis=1)
    bank.close()
    assert own.shape == (8, TOTAL)
    s = np.zeros((6, TOTAL), np.uint8)
    for r, c in enumerate((0, 7, 2)):
        s[r] = own[c]
        assert np.array_equal(s[r], fr.FSKDetector(chans[c][1], chans[c][2]).process(audio[c][None])[0]), c
    rng, t = np.random.default_rng(7), np.arange(TOTAL)
    s[3] = ((t / (FS / 512.0 * 0.99)).astype(np.int64) & 1) ^ (rng.random(TOTAL) < 0.02)
    s[4] = np.repeat(rng.integers(0, 2, TOTAL // 9 + 1), 9)[:TOTAL]
    s[5] = (t / 2.985).astype(np.int64) & 1
    s.setflags(write=False)
    return s


def _bits_schedules(switch):
    sched = [[(0, cfg)] for cfg in BIT_ROWS]
    if switch:
        sched[2].append((SWITCH, (1200.0, N)))           # L = 242 -> 18: row 0's parameters
        sched[1].append((SWITCH, (90.90, N)))            # L = 18 -> 242, TRANSITION -> NORMAL
        sched[4].append((SWITCH, BIT_ROWS[4]))           # its own parameters again: still a restart
    return sched


def _current(sched, k):
    return [s for s in sched if s[0] <= k][-1][1]


@pytest.mark.hostptr_only
@pytest.mark.parametrize("switch", [False, True], ids=["steady", "set_channel"])
def test_bitstream_bank(ctx, symbols, switch):
    sched = _bits_schedules(switch)
    calls = _calls(symbols, BIT_LENS)
    bank = sa.BitStreamBank(ctx, FS, [b for b, _ in BIT_ROWS], [m for _, m in BIT_ROWS], max_in=BIG)
    assert bank.kernel_names == ["bitsbank_pll_kernel", "bitsbank_flags_kernel"]
    assert bank.corr_len == 242
    CH, si, pad, fill = 6, BIG + 13, 9, 0x5A
    so_max = bank.out_capacity(BIG) + pad
    dsym, dbits, dcnt = ctx.malloc(CH * si), ctx.malloc(CH * so_max), ctx.malloc(4 * CH)
    got, over, single = [], 0, {}
    try:
        for k, x in enumerate(calls):
            for c in range(CH):
                for at, cfg in sched[c][1:]:
                    if at == k:
                        bank.set_channel(c, *cfg)
            n = x.shape[1]
            refs = [fr.BitStream(FS, *_current(sched[c], k)) for c in range(CH)]
            cap = bank.out_capacity(n)
            assert cap == max(r.capacity(n) for r in refs)          # the largest channel's: the row stride a caller needs
            for c, r in enumerate(refs):
                info = bank.channel_info(c, n)
                assert info["corr_len"] == r.L and info["capacity"] == r.capacity(n), (k, c, info)
                assert np.float32(info["omega_min"]) == r.omin and np.float32(info["omega_max"]) == r.omax, (k, c, info)
                cfg = _current(sched[c], k)
                if cfg not in single:
                    single[cfg] = sa.BitStream(ctx, FS, cfg[0], cfg[1], channels=1, max_in=BIG)
                one = single[cfg]                                    # the one-parameter handle with the row's parameters
                assert info["capacity"] == one.out_capacity(n) and info["corr_len"] == one.corr_len, (k, c, info)
            assert cap == max(single[_current(sched[c], k)].out_capacity(n) for c in range(CH))
            so = cap + pad
            full = np.zeros((CH, si), np.uint8)
            full[:, :n] = x
            ctx.h2d(dsym, full)
            ctx.memset(dbits, fill, CH * so_max)
            ctx.memset(dcnt, fill, 4 * CH)
            bank.process_dev(dsym, n, si, dbits, so, dcnt)
            ctx.synchronize()
            out, cnt = np.zeros((CH, so), np.uint8), np.zeros(CH, np.uint32)
            ctx.d2h(out, dbits)
            ctx.d2h(cnt, dcnt)
            for c in range(CH):
                assert cnt[c] <= refs[c].capacity(n), (k, c, cnt[c])
                assert (out[c, cnt[c]:] == fill).all(), ("bytes behind row %d's count were written" % c, k)
            if n == 0:
                assert not cnt.any() and (out == fill).all()
            got.append([out[c, :cnt[c]].copy() for c in range(CH)])
            over += int(n > 0 and cnt[5] > 1 + n // 3)
    finally:
        for p in (dsym, dbits, dcnt):
            ctx.free(p)
    assert over > 0   # row 5 does exceed the reference's own buffer size 1 + n / corr_len
    for c in range(CH):
        row, rcalls = [g[c] for g in got], [x[c] for x in calls]
        _same(row, _row(_ref_bits_node, sched[c], rcalls), ("restatement", c))
        _same(row, _row(lambda cfg: _gpu_bits_node(ctx, cfg, BIG), sched[c], rcalls), ("one-parameter handle", c))
        assert sum(r.size for r in row) > 0, c


def test_bitstream_bank_through_the_arena_and_reset(ctx, symbols):
    """process() inside the red-zoned arena (rows of the LARGEST capacity, guard bands between them), then reset: fresh nodes."""
    sched = _bits_schedules(False)
    bank = sa.BitStreamBank(ctx, FS, [b for b, _ in BIT_ROWS], [m for _, m in BIT_ROWS], max_in=700)
    from redzone import RedZone
    calls0 = RedZone.calls
    bank.process(symbols[:, 2000:2700])
    assert RedZone.active and RedZone.calls > calls0
    bank.reset()
    calls = _calls(symbols[:, :958], [257, 0, 700, 1])
    got = [bank.process(x) for x in calls]
    for c in range(6):
        _same([g[c] for g in got], _row(_ref_bits_node, sched[c], [x[c] for x in calls]), ("after reset", c))


@pytest.mark.hostptr_only
def test_host_pointer_calls_across_a_set_channel_to_a_faster_baud_rate(ctx, audio, symbols):
    """sdrhip_bits_process / sdrhip_detector_process on per-channel handles (outside the arena: the library's own staging).
    Row 0 goes from 90.90 to 2400 baud between two calls: the bank's capacity grows past what the first call staged for, the
    rows come back at the new pitch, row 0 is a fresh node and row 1 streams on; bytes behind a row's count arrive as zeros."""
    assert sa.nodes.device_router is None
    n = 700
    cfgs = [(90.90, N), (512.0, N)]
    bank = sa.BitStreamBank(ctx, FS, [b for b, _ in cfgs], [m for _, m in cfgs], max_in=n)
    sym = symbols[[2, 3]]
    calls = [sym[:, :n], sym[:, n:2 * n], sym[:, 2 * n:2 * n + 257], sym[:, 2 * n + 257:3 * n + 257]]
    sched = [[(0, cfgs[0]), (2, (2400.0, T))], [(0, cfgs[1])]]
    caps, got = [], []
    for k, x in enumerate(calls):
        if k == 2:
            bank.set_channel(0, 2400.0, T)
        caps.append(bank.out_capacity(n))
        out, cnt = bank.process_raw(x)
        assert out.shape == (2, bank.out_capacity(x.shape[1]))
        for c in range(2):
            assert not out[c, cnt[c]:].any(), (k, c)
        got.append([out[c, :cnt[c]].copy() for c in range(2)])
    assert caps[0] == caps[1] == fr.BitStream(FS, 512.0, N).capacity(n) and caps[2] == caps[3] == fr.BitStream(FS, 2400.0, T).capacity(n)
    assert caps[2] > 3 * caps[0]
    for c in range(2):
        row, rcalls = [g[c] for g in got], [x[c] for x in calls]
        _same(row, _row(_ref_bits_node, sched[c], rcalls), ("restatement", c))
        _same(row, _row(lambda cfg: _gpu_bits_node(ctx, cfg, n), sched[c], rcalls), ("one-parameter handle", c))
    assert sum(g[0].size for g in got[2:]) > caps[0]          # row 0 did use the room beyond the first staging
    # the detector bank through sdrhip_detector_process, a set_channel between the calls
    chans, dsched = _det_schedules(True)
    det = sa.SymbolDetectorBank(ctx, chans, max_in=max(LENS), max_corr_len=300)
    dcalls = _calls(audio[:, :sum(LENS)], LENS)
    dgot = []
    for k, x in enumerate(dcalls):
        for c in range(8):
            for at, cfg in dsched[c][1:]:
                if at == k:
                    det.set_channel(c, cfg)
        dgot.append(det.process(x))
    for c in range(8):
        _same([g[c] for g in dgot], _row(_ref_det_node, dsched[c], [x[c] for x in dcalls]), ("host pointers", c))


# ---- one-parameter handles keep their kernels and refuse set_channel ------------------------------------------------------------
@pytest.mark.hostptr_only
def test_kernel_names_and_one_parameter_handles(ctx):
    lm, ls = sa.design_fsk_lut(FS, 1200.0, 1200.0), sa.design_fsk_lut(FS, 1200.0, 2200.0)
    det = sa.SymbolDetector(ctx, sa.DET_FSK, lm, ls, channels=2, max_in=16)
    ask = sa.ASKDetector(ctx, channels=2, max_in=16)
    bits = sa.BitStream(ctx, FS, 1200.0, T, channels=2, max_in=16)
    assert det.kernel_names == ["fsk_detect_kernel"] and ask.kernel_names == ["ask_detect_kernel"]
    assert bits.kernel_names == ["bits_pll_kernel", "bits_flags_kernel"]
    L = sa.abi.lib()
    f32p = C.POINTER(C.c_float)
    p = lm.ctypes.data_as(f32p)
    assert L.sdrhip_detectorbank_set_channel(det._h, 0, sa.DET_FSK, p, p, 18, 0) == sa.abi.E_UNSUPPORTED
    assert L.sdrhip_bitsbank_set_channel(bits._h, 0, 1200.0, N) == sa.abi.E_UNSUPPORTED
    assert L.sdrhip_bitsbank_channel_info(bits._h, 0, 16, None, None, None, None) == sa.abi.E_UNSUPPORTED
    # a per-channel handle: a refused set_channel changes nothing
    bank = sa.SymbolDetectorBank(ctx, [("fsk", lm, ls), ("ask", False)], max_in=64, max_corr_len=20)
    big = sa.design_fsk_lut(FS, 1000.0, 1200.0)          # L = 22 > max_corr_len
    for bad in (lambda: bank.set_channel(2, ("ask", False)), lambda: bank.set_channel(-1, ("ask", False))):
        with pytest.raises(sa.SdrHipError) as e:
            bad()
        assert e.value.code == sa.abi.E_INVALID and "outside [0,2)" in str(e.value), str(e.value)
    with pytest.raises(sa.SdrHipError):
        bank.set_channel(0, ("fsk", big, big))
    assert L.sdrhip_detectorbank_set_channel(bank._h, 0, 7, p, p, 18, 0) == sa.abi.E_INVALID
    assert L.sdrhip_detectorbank_set_channel(bank._h, 0, sa.DET_FSK, p, p, 0, 0) == sa.abi.E_INVALID
    assert L.sdrhip_detectorbank_set_channel(bank._h, 0, sa.DET_FSK, p, p, 21, 0) == sa.abi.E_UNSUPPORTED
    assert L.sdrhip_detectorbank_set_channel(bank._h, 0, sa.DET_FSK, None, p, 18, 0) == sa.abi.E_INVALID
    bb = sa.BitStreamBank(ctx, FS, [1200.0, 2400.0], [N, T], max_in=64)
    before = [bb.channel_info(c, 64) for c in range(2)]
    for baud, mode, want in ((1200.0, 5, sa.abi.E_INVALID), (0.0, N, sa.abi.E_INVALID), (30000.0, N, sa.abi.E_INVALID),
                             (1000.0, N, sa.abi.E_UNSUPPORTED)):       # (1000 baud: L = 22 > the bank's 18)
        assert L.sdrhip_bitsbank_set_channel(bb._h, 1, baud, mode) == want, (baud, mode)
    assert L.sdrhip_bitsbank_set_channel(bb._h, 2, 1200.0, N) == sa.abi.E_INVALID
    assert [bb.channel_info(c, 64) for c in range(2)] == before
    x = (np.arange(2 * 64, dtype=np.int16).reshape(2, 64) - 40) * np.int16(97)
    want = [fr.FSKDetector(lm, ls).process(x[:1])[0], fr.ask_detect(x[1], False)]
    s = bank.process(x)
    assert np.array_equal(s[0], want[0]) and np.array_equal(s[1], want[1])


@pytest.mark.hostptr_only
def test_the_bitstream_banks_row_calls_refuse_a_row_outside_the_bank(ctx, symbols):
    """The smallest bank that has two rows to tell apart: 2 rows, max_in 64, one call each. Rows -1 and 2 are refused by
    set_channel and channel_info with the range in the message and nothing changed; a set_channel that succeeds leaves row 0
    as it is in a bank never touched."""
    n, cfgs = 64, [(1200.0, N), (2400.0, T)]
    bank, twin = (sa.BitStreamBank(ctx, FS, [b for b, _ in cfgs], [m for _, m in cfgs], max_in=n) for _ in range(2))
    before = [bank.channel_info(c, n) for c in range(2)]
    for c in (-1, 2):
        for call in (lambda: bank.set_channel(c, 1200.0, N), lambda: bank.channel_info(c, n)):
            with pytest.raises(sa.SdrHipError) as e:
                call()
            assert e.value.code == sa.abi.E_INVALID and "outside [0,2)" in str(e.value), (c, str(e.value))
    assert [bank.channel_info(c, n) for c in range(2)] == before
    sym = symbols[[0, 4]]
    calls = [sym[:, :n], sym[:, n:2 * n]]
    sched = [[(0, cfgs[0])], [(0, cfgs[1]), (1, (1200.0, T))]]
    got, und = [], []
    for k, x in enumerate(calls):
        if k == 1:
            bank.set_channel(1, 1200.0, T)
        for node, rows in ((bank, got), (twin, und)):
            out, cnt = node.process_raw(x)
            rows.append([out[c, :cnt[c]].copy() for c in range(2)])
    for c in range(2):
        _same([g[c] for g in got], _row(_ref_bits_node, sched[c], [x[c] for x in calls]), ("restatement", c))
    _same(got[0], und[0], "the refused calls changed nothing")
    _same([got[1][0]], [und[1][0]], "row 0 streamed on")
    assert sum(g[0].size for g in got) > 0
    bank.close()
    twin.close()


# ---- the chain on device pointers: modes bank -> detector bank -> BitStream bank -------------------------------------------------
@pytest.mark.hostptr_only
def test_chain_from_the_modes_bank_on_device_pointers(ctx):
    """4 channels, 127 taps, /8, 2048 samples per call, FM / AM / USB mixed: the audio rows never leave the device between the
    three banks; every row equals the same chain built from one-parameter handles for that row alone — a one-channel IQBaseBand plan with the
    row's tune and demodulator on the same input, then a one-parameter detector and BitStream."""
    CH, order, D, n_in, ncalls = 4, 127, 8, 2048, 3
    Fs_in = FS * D
    r = np.random.default_rng(11)
    n = n_in * ncalls
    fc = [20e3, -35e3, 50e3, -8e3]
    t = np.arange(n)
    x = np.zeros(n, np.complex128)
    for c in range(CH):
        key = np.repeat(r.integers(0, 2, n // 147 + 2), 147)[:n]
        tone = np.sin(2 * np.pi * np.cumsum(np.where(key, 2200.0, 1200.0) / Fs_in))
        x += 5000 * (0.3 + 0.7 * key * (c % 2) + (1 - c % 2)) * np.exp(2j * np.pi * (fc[c] * t / Fs_in + np.cumsum(3000.0 * tone / Fs_in)))
    x = np.stack([x.real, x.imag], axis=1) + r.normal(0, 200, (n, 2))
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    taps = np.stack([np.asarray(sa.design_iqbb_taps(f, 12e3, Fs_in, order), np.int32).reshape(-1, 2) for f in fc])
    inc = [sa.design_freqshift_inc(f, Fs_in) for f in fc]
    modes = [sa.EPI_FM, sa.EPI_AM, sa.EPI_USB, sa.EPI_FM]
    tuner = sa.TunerBankI16(ctx, taps, sa.design_freqshift_lut_i16(), inc, [f < 0 for f in fc], D, max_in=n_in, modes=modes)
    M = n_in // D + 2
    det_cfg = [_fsk(*AX25, 18), ("ask", False), _fsk(*RTTY, 242), ("ask", True)]
    bit_cfg = [(1200.0, T), (512.0, N), (90.90, N), (1200.0, N)]
    det = sa.SymbolDetectorBank(ctx, det_cfg, max_in=M)
    bits = sa.BitStreamBank(ctx, FS, [b for b, _ in bit_cfg], [m for _, m in bit_cfg], max_in=M)
    cap = bits.out_capacity(M)
    din, dau, dsym, dbits, dcnt = (ctx.malloc(b) for b in (n_in * 4, CH * M * 2, CH * M, CH * cap, 4 * CH))
    lut = sa.design_freqshift_lut_i16()
    rtune = [sa.IQBaseBandI16(ctx, taps[c], lut, inc[c], fc[c] < 0, D, channels=1, max_in=n_in, epilogue=modes[c]) for c in range(CH)]
    rdet = [_gpu_det_node(ctx, cfg, M) for cfg in det_cfg]
    rbits = [_gpu_bits_node(ctx, cfg, M) for cfg in bit_cfg]
    total = 0
    try:
        for k in range(ncalls):
            ctx.h2d(din, x[k * n_in:(k + 1) * n_in])
            no = tuner.process_dev(din, n_in, dau, M)
            assert 0 < no <= M
            det.process_dev(dau, no, M, dsym, M)
            bits.process_dev(dsym, no, M, dbits, cap, dcnt)
            ctx.synchronize()
            au, sym, out, cnt = np.zeros((CH, M), np.int16), np.zeros((CH, M), np.uint8), np.zeros((CH, cap), np.uint8), np.zeros(CH, np.uint32)
            ctx.d2h(au, dau); ctx.d2h(sym, dsym); ctx.d2h(out, dbits); ctx.d2h(cnt, dcnt)
            for c in range(CH):
                wa = rtune[c].process(x[None, k * n_in:(k + 1) * n_in])[0]
                assert wa.shape == (no,) and np.array_equal(au[c, :no], wa), (k, c)
                ws = rdet[c](wa)
                assert np.array_equal(sym[c, :no], ws), (k, c)
                wb = rbits[c](ws)
                assert cnt[c] == wb.size and np.array_equal(out[c, :cnt[c]], wb), (k, c)
            total += int(cnt.sum())
            assert au.any(axis=1).all()
    finally:
        for p in (din, dau, dsym, dbits, dcnt):
            ctx.free(p)
    assert total > 0
