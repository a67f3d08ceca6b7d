"""GPU parity of the symbol path (sdrhip_detector_*, sdrhip_bits_*): the g18 fixtures cut from the reference and the numpy
restatement (tests/fsk_restatement.py) at shapes no fixture covers. The contract is bit-exact: zero differing symbols, zero
differing bits, identical counts; no tolerance, no skip list. The module name makes tests/conftest.py run every process()
call inside the red-zoned device arena (device-pointer entry points, row strides larger than n); cases marked
`hostptr_only` go through the host-pointer entry points instead."""
import numpy as np
import pytest

import fsk_restatement as fr
import libsdr_amd as sa
from test_fsk_restatement import G18, split

pytestmark = pytest.mark.gpu

ROUTES = [pytest.param("dev", id="dev"), pytest.param("host", id="host", marks=pytest.mark.hostptr_only)]
MODE = {"normal": sa.BITS_NORMAL, "transition": sa.BITS_TRANSITION}


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g18():
    return G18()


def _routed(route):
    from redzone import RedZone
    assert RedZone.active == (route == "dev")
    return RedZone.calls


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mode", ["normal", "transition"])
@pytest.mark.parametrize("case", ["g18_ax25", "g18_rtty", "g18_reconf"])
def test_fsk_fixture(ctx, g18, case, mode, route):
    calls0 = _routed(route)
    m = g18.meta(case + "_x")
    x, lens = g18.load(case + "_x"), m["lens"]
    det = sa.FSKDetector(ctx, m["Fs"], m["baud"], m["Fmark"], m["Fspace"], channels=1, max_in=max(lens),
                         mark_lut=g18.load(case + "_lut_mark"), space_lut=g18.load(case + "_lut_space"))
    bits = sa.BitStream(ctx, m["Fs"], m["baud"], MODE[mode], channels=1, max_in=max(lens))
    assert det.kernel_names == ["fsk_detect_kernel"] and bits.kernel_names == ["bits_pll_kernel", "bits_flags_kernel"]
    assert bits.corr_len == m["corr_len"]
    sym, out, counts = [], [], []
    for b, buf in enumerate(split(x, lens)):
        if b == m["reconf_at"]:
            det.reset()
            bits.reset()
        s = det.process(buf)
        o = bits.process(s)[0]
        sym.append(s[0])
        out.append(o)
        counts.append(o.size)
    sym, out = np.concatenate(sym), np.concatenate(out)
    want_sym, want = g18.load(case + "_sym"), g18.load("%s_bits_%s" % (case, mode))
    assert sym.size == want_sym.size and int((sym != want_sym).sum()) == 0
    assert counts == list(g18.load("%s_bits_%s_counts" % (case, mode)))
    assert out.size == want.size and int((out != want).sum()) == 0
    if route == "dev":
        from redzone import RedZone
        assert RedZone.calls > calls0


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("inv", [0, 1])
def test_ask_fixture(ctx, g18, inv, route):
    _routed(route)
    m = g18.meta("g18_ask_x")
    x, lens = g18.load("g18_ask_x"), m["lens"]
    det = sa.ASKDetector(ctx, invert=bool(inv), channels=1, max_in=max(lens))
    bits = sa.BitStream(ctx, m["Fs"], m["baud"], sa.BITS_NORMAL, channels=1, max_in=max(lens))
    assert det.kernel_names == ["ask_detect_kernel"]
    sym, out = [], []
    for buf in split(x, lens):
        s = det.process(buf)
        sym.append(s[0])
        out.append(bits.process(s)[0])
    assert np.array_equal(np.concatenate(sym), g18.load("g18_ask_inv%d_sym" % inv))
    assert [o.size for o in out] == list(g18.load("g18_ask_inv%d_bits_normal_counts" % inv))
    assert np.array_equal(np.concatenate(out), g18.load("g18_ask_inv%d_bits_normal" % inv))


def _audio(C, n, Fs, baud, f0, f1, seed):
    """Different data per channel: keyed tones of different amplitudes plus noise, a silent stretch, full-scale samples."""
    r = np.random.default_rng(seed)
    key = np.repeat(r.integers(0, 2, (C, n // max(int(Fs / baud), 1) + 2)), max(int(Fs / baud), 1), axis=1)[:, :n]
    ph = 2 * np.pi * np.cumsum(np.where(key, f1, f0) / Fs, axis=1)
    x = r.uniform(2000, 14000, (C, 1)) * np.sin(ph + r.uniform(0, 6, (C, 1))) + r.normal(0, 1500, (C, n))
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    if n > 900:
        x[:, 300:300 + 260] = 0
        x[:, 700:760] = np.where(r.integers(0, 2, (C, 60)) > 0, 32767, -32768)
    return x


@pytest.mark.parametrize("C", [1, 3, 64, 1024])
@pytest.mark.parametrize("L", [2, 18, 64, 65, 242])
def test_detector_and_bits_against_restatement(ctx, C, L):
    """Ragged sequences of 0, 1, L-1, L, L+1 and 8192 samples with a reset in between, different data per channel, both
    BitStream modes (by L's parity), the same LUT arrays on both sides."""
    baud = 1200.0
    Fs = baud * L + 600.0
    assert fr.corr_len(Fs, baud) == L
    lm, ls = sa.design_fsk_lut(Fs, baud, 1200.0), sa.design_fsk_lut(Fs, baud, 2200.0)
    assert lm.shape == (L, 2)
    mode = fr.TRANSITION if L & 1 else fr.NORMAL
    big = 8192 if (C < 1024 or L <= 65) else 2048     # (the restatement's memory at 1024 channels x 242 slots)
    lens = [1, 0, L - 1, L, L + 1, big, 1, "reset", L + 1, 0, 777, L - 1, big // 2 + 3]
    det = sa.SymbolDetector(ctx, sa.DET_FSK, lm, ls, channels=C, max_in=8192)
    bits = sa.BitStream(ctx, Fs, baud, mode, channels=C, max_in=8192)
    rdet, rbits = fr.FSKDetector(lm, ls, channels=C), fr.BitStream(Fs, baud, mode, channels=C)
    assert bits.corr_len == L
    total = 0
    for k, n in enumerate(lens):
        if n == "reset":
            det.reset(); bits.reset(); rdet.reset(); rbits.reset()
            continue
        x = _audio(C, n, Fs, baud, 1200.0, 2200.0, 1000 * L + 10 * C + k)
        s = det.process(x)
        ws = rdet.process(x)
        assert s.shape == ws.shape and int((s != ws).sum()) == 0, (C, L, k, n, np.argwhere(s != ws)[:4])
        raw, counts = bits.process_raw(s)
        want = rbits.process(ws)
        assert list(counts) == [w.size for w in want], (C, L, k, n)
        assert int(counts.max(initial=0)) <= bits.out_capacity(n) == rbits.capacity(n)
        for c in range(C):
            assert np.array_equal(raw[c, :counts[c]], want[c]), (C, L, k, n, c)
        total += int(counts.sum())
    assert total > 0


def test_all_zero_input_and_quiet_channels(ctx):
    """All-zero rows give f == 0, symbol 0 (src/fsk.cc:86), beside live rows; BitStream on constant symbols."""
    Fs, baud, L, C, n = 22050.0, 1200.0, 18, 5, 4000
    lm, ls = sa.design_fsk_lut(Fs, baud, 1200.0), sa.design_fsk_lut(Fs, baud, 2200.0)
    x = _audio(C, n, Fs, baud, 1200.0, 2200.0, 7)
    x[1] = 0
    x[3] = 0
    det, rdet = sa.SymbolDetector(ctx, sa.DET_FSK, lm, ls, channels=C, max_in=n), fr.FSKDetector(lm, ls, channels=C)
    s = det.process(x)
    assert np.array_equal(s, rdet.process(x)) and not s[1].any() and not s[3].any() and s[0].any()
    for mode in (fr.NORMAL, fr.TRANSITION):
        bits, rbits = sa.BitStream(ctx, Fs, baud, mode, channels=C, max_in=n), fr.BitStream(Fs, baud, mode, channels=C)
        got, want = bits.process(s), rbits.process(s)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and [g.size for g in got] == [w.size for w in want]


@pytest.mark.parametrize("invert", [False, True])
def test_ask_against_restatement(ctx, invert):
    r = np.random.default_rng(3)
    C = 64
    det = sa.ASKDetector(ctx, invert=invert, channels=C, max_in=8192)
    for n in (0, 1, 17, 8192, 255, 256, 257):
        x = r.integers(-3, 4, (C, n)).astype(np.int16) * r.integers(0, 9000, (C, 1)).astype(np.int16)
        assert np.array_equal(det.process(x), fr.ask_detect(x, invert))


@pytest.mark.hostptr_only
def test_explicit_device_pointers_and_strides(ctx):
    """process_dev on caller-owned device memory with row strides larger than n on every buffer; the bytes between the rows
    stay untouched; the output may not overlap the input."""
    Fs, baud, L, C, n, si, so = 22050.0, 1200.0, 18, 3, 1000, 1111, 1203
    lm, ls = sa.design_fsk_lut(Fs, baud, 1200.0), sa.design_fsk_lut(Fs, baud, 2200.0)
    x = _audio(C, n, Fs, baud, 1200.0, 2200.0, 11)
    det = sa.SymbolDetector(ctx, sa.DET_FSK, lm, ls, channels=C, max_in=n)
    bits = sa.BitStream(ctx, Fs, baud, sa.BITS_TRANSITION, channels=C, max_in=n)
    cap = bits.out_capacity(n)
    sb = cap + 9
    din, dsym, dbits, dcnt = ctx.malloc(C * si * 2), ctx.malloc(C * so), ctx.malloc(C * sb), ctx.malloc(4 * C)
    try:
        full = np.zeros((C, si), np.int16)
        full[:, :n] = x
        ctx.h2d(din, full)
        ctx.memset(dsym, 0x5a, C * so)
        ctx.memset(dbits, 0x5a, C * sb)
        det.process_dev(din, n, si, dsym, so)
        bits.process_dev(dsym, n, so, dbits, sb, dcnt)
        ctx.synchronize()
        sym, out, cnt = np.zeros((C, so), np.uint8), np.zeros((C, sb), np.uint8), np.zeros(C, np.uint32)
        ctx.d2h(sym, dsym); ctx.d2h(out, dbits); ctx.d2h(cnt, dcnt)
        ws = fr.FSKDetector(lm, ls, channels=C).process(x)
        want = fr.BitStream(Fs, baud, fr.TRANSITION, channels=C).process(ws)
        assert np.array_equal(sym[:, :n], ws) and (sym[:, n:] == 0x5a).all()
        for c in range(C):
            assert cnt[c] == want[c].size and np.array_equal(out[c, :cnt[c]], want[c]) and (out[c, cnt[c]:] == 0x5a).all()
        with pytest.raises(sa.SdrHipError):
            det.process_dev(din, n, si, din + 100, so)
        with pytest.raises(sa.SdrHipError):
            bits.process_dev(dsym, n, so, dbits, cap - 1, dcnt)
        bits.process_dev(dsym, 0, so, dbits, sb, dcnt)          # an empty call: counts 0, nothing else happens
        ctx.synchronize()
        ctx.d2h(cnt, dcnt)
        assert not cnt.any()
    finally:
        for p in (din, dsym, dbits, dcnt):
            ctx.free(p)


@pytest.mark.parametrize("mode", [fr.NORMAL, fr.TRANSITION])
def test_output_capacity_when_fs_over_baud_is_nearly_an_integer(ctx, mode):
    """Fs / baud = 18.01 (0.06 % above an integer): symbols that flip slightly faster than the nominal rate drive the PLL to
    its upper limit, where a call emits more bits than the reference's own buffer size 1 + n / corrLen; the product's
    capacity ceil(n omegaMax) + 1 holds them."""
    baud, C, n = 1200.0, 4, 8192
    Fs = baud * 18.01
    bits, rbits = sa.BitStream(ctx, Fs, baud, mode, channels=C, max_in=n), fr.BitStream(Fs, baud, mode, channels=C)
    assert bits.corr_len == 18 and bits.out_capacity(n) == rbits.capacity(n) > 1 + n // 18
    t = np.arange(3 * n)
    sym = np.stack([((t / p).astype(np.int64) & 1).astype(np.uint8) for p in (17.8, 17.9, 18.0, 18.2)])
    over = 0
    for k in range(3):
        raw, counts = bits.process_raw(sym[:, k * n:(k + 1) * n])
        want = rbits.process(sym[:, k * n:(k + 1) * n])
        assert list(counts) == [w.size for w in want] and int(counts.max()) <= bits.out_capacity(n)
        for c in range(C):
            assert np.array_equal(raw[c, :counts[c]], want[c])
        over += int((counts > 1 + n // 18).sum())
    assert over > 0   # the case does exceed the reference's buffer size


@pytest.mark.hostptr_only
def test_device_resident_chain_to_bits(ctx, orc):
    """IQBaseBand(FM epilogue) -> FMDeemph -> FSKDetector -> BitStream on 64 channels, every stage on device pointers (the only
    copies are the input upload and the final read-back), against the oracle front end feeding the restatement."""
    C, N, D, calls = 64, 16384, 8, 3
    Fs = 22050.0 * D
    baud, f0, f1 = 1200.0, 1200.0, 2200.0
    r = np.random.default_rng(5)
    n = calls * N
    key = np.repeat(r.integers(0, 2, (C, n // 147 + 2)), 147, axis=1)[:, :n]            # 1200 baud at 176.4 kS/s
    audio = np.sin(2 * np.pi * np.cumsum(np.where(key, f1, f0) / Fs, axis=1))
    phase = 2 * np.pi * np.cumsum(3000.0 * audio / Fs, axis=1) + 2 * np.pi * 10e3 * np.arange(n) / Fs
    x = np.stack([np.rint(9000 * np.cos(phase)), np.rint(9000 * np.sin(phase))], axis=2) + r.normal(0, 300, (C, n, 2))
    x = np.clip(x, -32768, 32767).astype(np.int16)
    taps, lut, inc = sa.design_iqbb_taps(10e3, 12e3, Fs, 127), sa.design_freqshift_lut_i16(), sa.design_freqshift_inc(10e3, Fs)
    oFs = Fs / D
    alpha = sa.design_fmdeemph_alpha(oFs)
    lm, ls = sa.design_fsk_lut(oFs, baud, f0), sa.design_fsk_lut(oFs, baud, f1)
    bb = sa.IQBaseBandI16(ctx, taps, lut, inc, False, D, channels=C, max_in=N, epilogue=sa.EPI_FM)
    de = sa.FMDeemphI16(ctx, alpha, channels=C, max_in=N // D)
    det = sa.SymbolDetector(ctx, sa.DET_FSK, lm, ls, channels=C, max_in=N // D)
    bits = sa.BitStream(ctx, oFs, baud, sa.BITS_TRANSITION, channels=C, max_in=N // D)
    assert det.kernel_names == ["fsk_detect_kernel"] and bits.kernel_names == ["bits_pll_kernel", "bits_flags_kernel"]
    M = N // D
    cap = bits.out_capacity(M)
    din, dfm, dau, dsym, dbits, dcnt = (ctx.malloc(b) for b in (C * N * 4, C * M * 2, C * M * 2, C * M, C * cap, 4 * C))
    refs = [(orc.IQBaseBandI16(taps, lut, inc, False, D), orc.FMDemodI16(), orc.FMDeemphI16(oFs)) for _ in range(C)]
    rdet, rbits = fr.FSKDetector(lm, ls, channels=C), fr.BitStream(oFs, baud, fr.TRANSITION, channels=C)
    try:
        total = 0
        for k in range(calls):
            ctx.h2d(din, x[:, k * N:(k + 1) * N])
            no = bb.process_dev(din, N, N, dfm, M)
            de.process_dev(dfm, no, M, dau, M)
            det.process_dev(dau, no, M, dsym, M)
            bits.process_dev(dsym, no, M, dbits, cap, dcnt)
            ctx.synchronize()
            out, cnt = np.zeros((C, cap), np.uint8), np.zeros(C, np.uint32)
            ctx.d2h(out, dbits); ctx.d2h(cnt, dcnt)
            au = np.stack([dm.process(fm.process(b.process(x[c, k * N:(k + 1) * N]))) for c, (b, fm, dm) in enumerate(refs)])
            assert au.shape == (C, no)
            want = rbits.process(rdet.process(au))
            assert list(cnt) == [w.size for w in want], k
            for c in range(C):
                assert np.array_equal(out[c, :cnt[c]], want[c]), (k, c)
            total += int(cnt.sum())
        assert total > C * 100   # the channels do carry bits
    finally:
        for p in (din, dfm, dau, dsym, dbits, dcnt):
            ctx.free(p)


@pytest.mark.hostptr_only
def test_argument_errors(ctx):
    lm = sa.design_fsk_lut(22050.0, 1200.0, 1200.0)
    with pytest.raises(sa.SdrHipError):
        sa.SymbolDetector(ctx, 7, lm, lm)
    with pytest.raises(sa.SdrHipError):
        sa.SymbolDetector(ctx, sa.DET_FSK, np.zeros((4000, 2), np.float32), np.zeros((4000, 2), np.float32))
    with pytest.raises(sa.SdrHipError):
        sa.BitStream(ctx, 22050.0, 1200.0, 5)
    with pytest.raises(sa.SdrHipError):
        sa.BitStream(ctx, 600.0, 1200.0, sa.BITS_NORMAL)
    det = sa.SymbolDetector(ctx, sa.DET_FSK, lm, lm, channels=2, max_in=16)
    with pytest.raises(sa.SdrHipError):
        det.process(np.zeros((2, 17), np.int16))
