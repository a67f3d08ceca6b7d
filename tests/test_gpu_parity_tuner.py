"""GPU parity of the tuner bank (sdrhip_tuner_i16_*, TunerBankI16): C IQBaseBand<int16_t> channels over ONE input row.
Every comparison is bit for bit: rows pinned to the golden vectors cut from the compiled reference, every row against the
CPU oracle's node restated per channel. Every test runs under both kernel forms (the matrix form where the plan has one, and
SDRHIP_TUNER_PATH=valu) and, as every module of the parity family, inside the red-zoned device arena (tests/redzone.py:
guard bands around the ONE input row and between the output rows, which therefore have a stride larger than n_out);
tests marked hostptr_only go through the library's own staging instead.
Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import libsdr_amd as sa

try:   # torch brings its own HIP runtime: it only finds the GPU when it initialises before libsdrhip.so does
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()
except Exception:   # pragma: no cover
    torch = None

from hot_classes import BOUNDARY

pytestmark = pytest.mark.gpu

FS = 2.4e6
EPIS = {"none": sa.EPI_NONE, "fm": sa.EPI_FM, "am": sa.EPI_AM, "usb": sa.EPI_USB}
HOT, VALU = "tuner_i16_mfma_kernel", "tuner_i16_valu_kernel"


def split(x, lens):
    out, off = [], 0
    for n in lens:
        out.append(x[off:off + n])
        off += n
    return out


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["auto", "valu"])
def form(request, monkeypatch):
    monkeypatch.delenv("SDRHIP_TUNER_PATH", raising=False)
    if request.param == "valu":
        monkeypatch.setenv("SDRHIP_TUNER_PATH", "valu")
    return request.param


def tune(Fc, Ff, width, order, Fs=FS):
    return sa.design_iqbb_taps(Ff, width, Fs, order), sa.design_freqshift_inc(Fc, Fs), Fc < 0


def other_tunes(n, order, seed, Fs=FS):
    """n tunes that differ from each other and from the fixtures': both signs of Fc, one unshifted."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        Fc = 0.0 if i == 1 else (float(rng.integers(-500, 500)) * 1e3 + 7e3) * Fs / FS
        out.append(tune(Fc, Fc, float(rng.integers(10, 120)) * 1e3 * Fs / FS, order, Fs))
    return out


class Ref:
    """The oracle's node (+ demodulator) of one channel."""

    def __init__(self, orc, taps, lut, inc, neg, D, epi):
        self.orc, self.epi = orc, epi
        self.bb = orc.IQBaseBandI16(taps, lut, inc, neg, D)
        self.fm = orc.FMDemodI16()

    def process(self, x):
        y = self.bb.process(x)
        if self.epi == sa.EPI_FM:
            return self.fm.process(y)
        if self.epi == sa.EPI_AM:
            return self.orc.am_i16(y)
        if self.epi == sa.EPI_USB:
            return self.orc.usb_i16(y)
        return y


def make_bank(ctx, tunes, D, epi, max_in, cu8=False):
    lut = sa.design_freqshift_lut_i16()
    taps = np.stack([np.asarray(t[0], np.int32).reshape(-1, 2) for t in tunes])
    bank = sa.TunerBankI16(ctx, taps, lut, [t[1] for t in tunes], [t[2] for t in tunes], D, max_in=max_in, epilogue=epi)
    if cu8:
        bank.set_input_format(sa.abi.IN_CU8)
    return bank, lut


def make_refs(orc, tunes, lut, D, epi):
    return [Ref(orc, t[0], lut, t[1], t[2], D, epi) for t in tunes]


def check_names(bank, form, hot_possible):
    names = bank.kernel_names
    assert all(n.startswith("tuner_") and "iqbb_hot" not in n for n in names), names
    assert names == ([HOT] if form == "auto" and hot_possible else [VALU]), (names, form)


# ---- 1. rows pinned to the compiled reference -------------------------------------------------------------------------------

# (fixtures of one bank: equal order, decimation, epilogue and input), input, cu8
GOLDEN_BANKS = [
    (["g3_iqbb127d8_out"], "g1_iq_cs16", False),
    (["g4_iqbb127d8_fm"], "g1_iq_cs16", False), (["g4_iqbb127d8_am"], "g1_iq_cs16", False), (["g4_iqbb127d8_usb"], "g1_iq_cs16", False),
    (["g8_o255_d8_out"], "g1_iq_cs16", False), (["g8_noshift_o21_d8_out"], "g1_iq_cs16", False),
    (["g8_o21_d3_out"], "g1_iq_cs16", False), (["g8_o33_d5_out"], "g1_iq_cs16", False), (["g8_o33_d5_fm"], "g1_iq_cs16", False),
    (["g8_o16_d4_even_out"], "g1_iq_cs16", False), (["g8_ofs_d300_out"], "g1_iq_cs16", False),
    (["g8_irregular_out", "g3_iqbb127d8_out"], "g1_iq_cs16", False),   # (the same tune: two rows of one bank, ragged calls)
    (["g8_irregular_fm"], "g1_iq_cs16", False), (["g8_irregular_usb"], "g1_iq_cs16", False),
    (["g8_neg_o16_d1_out"], "g1_iq_cs16_tone_m100k", False),
    (["g8_loud_iqbb127d8_fm"], "g8_iq_cs16_loud", False), (["g8_loud_iqbb127d8_am"], "g8_iq_cs16_loud", False),
    (["g9_cu8_iqbb21d8_fm"], "g9_iq_cu8", True), (["g9_cu8_iqbb127d8_fm"], "g9_iq_cu8", True),
]


def _fixture_tune(golden, name):
    """(taps, inc, negative, order, D, epilogue, in_lens) of a golden output."""
    m = golden.meta(name)
    base, kind = name.rsplit("_", 1)
    epi = EPIS["none" if kind == "out" else kind]
    if name.startswith("g9_cu8"):
        mt = golden.meta(base + "_taps")
        taps = golden.load(base + "_taps")
        return (taps, mt["lut_inc"], False), np.asarray(taps).reshape(-1, 2).shape[0], 8, epi, [4096] * 3
    tcase = base if (base + "_taps") in golden.manifest else "g3_iqbb127d8"
    tm = golden.meta(name) if "lut_inc" in m else golden.meta(tcase + "_out")
    return (golden.load(tcase + "_taps"), tm["lut_inc"], bool(tm["negative"])), tm["order"], tm["decim"], epi, m["in_lens"]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("names,inp,cu8", GOLDEN_BANKS, ids=[b[0][0] for b in GOLDEN_BANKS])
def test_tuner_rows_pinned_to_reference(ctx, golden, names, inp, cu8, where, form):
    fx = [_fixture_tune(golden, n) for n in names]
    (_, order, D, epi, in_lens) = fx[0]
    assert all(f[1:4] == (order, D, epi) for f in fx)
    Fs = 1e6 if cu8 else FS
    tunes = other_tunes(5 - len(fx), order, seed=order + D, Fs=Fs)
    pos = {"first": 0, "middle": 2, "last": 5 - len(fx)}[where]
    rows = list(range(pos, pos + len(fx)))
    for f in reversed(fx):
        tunes.insert(pos, f[0])
    # (the second fixture of a two-row bank was cut with equal calls: both rows see the first one's ragged calls, and the
    # concatenated baseband output does not depend on how the stream is cut)
    bank, _ = make_bank(ctx, tunes, D, epi, max_in=4096, cu8=cu8)
    x = golden.load(inp).reshape(-1, 2)
    outs = [bank.process(c) for c in split(x, in_lens)]
    check_names(bank, form, D >= 4 and [n for n in in_lens if n][-1] >= 512)
    for r, name in zip(rows, names):
        got = [o[r] for o in outs]
        if epi == sa.EPI_FM:   # FMDemod does not send on an empty buffer
            got = [o for o in got if len(o)]
        if name == names[0]:
            assert [len(o) for o in got] == golden.meta(name)["out_lens"]
        want = golden.load(name)
        assert np.array_equal(np.concatenate(got), want if epi != sa.EPI_NONE else want.reshape(-1, 2)), (name, r)
    # the other rows carry other tunes: none of them repeats the fixture row
    whole = [np.concatenate([o[r] for o in outs]) for r in range(5)]
    assert all(not np.array_equal(whole[r], whole[rows[0]]) for r in range(5) if r not in rows)


# ---- 2. every row against the oracle ------------------------------------------------------------------------------------

AX_C = [1, 2, 31, 32, 33, 64, 257, 1024]
AX_ORDER = [1, 16, 21, 127, 128, 255, 300, 513]
AX_D = [1, 3, 8, 20, 125, 512]
AX_EPI = ["none", "fm", "am", "usb"]


def _selection():
    """A fixed selection of the cross product: the four epilogues at C = 33 first (their other axes drawn), then two passes over
    every axis in which pass p pairs value i of an axis with the values (i * step_p + p) of the others — every value of every
    axis appears at least twice. Drawn once with numpy's default_rng(20261016); the list is what counts."""
    rng = np.random.default_rng(20261016)
    cases = [(33, int(rng.choice(AX_ORDER)), int(rng.choice(AX_D)), e) for e in AX_EPI]
    for p, step in enumerate((3, 5)):
        for i in range(8):
            cases.append((AX_C[i], AX_ORDER[(i * step + p) % 8], AX_D[(i + 2 * p) % 6], AX_EPI[(i + p) % 4]))
    for ax, vals, k in ((AX_C, [c[0] for c in cases], 2), (AX_ORDER, [c[1] for c in cases], 2), (AX_D, [c[2] for c in cases], 2), (AX_EPI, [c[3] for c in cases], 2)):
        assert all(vals.count(v) >= k for v in ax), (ax, vals)
    return cases


def bank_tunes(C, order, seed):
    """Per channel a different Fc: both signs, zero (channel 1 where there is one), and channels 0 and C - 1 with equal Fc but
    different widths."""
    rng = np.random.default_rng(seed)
    tunes = []
    for c in range(C):
        Fc = float(rng.integers(-1100, 1100)) * 1e3 + 500.0
        width = float(rng.integers(8, 200)) * 1e3
        if c == 1:
            Fc = 0.0
        if c == C - 1 and C > 2:
            Fc, width = 210e3, 25e3
        if c == 0:
            Fc, width = 210e3, 90e3
        tunes.append(tune(Fc, Fc, width, order))
    return tunes


@pytest.mark.parametrize("C,order,D,epi", _selection())
def test_tuner_rows_vs_oracle(ctx, orc, C, order, D, epi, form):
    max_in = 6000
    lens = [0, 1, 3, 777, max_in, 300, 2, 1500]   # empty, one sample, shorter than most orders and decimations, ragged, max_in
    x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3), (210e3, 9000, 1.0)]).next_cs16(sum(lens))
    x = (x.astype(np.int32) + np.random.default_rng(C + order).integers(-3000, 3000, x.shape)).astype(np.int16)
    tunes = bank_tunes(C, order, seed=1000 * C + order)
    bank, lut = make_bank(ctx, tunes, D, EPIS[epi], max_in)
    refs = make_refs(orc, tunes, lut, D, EPIS[epi])
    for k, chunk in enumerate(split(x, lens)):
        y = bank.process(chunk)
        assert y.shape[0] == C
        for c in range(C):
            assert np.array_equal(y[c], refs[c].process(chunk)), (k, c, len(chunk))
        if len(chunk) == max_in:
            check_names(bank, form, D >= 4)


# ---- 3. tap extremes ------------------------------------------------------------------------------------------------------

def test_tuner_tap_extremes(ctx, orc, form):
    order, D, C = 40, 8, 6
    rng = np.random.default_rng(3)
    lut = sa.design_freqshift_lut_i16()
    taps = np.zeros((C, order, 2), np.int32)
    for c in range(C):   # rows on the byte-plane boundaries, each with its own arrangement
        taps[c] = np.asarray(BOUNDARY, np.int32)[rng.integers(0, len(BOUNDARY), (order, 2))]
    taps[2, :, 0] = 32639; taps[2, :, 1] = -32639          # the planes' limit on every tap: the int32 sums wrap
    incs, negs = [1365, 0, 4096, 77, 3000, 1], [0, 0, 1, 1, 0, 1]
    x = np.random.default_rng(4).integers(-32768, 32768, (9000, 2)).astype(np.int16)
    bank = sa.TunerBankI16(ctx, taps, lut, incs, negs, D, max_in=4096)
    refs = [Ref(orc, taps[c], lut, incs[c], negs[c], D, sa.EPI_NONE) for c in range(C)]
    for chunk in split(x, [4096, 4096, 808]):
        y = bank.process(chunk)
        for c in range(C):
            assert np.array_equal(y[c], refs[c].process(chunk)), c
    check_names(bank, form, True)
    # one row whose high byte plane does not fit int8: the whole bank falls back to the plain kernel, says so, stays exact
    big = taps[4].copy(); big[5, 0] = 32700
    bank.set_taps(4, big); refs[4].bb.set_taps(big)
    y = bank.process(x[:4096])
    assert bank.kernel_names == [VALU]
    for c in range(C):
        assert np.array_equal(y[c], refs[c].process(x[:4096])), c
    # ... created that way too
    taps2 = taps.copy(); taps2[4] = big
    bank2 = sa.TunerBankI16(ctx, taps2, lut, incs, negs, D, max_in=4096)
    assert bank2.kernel_names == [VALU]
    refs2 = [Ref(orc, taps2[c], lut, incs[c], negs[c], D, sa.EPI_NONE) for c in range(C)]
    y = bank2.process(x[:4096])
    for c in range(C):
        assert np.array_equal(y[c], refs2[c].process(x[:4096])), c
    # replaced by taps that fit: the matrix form again
    bank.set_taps(4, taps[4]); refs[4].bb.set_taps(taps[4])
    y = bank.process(x[4096:8192])
    for c in range(C):
        assert np.array_equal(y[c], refs[c].process(x[4096:8192])), c
    check_names(bank, form, True)


# ---- 4. retune one channel mid-stream -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", ["none", "fm"])
def test_tuner_retune_one_channel(ctx, orc, epi, form):
    C, order, D = 35, 127, 8
    tunes = bank_tunes(C, order, seed=5)
    x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3)]).next_cs16(14000)
    bank, lut = make_bank(ctx, tunes, D, EPIS[epi], 4096)
    still, _ = make_bank(ctx, tunes, D, EPIS[epi], 4096)      # the same bank, never retuned
    refs = make_refs(orc, tunes, lut, D, EPIS[epi])
    chunks = split(x, [4096, 3000, 2000, 777, 4096])
    for k, chunk in enumerate(chunks):
        if k == 1:
            t = tune(-150e3, -150e3, 50e3, order)
            bank.set_shift(17, t[1], t[2]); refs[17].bb.set_shift(t[1], t[2])
        if k == 2:
            t = tune(0.0, -150e3, 30e3, order)
            bank.set_taps(17, t[0]); refs[17].bb.set_taps(t[0])
            bank.set_shift(0, 0, False); refs[0].bb.set_shift(0, False)   # channel 0 stops rotating
        if k == 3:
            t = tune(333e3, 333e3, 30e3, order)
            bank.set_shift(34, t[1], t[2]); refs[34].bb.set_shift(t[1], t[2])
            bank.set_taps(34, t[0]); refs[34].bb.set_taps(t[0])
        y, ys = bank.process(chunk), still.process(chunk)
        for c in range(C):
            assert np.array_equal(y[c], refs[c].process(chunk)), (k, c)
            if c not in (0, 17, 34):
                assert np.array_equal(y[c], ys[c]), (k, c)
    assert not np.array_equal(y[17], ys[17])


def test_tuner_setters_refuse_a_channel_outside_the_bank(ctx, orc, form):
    """The smallest bank that has two rows to tell apart: 2 channels, max_in 64, one call each. Channels -1 and 2 are refused
    by set_taps and set_shift with the range in the message and nothing changed; a retune of channel 1 that succeeds leaves
    channel 0 as it is in a bank never retuned."""
    C, order, D, n = 2, 21, 8, 64
    tunes = bank_tunes(C, order, seed=9)
    x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3)]).next_cs16(2 * n)
    bank, lut = make_bank(ctx, tunes, D, sa.EPI_NONE, n)
    still, _ = make_bank(ctx, tunes, D, sa.EPI_NONE, n)
    refs = make_refs(orc, tunes, lut, D, sa.EPI_NONE)
    for c in (-1, C):
        for call in (lambda: bank.set_taps(c, tunes[0][0]), lambda: bank.set_shift(c, 1, False)):
            with pytest.raises(sa.SdrHipError) as e:
                call()
            assert e.value.code == sa.abi.E_INVALID and "outside [0,2)" in str(e.value), (c, str(e.value))
    for k, chunk in enumerate(split(x, [n, n])):
        if k == 1:
            t = tune(-150e3, -150e3, 50e3, order)
            bank.set_shift(1, t[1], t[2]); refs[1].bb.set_shift(t[1], t[2])
            bank.set_taps(1, t[0]); refs[1].bb.set_taps(t[0])
        y, ys = bank.process(chunk), still.process(chunk)
        for c in range(C):
            assert np.array_equal(y[c], refs[c].process(chunk)), (k, c)
        assert np.array_equal(y[0], ys[0]) and (k == 0) == np.array_equal(y[1], ys[1]), k


class _RowRetune:
    """One row of a bank driven by test_oracle_golden.replay_retune; the other rows keep their tunes."""

    def __init__(self, ctx, Ff, width, Fc, epi, row, C=4, order=127, D=8):
        self.order, self.row = order, row
        tunes = other_tunes(C - 1, order, seed=12)
        tunes.insert(row, tune(Fc, Ff, width, order))
        self.bank, _ = make_bank(ctx, tunes, D, epi, 4096)

    def process(self, x):
        return self.bank.process(x)[self.row]

    def set_shift_hz(self, Fc):
        self.bank.set_shift(self.row, sa.design_freqshift_inc(Fc, FS), Fc < 0)

    def set_filter(self, Ff, width):
        self.bank.set_taps(self.row, sa.design_iqbb_taps(Ff, width, FS, self.order))

    def reconfigure(self):
        self.bank.reset(keep_history=True, keep_fm=True)   # (acts on every row: the fixture row is the one compared)


@pytest.mark.parametrize("row", [0, 3])
@pytest.mark.parametrize("which,epi", [("g12_retune_out", sa.EPI_NONE), ("g12_retune_fm", sa.EPI_FM)])
def test_tuner_retune_midstream_golden(ctx, golden, which, epi, row, form):
    from test_oracle_golden import replay_retune
    m = golden.meta(which)
    outs = replay_retune(m, golden.load("g1_iq_cs16"), lambda Ff, w, Fc: _RowRetune(ctx, Ff, w, Fc, epi, row))
    assert [len(o) for o in outs] == m["out_lens"]
    assert np.array_equal(np.concatenate(outs), golden.load(which))


# ---- 5. reset ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,D,first", [(127, 8, 4096), (21, 20, 1003), (16, 3, 999)])
def test_tuner_reset_semantics(ctx, orc, order, D, first, form):
    C = 18
    tunes = bank_tunes(C, order, seed=6)
    x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3)]).next_cs16(first + 4096)
    a, b = x[:first], x[first:]
    bank, lut = make_bank(ctx, tunes, D, sa.EPI_FM, 4096)
    y0 = bank.process(a)
    bank.reset(keep_history=False)                       # a freshly constructed bank
    assert np.array_equal(bank.process(a), y0)
    # keep_history = 1: _reconfigure keeps the ring where it lies, the FMDemod behind the node is reset
    refs = make_refs(orc, tunes, lut, D, sa.EPI_FM)
    for r in refs:
        r.process(a); r.bb.reset(); r.fm = orc.FMDemodI16()
    bank.reset(keep_history=True)
    y = bank.process(b)
    for c in range(C):
        assert np.array_equal(y[c], refs[c].process(b)), c
    # | 2: the demodulators' last angles survive as well
    for r in refs:
        r.bb.reset()
    bank.reset(keep_history=True, keep_fm=True)
    y = bank.process(a)
    for c in range(C):
        assert np.array_equal(y[c], refs[c].process(a)), c


# ---- 6. memory discipline: the host-pointer entry point with its own staging, and a strided device call ---------------------

@pytest.mark.hostptr_only
def test_tuner_host_pointer_path_and_strides(ctx, orc, form):
    C, order, D = 19, 64, 8
    tunes = bank_tunes(C, order, seed=7)
    x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3)]).next_cs16(9000)
    bank, lut = make_bank(ctx, tunes, D, sa.EPI_AM, 5000)
    refs = make_refs(orc, tunes, lut, D, sa.EPI_AM)
    want = [np.stack([r.process(c) for r in refs]) for c in split(x, [5000, 4000])]
    assert np.array_equal(bank.process(x[:5000]), want[0])
    # the device entry point on rows twice as far apart as they are long, canaries between them
    n, no = 4000, bank.out_count(4000)
    stride = 2 * no + 3
    hout = np.full((C, stride), 0x5A5A, np.int16)
    din, dout = ctx.malloc(n * 4), ctx.malloc(hout.nbytes)
    try:
        ctx.h2d(din, np.ascontiguousarray(x[5000:])); ctx.h2d(dout, hout)
        assert bank.process_dev(din, n, dout, stride) == no
        ctx.synchronize(); ctx.d2h(hout, dout)
    finally:
        ctx.free(din); ctx.free(dout)
    assert np.array_equal(hout[:, :no], want[1])
    assert np.all(hout[:, no:] == 0x5A5A)
    # invalid arguments: the existing codes
    for bad in (lambda: bank.process_dev(0, 5001, 0, 0), lambda: bank.set_shift(C, 1, 0), lambda: bank.set_taps(-1, tunes[0][0])):
        with pytest.raises(sa.SdrHipError) as e:
            bad()
        assert e.value.code in (sa.abi.E_SIZE, sa.abi.E_INVALID)
    with pytest.raises(sa.SdrHipError) as e:
        make_bank(ctx, tunes, 513, sa.EPI_NONE, 4096)
    assert e.value.code == sa.abi.E_UNSUPPORTED


# ---- 7. full size once ------------------------------------------------------------------------------------------------------

def test_tuner_full_size(ctx, orc, form):
    C, order, D, N = 1024, 127, 8, 65536
    tunes = bank_tunes(C, order, seed=8)
    x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3), (700e3, 5000, 2.0)]).next_cs16(N)
    x = (x.astype(np.int32) + np.random.default_rng(9).integers(-2000, 2000, x.shape)).astype(np.int16)
    bank, lut = make_bank(ctx, tunes, D, sa.EPI_FM, N)
    y = bank.process(x)
    check_names(bank, form, True)
    assert y.shape == (C, (N - 1) // D)   # the first window closes after D + 1 samples
    rows = sorted(set([0, 1, 15, 16, 17, 31, 32, 127, 128, 511, 512, 1007, 1008, 1022, 1023])
                  | set(int(r) for r in np.random.default_rng(10).choice(C, 17, replace=False)))[:32]
    for c in rows:
        assert np.array_equal(y[c], Ref(orc, tunes[c][0], lut, tunes[c][1], tunes[c][2], D, sa.EPI_FM).process(x)), c
    # rows differ pairwise where their tunes do (every channel has its own Fc or width)
    keys = {}
    for c in range(C):
        keys.setdefault(y[c, 1:].tobytes(), []).append(c)
    dup = [v for v in keys.values() if len(v) > 1]
    for v in dup:
        t0 = tunes[v[0]]
        assert all(np.array_equal(tunes[c][0], t0[0]) and tunes[c][1:] == t0[1:] for c in v), v
