"""GPU parity of the real-input tuner bank (sdrhip_tunerbb_i16_create / sdrhip_tunermodes_bb_i16_create, TunerBankI16(real=True)):
C BaseBand<int16_t> channels (+ FMDemod / AMDemod / USBDemod in place) over ONE row of real int16 samples. Every comparison is
exact equality of whole rows against the CPU oracle's BaseBandI16 per channel followed by that row's demodulator (the oracle
is pinned to the compiled reference by tests/test_oracle_golden.py). Every test runs under both kernel forms (the matrix form
where the plan has one — asserted through plan_info before the call, so that a silent fallback cannot pass — and
SDRHIP_TUNER_PATH=valu) and inside the red-zoned device arena (tests/redzone.py); tests marked hostptr_only go through the
library's own staging instead. A case's oracle rows are computed once and shared by both forms.
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

pytestmark = pytest.mark.gpu

FS = 2.0e6   # a direct-sampling HF receiver
NONE, FM, AM, USB = sa.EPI_NONE, sa.EPI_FM, sa.EPI_AM, sa.EPI_USB
EPIS = {"none": NONE, "fm": FM, "am": AM, "usb": USB}
HOT, VALU = "tuner_bb_i16_mfma_kernel", "tuner_bb_i16_valu_kernel"
HOT_MIN_D, HOT_MIN_IN = 4, 512          # sdrhip.h: the matrix form's decimations and call lengths
PLANE_LIMIT = (1 << 15) - 128           # ... and taps: |component| below this on every channel


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
    monkeypatch.delenv("SDRHIP_TUNER_CTW", raising=False)
    if request.param == "valu":
        monkeypatch.setenv("SDRHIP_TUNER_PATH", "valu")
    return request.param


_streams, _refs = {}, {}


def stream(n, seed):
    """n real int16 samples: carriers all over the band plus noise. Computed once per (n, seed), read only."""
    if (n, seed) not in _streams:
        rng = np.random.default_rng(seed)
        t = np.arange(n, dtype=np.float64)
        x = sum(a * np.cos(2 * np.pi * f / FS * t + p) for f, a, p in
                ((7.1e3, 5000, 0.0), (101.5e3, 7000, 0.3), (455e3, 6000, 1.0), (803e3, 4000, 2.0), (14.07e3, 3000, 0.7)))
        x = np.clip(np.rint(x) + rng.integers(-3000, 3000, n), -32768, 32767).astype(np.int16)
        x.setflags(write=False)
        _streams[(n, seed)] = x
    return _streams[(n, seed)]


def cached(key, make):
    """The oracle's rows of a case: computed by the first form that asks, shared with the other, never changed."""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def fits(taps):
    return bool(np.all(np.abs(np.asarray(taps, np.int64)) < PLANE_LIMIT))


def tune(Fc, Ff, width, order):
    """(taps, lut_inc, negative): the reference's Q16 design; where the taps of a very short filter exceed two byte planes
    (one tap: 2^16), a quarter of them — a narrow channel of a wideband stream has small taps, and the bank takes any."""
    taps = sa.design_bb_taps(Ff, width, FS, order)
    if not fits(taps):
        taps = taps // 4
    assert fits(taps)
    return taps, sa.design_freqshift_inc(Fc, FS), Fc < 0


def bank_tunes(C, order, seed):
    """Per channel a different Fc: both signs, zero (channel 1 where there is one), channels 0 and C - 1 with equal Fc but
    different widths."""
    rng = np.random.default_rng(seed)
    tunes = []
    for c in range(C):
        Fc, width = float(rng.integers(-900, 900)) * 1e3 + 500.0, float(rng.integers(2, 60)) * 1e3
        if c == 1:
            Fc = 0.0
        if c == C - 1 and C > 2:
            Fc, width = 101e3, 6e3
        if c == 0:
            Fc, width = 101e3, 20e3
        tunes.append(tune(Fc, Fc, width, order))
    return tunes


class Ref:
    """The oracle's real-input node (+ demodulator) of one channel."""

    def __init__(self, orc, taps, lut, inc, neg, D, epi):
        self.orc, self.epi = orc, epi
        self.bb = orc.BaseBandI16(taps, lut, inc, neg, D)
        self.fm = orc.FMDemodI16()

    def set_mode(self, mode):   # a new demodulator node behind the baseband
        self.epi, self.fm = mode, self.orc.FMDemodI16()

    def process(self, x):
        y = self.bb.process(x)
        if self.epi == FM:
            return self.fm.process(y)
        if self.epi == AM:
            return self.orc.am_i16(y)
        if self.epi == USB:
            return self.orc.usb_i16(y)
        return y


def stack(tunes):
    return np.stack([np.asarray(t[0], np.int32).reshape(-1, 2) for t in tunes])


def make_bank(ctx, tunes, D, epi, max_in, modes=None):
    lut = sa.design_freqshift_lut_i16()
    bank = sa.TunerBankI16(ctx, stack(tunes), lut, [t[1] for t in tunes], [t[2] for t in tunes], D, max_in=max_in, epilogue=epi, modes=modes, real=True)
    return bank, lut


def make_refs(orc, tunes, lut, D, epis):
    epis = epis if isinstance(epis, (list, tuple)) else [epis] * len(tunes)
    return [Ref(orc, t[0], lut, t[1], t[2], D, e) for t, e in zip(tunes, epis)]


def run_call(bank, chunk, form, D, all_fit=True):
    """One call; where the matrix form is meant to run, plan_info says so BEFORE the call and kernel_names after it."""
    n = len(chunk)
    hot = form == "auto" and D >= HOT_MIN_D and n >= HOT_MIN_IN and all_fit
    if n:
        assert bank.plan_info(n)["hot"] == (1 if hot else 0), (n, D, form, bank.plan_info(n))
    y = bank.process(chunk)
    if n:
        assert bank.kernel_names == [HOT if hot else VALU], (bank.kernel_names, n, D, form)
    return y


def assert_rows(y, want, tag):
    assert y.shape[0] == len(want), (y.shape, tag)
    for c, w in enumerate(want):
        assert y[c].shape == w.shape and np.array_equal(y[c], w), (tag, c)


# ---- 1. rows against the oracle -----------------------------------------------------------------------------------------------

AX_C = [1, 15, 16, 17, 33]                                  # partial and multiple tiles of 16 channels
AX_ORDER = [1, 31, 32, 33, 64, 65, 127, 273, 513]           # S = ceil(order / 32) boundaries and the front pad
AX_D = [1, 3, 4, 5, 8, 20, 125, 512]
AX_EPI = ["none", "fm", "am", "usb"]


def _selection():
    """A fixed selection of the cross product: the four epilogues at C = 33 first (their other axes drawn), then six passes over
    the nine orders in which pass p pairs order (i * step_p + p) with channel count i, decimation (i + 3 p) and epilogue
    (i + p) — every value of every axis appears at least four times. Drawn once with numpy's default_rng(20261018); the list
    is what counts."""
    rng = np.random.default_rng(20261018)
    cases = [(33, int(rng.choice(AX_ORDER)), int(rng.choice(AX_D)), e) for e in AX_EPI]
    for p, step in enumerate((1, 2, 4, 5, 7, 8)):
        for i in range(9):
            cases.append((AX_C[(i + p) % 5], AX_ORDER[(i * step + p) % 9], AX_D[(i + 3 * p) % 8], AX_EPI[(i + p) % 4]))
    cases = list(dict.fromkeys(cases))
    for ax, vals in ((AX_C, [c[0] for c in cases]), (AX_ORDER, [c[1] for c in cases]), (AX_D, [c[2] for c in cases]), (AX_EPI, [c[3] for c in cases])):
        assert all(vals.count(v) >= 4 for v in ax), (ax, vals)
    assert 50 <= len(cases) <= 64
    return cases


def case_lens(D):
    """Empty, one sample, either side of the matrix form's shortest call, ragged, and 74 windows plus 5 samples: history, open
    windows, LUT phase and FM angles cross calls, and both forms run on the same bank."""
    return [0, 1, 511, 512, 513, 777, 2 * D * 37 + 5]


@pytest.mark.parametrize("C,order,D,epi", _selection())
def test_real_rows_vs_oracle(ctx, orc, C, order, D, epi, form):
    lens = case_lens(D)
    x = stream(sum(lens), seed=order + D)
    tunes = bank_tunes(C, order, seed=1000 * C + order)
    bank, lut = make_bank(ctx, tunes, D, EPIS[epi], max(lens))
    want = cached(("rows", C, order, D, epi), lambda: [[r.process(c) for c in split(x, lens)] for r in make_refs(orc, tunes, lut, D, EPIS[epi])])
    assert bank.plan_info(max(lens))["S"] == (order + 31) // 32
    for k, chunk in enumerate(split(x, lens)):
        y = run_call(bank, chunk, form, D)
        assert_rows(y, [w[k] for w in want], (k, len(chunk)))


# ---- 2. odd alignment -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", ["none", "fm"])
def test_real_odd_alignment(ctx, orc, epi, form):
    """Decimation 5 and a first buffer of 513 samples. A time tile holds 102 windows = 510 columns (FM: 101 new ones = 505), and a
    lane's K slice starts at plane byte tc + 16 h + 32 s with tc = 32 kb + n over all columns of the tile: the lanes n, n + 1,
    n + 2, n + 3 of every column block are the four `off & 3` classes 0, 1, 2, 3, in every tile of every call. What changes with
    the buffers is where a tile's staged window starts in the input row: the calls begin at absolute samples 0, 513, 1290,
    3338, so their first windows begin at call-relative samples 0, -3, 0, -3 and tile k's window at (0 | -3) + 510 k - (KW - 1)
    (505 k with FM), KW = 96: input offsets of all four residues mod 4, odd ones included, on a row that itself starts at an odd
    multiple of two bytes in the arena."""
    C, order, D = 17, 65, 5
    lens = [513, 777, 2048, 1531]
    x = stream(sum(lens), seed=5)
    tunes = bank_tunes(C, order, seed=55)
    bank, lut = make_bank(ctx, tunes, D, EPIS[epi], max(lens))
    want = cached(("odd", epi), lambda: [[r.process(c) for c in split(x, lens)] for r in make_refs(orc, tunes, lut, D, EPIS[epi])])
    info = bank.plan_info(2048)
    if form == "auto":
        assert info["hot"] == 1 and info["S"] == 3 and info["CG"] == 102 and info["OG"] == (101 if epi == "fm" else 102) and info["tiles"] >= 4, info
    for k, chunk in enumerate(split(x, lens)):
        assert_rows(run_call(bank, chunk, form, D), [w[k] for w in want], k)


# ---- 3. a demodulator per channel ------------------------------------------------------------------------------------------------

def test_real_per_channel_modes(ctx, orc, form):
    C, order, D = 17, 127, 8
    modes = [(FM, AM, USB)[c % 3] for c in range(C)]
    lens = [2048, 511, 1, 513, 1500]
    x = stream(sum(lens), seed=31)
    tunes = bank_tunes(C, order, seed=32)
    bank, lut = make_bank(ctx, tunes, D, NONE, max(lens), modes=modes)
    assert bank.modes() == modes
    single = {m: make_bank(ctx, tunes, D, m, max(lens))[0] for m in (FM, AM, USB)}
    refs = make_refs(orc, tunes, lut, D, modes)
    switched = set()
    for k, chunk in enumerate(split(x, lens)):
        if k == 2:    # channel 3: FM -> USB; 16 (the second tile's only row): AM -> FM; 6: FM -> FM, a fresh FMDemod
            for c, m in ((3, USB), (16, FM), (6, FM)):
                bank.set_mode(c, m); refs[c].set_mode(m); modes[c] = m; switched.add(c)
            assert bank.modes() == modes
        y = run_call(bank, chunk, form, D)
        assert y.dtype == np.int16 and y.ndim == 2
        assert_rows(y, [r.process(chunk) for r in refs], k)
        ys = {m: b.process(chunk) for m, b in single.items()}
        for c in range(C):
            if c not in switched:
                assert np.array_equal(y[c], ys[modes[c]][c]), (k, c)
    with pytest.raises(sa.SdrHipError) as e:
        bank.set_mode(0, NONE)
    assert e.value.code == sa.abi.E_INVALID
    with pytest.raises(sa.SdrHipError) as e:
        single[FM].set_mode(0, AM)
    assert e.value.code == sa.abi.E_UNSUPPORTED


# ---- 4. tap and sample extremes ----------------------------------------------------------------------------------------------------

def test_real_tap_and_sample_extremes(ctx, orc, form):
    order, D, C, n = 40, 8, 6, 2048
    rng = np.random.default_rng(3)
    lut = sa.design_freqshift_lut_i16()
    lim = PLANE_LIMIT - 1                                   # 2^15 - 129: the last value two byte planes hold
    taps = (rng.integers(0, 2, (C, order, 2)) * 2 - 1).astype(np.int32) * lim   # +-(2^15 - 129) on every channel, signs drawn
    taps[2, :, 0] = lim; taps[2, :, 1] = -lim              # one sign per component: the int32 sums wrap
    incs, negs = [1365, 0, 4096, 77, 3000, 1], [0, 0, 1, 1, 0, 1]
    x = np.concatenate([np.full(n // 2, -32768, np.int16), np.full(n // 2, 32767, np.int16),
                        np.random.default_rng(4).integers(-32768, 32768, 2 * n).astype(np.int16)])
    assert order * lim * 32768 > 2 ** 31
    bank = sa.TunerBankI16(ctx, taps, lut, incs, negs, D, max_in=n, real=True)
    refs = [Ref(orc, taps[c], lut, incs[c], negs[c], D, NONE) for c in range(C)]
    assert_rows(run_call(bank, x[:n], form, D), [r.process(x[:n]) for r in refs], "limit")
    # one channel at 2^15 - 128: the whole bank runs the plain form, says so, stays exact. (The oracle's real node has no
    # set_taps: a second node with the new taps is fed the same stream, and behind a retap at a window boundary — n is a
    # multiple of D — ring, LUT phase and decimator of the two are equal, so the row goes on as that node's.)
    big = taps[4].copy(); big[5, 0] = PLANE_LIMIT
    shadow = Ref(orc, big, lut, incs[4], negs[4], D, NONE)
    shadow.process(x[:n])
    assert n % D == 0
    bank.set_taps(4, big)
    y = run_call(bank, x[n:2 * n], form, D, all_fit=False)
    assert bank.kernel_names == [VALU]
    w = [r.process(x[n:2 * n]) for r in refs]
    w[4] = shadow.process(x[n:2 * n])
    assert_rows(y, w, "misfit")
    # ... created that way too
    taps2 = taps.copy(); taps2[4] = big
    bank2 = sa.TunerBankI16(ctx, taps2, lut, incs, negs, D, max_in=n, real=True)
    assert bank2.kernel_names == [VALU]
    assert_rows(run_call(bank2, x[:n], form, D, all_fit=False), [Ref(orc, taps2[c], lut, incs[c], negs[c], D, NONE).process(x[:n]) for c in range(C)], "created")
    # replaced by taps that fit: the matrix form again
    bank.set_taps(4, taps[4])
    assert_rows(run_call(bank, x[2 * n:3 * n], form, D), [r.process(x[2 * n:3 * n]) for r in refs], "fits again")
    # the widest taps the node takes, full-scale rows: the plain form's 24-bit multiplies, sums that wrap many times over
    wide = (rng.integers(0, 2, (C, order, 2)) * 2 - 1).astype(np.int32) * ((1 << 23) - 1)
    wide[1, :, 0] = (1 << 23) - 1; wide[1, :, 1] = -(1 << 23) + 1
    bank3 = sa.TunerBankI16(ctx, wide, lut, incs, negs, D, max_in=n, real=True)
    refs3 = [Ref(orc, wide[c], lut, incs[c], negs[c], D, NONE) for c in range(C)]
    for k in range(2):
        chunk = x[k * n:(k + 1) * n]
        assert_rows(run_call(bank3, chunk, form, D, all_fit=False), [r.process(chunk) for r in refs3], ("wide", k))


# ---- 5. retunes and resets -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", ["none", "fm"])
def test_real_retune_one_channel(ctx, orc, epi, form):
    """set_shift and set_taps on channels 17 and 34 mid-stream; the others equal a bank that is never retuned. The oracle's real
    node has no set_taps, so the retapped rows are compared with a second oracle node made with the new taps and fed the same
    stream: behind a retap at a window boundary (here 4096 + 3000 + 1000 samples, a multiple of 8, no open window) both have the
    same ring, LUT phase and decimator — from then on the row must equal it."""
    C, order, D = 35, 127, 8
    lens = [4096, 3000, 1000, 777, 2048]
    tunes = bank_tunes(C, order, seed=5)
    x = stream(sum(lens), seed=6)
    bank, lut = make_bank(ctx, tunes, D, EPIS[epi], max(lens))
    still, _ = make_bank(ctx, tunes, D, EPIS[epi], max(lens))
    refs = make_refs(orc, tunes, lut, D, EPIS[epi])
    t_shift, t_taps = tune(-150e3, -150e3, 10e3, order), tune(333e3, 333e3, 4e3, order)
    shadow = Ref(orc, t_taps[0], lut, tunes[34][1], tunes[34][2], D, EPIS[epi])   # channel 34 with the taps it will get
    for k, chunk in enumerate(split(x, lens)):
        if k == 1:
            bank.set_shift(17, t_shift[1], t_shift[2]); refs[17].bb.set_shift(t_shift[1], t_shift[2])
        if k == 3:
            assert sum(lens[:3]) % D == 0
            bank.set_taps(34, t_taps[0]); refs[34].bb = shadow.bb   # (the FMDemod behind it goes on: it saw the row so far)
            bank.set_shift(0, 0, False); refs[0].bb.set_shift(0, False)   # channel 0 stops rotating
        if k < 3:
            shadow.bb.process(chunk)
        y, ys = run_call(bank, chunk, form, D), still.process(chunk)
        assert_rows(y, [r.process(chunk) for r in refs], k)
        for c in range(C):
            if c not in (0, 17, 34):
                assert np.array_equal(y[c], ys[c]), (k, c)
    assert not np.array_equal(y[17], ys[17]) and not np.array_equal(y[34], ys[34])


@pytest.mark.parametrize("order,D,first", [(127, 8, 4096), (21, 20, 1003), (33, 3, 999)])
def test_real_reset_semantics(ctx, orc, order, D, first, form):
    C = 18
    tunes = bank_tunes(C, order, seed=6)
    x = stream(first + 4096, seed=7)
    a, b = x[:first], x[first:]
    bank, lut = make_bank(ctx, tunes, D, FM, 4096)
    y0 = run_call(bank, a, form, D)
    bank.reset(keep_history=False)                       # a freshly constructed bank
    assert np.array_equal(bank.process(a), y0)
    # keep_history = 1: the ring stays where it lies, counters and phases restart, the FMDemod behind the node is reset
    refs = make_refs(orc, tunes, lut, D, FM)
    for r in refs:
        r.process(a); r.bb.reset(); r.fm = orc.FMDemodI16()
    bank.reset(keep_history=True)
    assert_rows(run_call(bank, b, form, D), [r.process(b) for r in refs], "keep ring")
    # | 2: the demodulators' last angles survive as well
    for r in refs:
        r.bb.reset()
    bank.reset(keep_history=True, keep_fm=True)
    assert_rows(run_call(bank, a, form, D), [r.process(a) for r in refs], "keep ring and fm")
    # 2 alone: a zeroed ring, the angles kept
    for k, r in enumerate(refs):
        fm = r.fm
        refs[k] = Ref(orc, tunes[k][0], lut, tunes[k][1], tunes[k][2], D, FM); refs[k].fm = fm
    bank.reset(keep_history=False, keep_fm=True)
    assert_rows(run_call(bank, b, form, D), [r.process(b) for r in refs], "keep fm")


# ---- 6. the same job by the other route ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi,D", [("none", 8), ("fm", 20), ("usb", 3)])
def test_real_bank_equals_one_channel_plans(ctx, epi, D, form):
    """Rows of a 3-channel bank = three one-channel sdrhip_bb_i16_create plans fed the same buffers; a retap in an OPEN window
    (the call lengths are no multiples of D) included."""
    order, lens = 127, [777, 2048, 513, 1, 1500]
    tunes = bank_tunes(3, order, seed=8)
    x = stream(sum(lens), seed=9)
    bank, lut = make_bank(ctx, tunes, D, EPIS[epi], max(lens))
    ones = [sa.BaseBandI16(ctx, t[0], lut, t[1], t[2], D, max_in=max(lens), epilogue=EPIS[epi]) for t in tunes]
    t2 = tune(50e3, 50e3, 3e3, order)
    for k, chunk in enumerate(split(x, lens)):
        if k == 2:
            assert sum(lens[:2]) % D != 0
            bank.set_taps(1, t2[0]); ones[1].set_taps(t2[0])
            bank.set_shift(2, t2[1], t2[2]); ones[2].set_shift(t2[1], t2[2])
        y = run_call(bank, chunk, form, D)
        for c in range(3):
            assert np.array_equal(y[c], ones[c].process(chunk)[0]), (k, c)


# ---- 7. memory discipline: the host-pointer entry point with its own staging, strides, the input format ----------------------------

@pytest.mark.hostptr_only
def test_real_host_pointer_path_and_strides(ctx, orc, form):
    import ctypes as C_
    C, order, D = 19, 64, 8
    tunes = bank_tunes(C, order, seed=7)
    x = stream(9000, seed=10)
    bank, lut = make_bank(ctx, tunes, D, AM, 5000)
    refs = make_refs(orc, tunes, lut, D, AM)
    want = [np.stack([r.process(c) for r in refs]) for c in split(x, [5000, 2000, 2000])]
    assert np.array_equal(run_call(bank, x[:5000], form, D), want[0])          # process(): tight rows
    # the host-pointer entry point on rows that are not tight, canaries between them
    n, no = 2000, bank.out_count(2000)
    stride = no + 5
    hout = np.full((C, stride), 0x5A5A, np.int16)
    got = C_.c_size_t(0)
    xin = np.ascontiguousarray(x[5000:7000])
    call = lambda s: sa.abi.lib().sdrhip_tuner_i16_process(bank._h, xin.ctypes.data_as(C_.c_void_p), n, hout.ctypes.data_as(C_.c_void_p), s, C_.byref(got))
    assert call(no - 1) == sa.abi.E_SIZE                                         # an out_stride smaller than the output count
    assert np.all(hout == 0x5A5A)
    assert call(stride) == sa.abi.OK and got.value == no
    assert np.array_equal(hout[:, :no], want[1]) and np.all(hout[:, no:] == 0x5A5A)
    # the device entry point on rows twice as far apart as they are long
    stride = 2 * no + 3
    hout = np.full((C, stride), 0x5A5A, np.int16)
    din, dout = ctx.malloc(n * 2), ctx.malloc(hout.nbytes)
    try:
        ctx.h2d(din, np.ascontiguousarray(x[7000:])); ctx.h2d(dout, hout)
        with pytest.raises(sa.SdrHipError) as e:
            bank.process_dev(din, n, dout, no - 1)
        assert e.value.code == sa.abi.E_SIZE
        assert bank.process_dev(din, n, dout, stride) == no
        ctx.synchronize(); ctx.d2h(hout, dout)
    finally:
        ctx.free(din); ctx.free(dout)
    assert np.array_equal(hout[:, :no], want[2]) and np.all(hout[:, no:] == 0x5A5A)
    for bad in (lambda: bank.process_dev(0, 5001, 0, 0), lambda: bank.set_shift(C, 1, 0), lambda: bank.set_taps(-1, tunes[0][0])):
        with pytest.raises(sa.SdrHipError) as e:
            bad()
        assert e.value.code in (sa.abi.E_SIZE, sa.abi.E_INVALID)


def test_real_bank_takes_its_own_sample_type_only(ctx, form):
    tunes = bank_tunes(3, 21, seed=11)
    for modes in (None, [FM, AM, USB]):
        bank, _ = make_bank(ctx, tunes, 8, NONE, 4096, modes=modes)
        with pytest.raises(sa.SdrHipError) as e:
            bank.set_input_format(sa.abi.IN_CU8)
        assert e.value.code == sa.abi.E_UNSUPPORTED
        y = bank.process(stream(1024, seed=12))            # ... and goes on taking real int16
        assert y.shape[:2] == (3, 128)
    with pytest.raises(sa.SdrHipError) as e:
        make_bank(ctx, tunes, 513, NONE, 4096)
    assert e.value.code == sa.abi.E_UNSUPPORTED


# ---- 8. seeded fuzz ------------------------------------------------------------------------------------------------------------------

FUZZ_PLANS = 40


def _fuzz_plan(i):
    """Plan i of the fixed draw: (C, order, D, epilogue or None, modes or None, taps, incs, negs, call lengths)."""
    rng = np.random.default_rng([20261018, i])
    C = int(rng.choice([1, 2, 7, 16, 17, 24, 40]))
    order = int(rng.choice([int(rng.integers(1, 514)), int(rng.integers(1, 70))]))
    D = int(rng.choice([int(rng.integers(1, 513)), int(rng.integers(1, 24))]))
    per_channel = bool(rng.integers(0, 3) == 0)
    modes = [int(m) for m in rng.choice([FM, AM, USB], C)] if per_channel else None
    epi = None if per_channel else int(rng.choice([NONE, FM, AM, USB]))
    kind = int(rng.integers(0, 4))   # 0, 1: taps within two byte planes; 2: one channel beyond them; 3: up to 24 bits everywhere
    lim = PLANE_LIMIT - 1 if kind < 3 else (1 << 23) - 1
    taps = rng.integers(-lim, lim + 1, (C, order, 2)).astype(np.int32)
    if kind == 2:
        taps[int(rng.integers(0, C)), int(rng.integers(0, order)), int(rng.integers(0, 2))] = int(rng.choice([-1, 1])) * int(rng.integers(PLANE_LIMIT, 1 << 23))
    incs = [int(v) for v in rng.integers(0, 32768, C)]
    negs = [bool(v) for v in rng.integers(0, 2, C)]
    lens = [int(v) for v in rng.choice([0, 1, 2, 77, 300, 511, 512, 513, 700, 1024, 1500], 5)] + [int(rng.integers(512, 2049))]
    return C, order, D, epi, modes, taps, incs, negs, lens


def test_real_seeded_fuzz(ctx, orc, form):
    lut = sa.design_freqshift_lut_i16()
    hot_calls = plain_calls = 0
    for i in range(FUZZ_PLANS):
        C, order, D, epi, modes, taps, incs, negs, lens = _fuzz_plan(i)
        x = np.random.default_rng([7, i]).integers(-32768, 32768, sum(lens)).astype(np.int16)
        bank = sa.TunerBankI16(ctx, taps, lut, incs, negs, D, max_in=max(lens), epilogue=NONE if epi is None else epi, modes=modes, real=True)
        want = cached(("fuzz", i), lambda: [[r.process(c) for c in split(x, lens)]
                                            for r in (Ref(orc, taps[c], lut, incs[c], negs[c], D, modes[c] if modes else epi) for c in range(C))])
        for k, chunk in enumerate(split(x, lens)):
            y = run_call(bank, chunk, form, D, all_fit=fits(taps))
            assert_rows(y, [w[k] for w in want], (i, k, C, order, D, epi, modes))
            if len(chunk):
                if bank.kernel_names == [HOT]:
                    hot_calls += 1
                else:
                    plain_calls += 1
        bank.close()
    # the draw covers both forms (run_call checked each call's form against the plan's decimation, taps and the call's length)
    assert plain_calls >= 20, plain_calls
    assert (hot_calls >= 20) if form == "auto" else hot_calls == 0, (hot_calls, plain_calls)


# ---- 9. full size once -------------------------------------------------------------------------------------------------------------------

def test_real_full_size(ctx, orc, form):
    C, order, D, N = 64, 127, 20, 65536
    tunes = bank_tunes(C, order, seed=8)
    x = stream(N, seed=9)
    bank, lut = make_bank(ctx, tunes, D, FM, N)
    y = run_call(bank, x, form, D)
    assert y.shape == (C, N // D)   # windows of D samples from the first sample on
    rows = [0, 17, 47, 63]
    want = cached("full", lambda: [Ref(orc, tunes[c][0], lut, tunes[c][1], tunes[c][2], D, FM).process(x) for c in rows])
    for c, w in zip(rows, want):
        assert np.array_equal(y[c], w), c
