"""GPU parity of the tuner bank with a demodulator per channel (sdrhip_tunermodes_i16_create / _set_mode / _get_modes,
TunerBankI16(modes=...)): FM, AM and USB channels over ONE input row in one launch. Every comparison is bit for bit. The
reference of every row is the CPU oracle's IQBaseBand<int16_t> followed by the demodulator of that row's mode (the oracle is
pinned to the compiled reference by tests/test_oracle_golden.py and the golden rows of tests/test_gpu_parity_tuner.py). Both
kernel forms run (SDRHIP_TUNER_PATH), the matrix form also with SDRHIP_TUNER_CTW = 1 and 8, inside the red-zoned device arena.
Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import libsdr_amd as sa

try:   # torch brings its own HIP runtime: it only finds the GPU when it initialises before libsdrhip.so does
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()
except Exception:   # pragma: no cover
    torch = None

import tuner_classes as tc
from test_gpu_parity_tuner import FS, HOT, VALU, Ref, bank_tunes, make_bank, split

pytestmark = pytest.mark.gpu

FM, AM, USB = sa.EPI_FM, sa.EPI_AM, sa.EPI_USB
MODES = [FM, AM, USB]
LENS = [4096, 1, 511, 513, 7, 3000]   # matrix | plain kernel at 512 samples; calls of 0 and 1 outputs; the open window


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


FORMS = ["auto", "valu", "ctw1", "ctw8"]


@pytest.fixture
def form(request, monkeypatch):
    """auto: the matrix kernel where the plan has one; valu: the plain kernel only; ctwN: auto with N channel tiles per
    workgroup. A test names its forms with @pytest.mark.parametrize("form", [...], indirect=True)."""
    monkeypatch.delenv("SDRHIP_TUNER_PATH", raising=False)
    monkeypatch.delenv("SDRHIP_TUNER_CTW", raising=False)
    if request.param == "valu":
        monkeypatch.setenv("SDRHIP_TUNER_PATH", "valu")
    if request.param.startswith("ctw"):
        monkeypatch.setenv("SDRHIP_TUNER_CTW", request.param[3:])
    return request.param


all_forms = pytest.mark.parametrize("form", FORMS, indirect=True)
both_forms = pytest.mark.parametrize("form", FORMS[:2], indirect=True)


def tile_modes(C):
    """Every tile of 16 channels holds all three modes, and the tile edges (rows 15 | 16, 31 | 32) change mode."""
    return [MODES[(c + c // 16) % 3] for c in range(C)]


def make_modes_bank(ctx, tunes, D, modes, max_in, cu8=False):
    lut = sa.design_freqshift_lut_i16()
    taps = np.stack([np.asarray(t[0], np.int32).reshape(-1, 2) for t in tunes])
    bank = sa.TunerBankI16(ctx, taps, lut, [t[1] for t in tunes], [t[2] for t in tunes], D, max_in=max_in, modes=modes)
    if cu8:
        bank.set_input_format(sa.abi.IN_CU8)
    return bank, lut


_streams = {}


def stream(orc, n, cu8, seed):
    """(what the bank is fed, the same as cs16 for the oracle): tones plus noise; computed once per (n, cu8, seed), read only."""
    key = (n, cu8, seed)
    if key not in _streams:
        x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3), (210e3, 9000, 1.0), (700e3, 5000, 2.0)]).next_cs16(n)
        x = (x.astype(np.int32) + np.random.default_rng(seed).integers(-3000, 3000, x.shape)).astype(np.int16)
        if cu8:
            x = ((x >> 8) + 128).astype(np.uint8)
        xo = orc.autocast_cu8_cs16(x) if cu8 else x
        x.setflags(write=False); xo.setflags(write=False)
        _streams[key] = (x, xo)
    return _streams[key]


def expect_names(bank, form, hot_possible):
    assert bank.kernel_names == ([HOT] if form != "valu" and hot_possible else [VALU]), (bank.kernel_names, form)


# ---- 1. rows against the oracle ---------------------------------------------------------------------------------------------

# (order, decimation, cu8)
PLANS = [(127, 8, False), (21, 125, True), (300, 20, False), (16, 3, False), (40, 4, False)]
# (decimations below 4 have no matrix form: SDRHIP_TUNER_CTW has nothing to act on)
PLAN_FORMS = [p + (f,) for p in PLANS for f in FORMS if p[1] >= tc.HOT_MIN_D or not f.startswith("ctw")]


@pytest.mark.parametrize("order,D,cu8,form", PLAN_FORMS, indirect=["form"],
                         ids=["o%d_d%d_%s-%s" % (o, d, "cu8" if u else "cs16", f) for o, d, u, f in PLAN_FORMS])
def test_mixed_rows_vs_oracle(ctx, orc, order, D, cu8, form):
    C = 48
    modes = tile_modes(C)
    assert all(set(modes[16 * t:16 * t + 16]) == set(MODES) for t in range(3)) and modes[15] != modes[16] and modes[31] != modes[32]
    tunes = bank_tunes(C, order, seed=100 * order + D)
    x, xo = stream(orc, sum(LENS), cu8, seed=order)
    bank, lut = make_modes_bank(ctx, tunes, D, modes, max(LENS), cu8)
    assert bank.modes() == modes
    refs = [Ref(orc, t[0], lut, t[1], t[2], D, m) for t, m in zip(tunes, modes)]
    n0 = 0
    for k, (chunk, chunk_o) in enumerate(zip(split(x, LENS), split(xo, LENS))):
        y = bank.process(chunk)
        assert y.dtype == np.int16 and y.shape == (C, tc.call_groups(n0, len(chunk), D)[1]), (k, y.shape)
        n0 += len(chunk)
        for c in range(C):
            assert np.array_equal(y[c], refs[c].process(chunk_o)), (k, c, modes[c], len(chunk))
        if y.shape[1]:
            expect_names(bank, form, D >= tc.HOT_MIN_D and len(chunk) >= tc.HOT_MIN_IN)


def _one_call_case(ctx, orc, C, modes, form):
    order, D, N = 127, 8, 8192
    tunes = bank_tunes(C, order, seed=31 * C)
    x, _ = stream(orc, N, False, seed=C)
    bank, lut = make_modes_bank(ctx, tunes, D, modes, N)
    force = int(form[3:]) if form.startswith("ctw") else None
    m = tc.model(C, order, D, True, 0, N, hot_plan=form != "valu", force_ctw=force)
    assert bank.plan_info(N) == m
    y = bank.process(x)
    expect_names(bank, form, True)
    if C <= tc.ORACLE_ALL_ROWS_UP_TO:
        rows = list(range(C))
    else:
        edge_model = m if m["hot"] else tc.model(C, order, D, True, 0, N)
        rows = sorted(tc.edge_rows(C, edge_model) | set(int(r) for r in np.random.default_rng(20261018).choice(C, 16, replace=False)))
    for c in rows:
        assert np.array_equal(y[c], Ref(orc, tunes[c][0], lut, tunes[c][1], tunes[c][2], D, modes[c]).process(x)), (c, modes[c])
    return y


@all_forms
@pytest.mark.parametrize("mode", MODES, ids=["fm", "am", "usb"])
def test_one_channel_of_each_mode(ctx, orc, mode, form):
    _one_call_case(ctx, orc, 1, [mode], form)


@all_forms
@pytest.mark.parametrize("C", [17, 257])
def test_random_modes_per_row(ctx, orc, C, form):
    modes = [MODES[int(i)] for i in np.random.default_rng(1000 + C).integers(0, 3, C)]
    assert set(modes) == set(MODES)
    _one_call_case(ctx, orc, C, modes, form)


# ---- 2. a mixed bank equals the single-mode banks ---------------------------------------------------------------------------------

@pytest.mark.parametrize("order,D,cu8", [(127, 8, False), (21, 125, True)], ids=["o127_d8_cs16", "o21_d125_cu8"])
@both_forms
def test_mixed_bank_equals_single_mode_banks(ctx, orc, order, D, cu8, form):
    C = 48
    modes = tile_modes(C)
    tunes = bank_tunes(C, order, seed=100 * order + D)
    x, _ = stream(orc, sum(LENS), cu8, seed=order)
    mixed, _ = make_modes_bank(ctx, tunes, D, modes, max(LENS), cu8)
    all_fm, _ = make_modes_bank(ctx, tunes, D, [FM] * C, max(LENS), cu8)
    single = {m: make_bank(ctx, tunes, D, m, max(LENS), cu8=cu8)[0] for m in MODES}
    for k, chunk in enumerate(split(x, LENS)):
        y, yf = mixed.process(chunk), all_fm.process(chunk)
        ys = {m: single[m].process(chunk) for m in MODES}
        assert mixed.kernel_names == single[FM].kernel_names
        for c in range(C):
            assert np.array_equal(y[c], ys[modes[c]][c]), (k, c, modes[c])
        assert np.array_equal(yf, ys[FM]), k


# ---- 3. set_mode mid-stream ---------------------------------------------------------------------------------------------------------

class StandAlone:
    """The oracle's baseband of one channel WITHOUT a demodulator, and stand-alone demodulator nodes behind it."""

    def __init__(self, orc, t, lut, D, mode):
        self.orc = orc
        self.bb = orc.IQBaseBandI16(t[0], lut, t[1], t[2], D)
        self.set_mode(mode)

    def set_mode(self, mode):
        self.mode = mode
        self.fm = self.orc.FMDemodI16()   # a fresh node at every switch

    def process(self, x):
        y = self.bb.process(x)
        if self.mode == FM:
            return self.fm.process(y)
        return self.orc.am_i16(y) if self.mode == AM else self.orc.usb_i16(y)


@both_forms
def test_set_mode_midstream(ctx, orc, form):
    C, order, D, n = 20, 127, 8, 2048
    seq = [AM, FM, FM, USB, FM, FM]   # channels 3 and 16 (the second tile's first row): AM -> FM -> USB -> FM between calls
    modes = tile_modes(C)
    modes[3] = modes[16] = seq[0]
    modes[7] = FM
    tunes = bank_tunes(C, order, seed=41)
    x, _ = stream(orc, n * len(seq), False, seed=42)
    bank, lut = make_modes_bank(ctx, tunes, D, modes, n)
    refs = [StandAlone(orc, t, lut, D, m) for t, m in zip(tunes, modes)]
    for k, chunk in enumerate(split(x, [n] * len(seq))):
        if k and seq[k] != seq[k - 1]:
            for c in (3, 16):
                bank.set_mode(c, seq[k]); refs[c].set_mode(seq[k]); modes[c] = seq[k]
            assert bank.modes() == modes
        y = bank.process(chunk)
        for c in range(C):
            assert np.array_equal(y[c], refs[c].process(chunk)), (k, c, modes[c])
    expect_names(bank, form, True)
    # a switch to the mode a channel has is a new node too: FM's last angle starts from 0 again
    bank.set_mode(7, FM); refs[7].set_mode(FM)
    y = bank.process(x[:n])
    for c in range(C):
        assert np.array_equal(y[c], refs[c].process(x[:n])), c


@both_forms
def test_reset_after_set_mode_keeps_or_clears_fm_angle(ctx, orc, form):
    C, order, D, n = 20, 127, 8, 2048
    modes = tile_modes(C)
    modes[7] = FM
    tunes = bank_tunes(C, order, seed=41)
    x, _ = stream(orc, 3 * n, False, seed=43)
    a, b, c3 = x[:n], x[n:2 * n], x[2 * n:]
    bank, lut = make_modes_bank(ctx, tunes, D, modes, n)
    refs = [StandAlone(orc, t, lut, D, m) for t, m in zip(tunes, modes)]

    def step(chunk):
        y = bank.process(chunk)
        for c in range(C):
            assert np.array_equal(y[c], refs[c].process(chunk)), (c, modes[c])
        return y

    step(a)
    bank.set_mode(3, FM); refs[3].set_mode(FM); modes[3] = FM
    bank.set_mode(16, USB); refs[16].set_mode(USB); modes[16] = USB
    step(b)
    # | 2: the FM channels' angles survive the reset (the node behind a reconfigured baseband is not reset)
    bank.reset(keep_history=True, keep_fm=True)
    for r in refs:
        r.bb.reset()
    y_kept = step(c3)
    assert bank.modes() == modes
    # without it every FMDemod is a fresh one; channel 7's first difference then starts from angle 0
    bank.reset(keep_history=True)
    for r in refs:
        r.bb.reset(); r.fm = orc.FMDemodI16()
    step(a)
    fresh = StandAlone(orc, tunes[7], lut, D, FM)
    fresh.process(a); fresh.process(b); fresh.bb.reset(); fresh.fm = orc.FMDemodI16()
    y_cleared = fresh.process(c3)
    assert y_kept[7][1] != y_cleared[1] and np.array_equal(y_kept[7][2:], y_cleared[2:])   # (the kept angle is what out[1] shows)


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------

def _raw_create_modes(ctx, taps, lut, incs, negs, modes, D, max_in):
    """sdrhip_tunermodes_i16_create with modes passed as it is (None: NULL); (code, handle)."""
    taps = np.ascontiguousarray(taps, np.int32); lut = np.ascontiguousarray(lut, np.int32)
    inc = np.ascontiguousarray(incs, np.uint32); neg = np.ascontiguousarray(negs, np.intc)
    m = None if modes is None else np.ascontiguousarray(modes, np.intc).ctypes.data_as(C.POINTER(C.c_int))
    h = C.c_void_p(0x1)
    code = sa.abi.lib().sdrhip_tunermodes_i16_create(ctx.handle, taps.ctypes.data_as(C.POINTER(C.c_int32)), taps.shape[1],
                                                      lut.ctypes.data_as(C.POINTER(C.c_int32)), inc.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      neg.ctypes.data_as(C.POINTER(C.c_int)), m, D, taps.shape[0], max_in, C.byref(h))
    return code, h.value


@both_forms
def test_mode_errors(ctx, orc, form):
    Cn, order, D, n = 20, 127, 8, 2048
    modes = tile_modes(Cn)
    tunes = bank_tunes(Cn, order, seed=51)
    lut = sa.design_freqshift_lut_i16()
    taps = np.stack([np.asarray(t[0], np.int32).reshape(-1, 2) for t in tunes])
    incs, negs = [t[1] for t in tunes], [t[2] for t in tunes]
    for bad in ([sa.EPI_NONE] + modes[1:], None, modes[:5] + [7] + modes[6:], modes[:-1] + [-1]):
        code, h = _raw_create_modes(ctx, taps, lut, incs, negs, bad, D, n)
        assert code == sa.abi.E_INVALID and h is None, (bad, code, h)
    x, _ = stream(orc, 2 * n, False, seed=52)
    bank, _ = make_modes_bank(ctx, tunes, D, modes, n)
    refs = [Ref(orc, t[0], lut, t[1], t[2], D, m) for t, m in zip(tunes, modes)]
    y = bank.process(x[:n])
    for c in range(Cn):
        assert np.array_equal(y[c], refs[c].process(x[:n])), c
    for c, m in ((-1, FM), (Cn, FM), (3, 7), (3, sa.EPI_NONE), (3, -1), (3, 4)):
        with pytest.raises(sa.SdrHipError) as e:
            bank.set_mode(c, m)
        assert e.value.code == sa.abi.E_INVALID, (c, m)
        assert ("outside [0,%d)" % Cn in str(e.value)) == (c in (-1, Cn)), (c, m, str(e.value))
    few = (C.c_int * (Cn - 1))()
    assert sa.abi.lib().sdrhip_tunermodes_i16_get_modes(bank._h, few, Cn - 1) == sa.abi.E_INVALID
    assert bank.modes() == modes
    y = bank.process(x[n:])       # nothing changed: the FM rows' angles included
    for c in range(Cn):
        assert np.array_equal(y[c], refs[c].process(x[n:])), c
    # a bank with one demodulator for all channels
    single, _ = make_bank(ctx, tunes, D, FM, n)
    for call in (lambda: single.set_mode(0, AM), lambda: single.set_mode(0, FM), single.modes):
        with pytest.raises(sa.SdrHipError) as e:
            call()
        assert e.value.code == sa.abi.E_UNSUPPORTED


@all_forms
@pytest.mark.parametrize("order,D", [(127, 8), (21, 125), (16, 3)])
def test_plan_info_is_fm_geometry(ctx, order, D, form):
    Cn, max_in = 48, 65536
    tunes = bank_tunes(Cn, order, seed=61)
    bank, _ = make_modes_bank(ctx, tunes, D, [AM, USB] * (Cn // 2), max_in)   # (whatever the modes are)
    force = int(form[3:]) if form.startswith("ctw") else None
    for n_in in (511, 512, 65536):
        want = tc.model(Cn, order, D, True, 0, n_in, hot_plan=form != "valu", force_ctw=force)
        got = bank.plan_info(n_in)
        assert list(got) == list(tc.FIELDS) and got == want, (n_in, got, want)
