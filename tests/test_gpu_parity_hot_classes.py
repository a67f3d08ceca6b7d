"""Every launchable instance of the IQBaseBand hot kernel, bit-exact against the oracle (tests/hot_classes.py holds the
matrix; tests/test_hot_classes_complete.py checks it against the build). One case per (form, input kind, S, high-plane range
[, low-plane range]): taps built so that the plan picks exactly that range, one plan per rotation and epilogue the
instance list holds, ragged long and short calls, and one call whose input follows the taps' signs so that the int32 FIR
sum wraps. Every process() runs in the red-zoned arena (conftest.py: the module name). Run with `pytest -m gpu` on an
MI355X."""
import numpy as np
import pytest

import hot_classes as hc
import libsdr_amd as sa
from redzone import RedZone

try:   # torch brings its own HIP runtime: it only finds the GPU when it initialises before libsdrhip.so does
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()
except Exception:   # pragma: no cover
    torch = None

pytestmark = pytest.mark.gpu

FS = 2.4e6
FC_ROT = (100e3, -100e3)   # rotation on: both signs of the shift (the table read backwards)
DECIMS = {hc.D8: (8,), hc.ANYD: (62, 125), hc.SD: (3, 5, 7)}
D_PARTIAL = 300            # the any-D form's large-decimation variant (HOT_EPI_PARTIAL)


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cu8_bytes(orc):
    """The complex<uint8> bytes AutoCast maps to the most positive and the most negative int16."""
    b = np.arange(256, dtype=np.uint8)
    v = orc.autocast_cu8_cs16(np.stack([b, b], 1))[:, 0]
    return int(np.argmax(v)), int(np.argmin(v))


def channels(S):
    return 2 if S >= 33 else 3


def lut_for(kind):
    return sa.design_freqshift_lut_i8() if kind == hc.CS8 else sa.design_freqshift_lut_i16()


def make_node(ctx, kind, taps, Fc, D, C, max_in, epi):
    lut, inc = lut_for(kind), sa.design_freqshift_inc(Fc, FS)
    assert (inc == 0) == (Fc == 0)
    cls = {hc.REAL: sa.BaseBandI16, hc.CS8: sa.IQBaseBandI8}.get(kind, sa.IQBaseBandI16)
    node = cls(ctx, taps, lut, inc, Fc < 0, D, channels=C, max_in=max_in, epilogue=epi)
    if kind == hc.CU8:
        node.set_input_format(sa.abi.IN_CU8)
    return node


class Oracle:
    """The oracle's baseband of one rotation for every channel, the epilogues derived from it."""

    def __init__(self, orc, kind, taps, Fc, D, C):
        self.orc, self.kind = orc, kind
        lut, inc = lut_for(kind), sa.design_freqshift_inc(Fc, FS)
        cls = {hc.REAL: orc.BaseBandI16, hc.CS8: orc.IQBaseBandI8}.get(kind, orc.IQBaseBandI16)
        self.bb = [cls(taps, lut, inc, Fc < 0, D) for _ in range(C)]
        self.fm = [orc.FMDemodI8() if kind == hc.CS8 else orc.FMDemodI16() for _ in range(C)]

    def set_taps(self, taps):
        for bb in self.bb:
            bb.set_taps(taps)

    def run(self, x):
        """{epilogue: [per-channel output]} for one call."""
        orc, out = self.orc, {e: [] for e in (hc.EPI_NONE, hc.EPI_FM, hc.EPI_AM, hc.EPI_USB)}
        for c, bb in enumerate(self.bb):
            r = bb.process(orc.autocast_cu8_cs16(x[c]) if self.kind == hc.CU8 else x[c])
            out[hc.EPI_NONE].append(r)
            out[hc.EPI_FM].append(self.fm[c].process(r) if len(r) else np.zeros(0, np.int16))
            if self.kind != hc.CS8:
                out[hc.EPI_AM].append(orc.am_i16(r))
                out[hc.EPI_USB].append(orc.usb_i16(r))
        return out


def random_input(rng, kind, C, n):
    if kind == hc.REAL:
        return rng.integers(-32768, 32768, (C, n), dtype=np.int16)
    if kind == hc.CU8:
        return rng.integers(0, 256, (C, n, 2), dtype=np.uint8)
    if kind == hc.CS8:
        return rng.integers(-128, 128, (C, n, 2), dtype=np.int8)
    return rng.integers(-32768, 32768, (C, n, 2), dtype=np.int16)


def aligned_input(kind, taps, C, n, cu8_bytes):
    """Full-scale samples that follow the taps' signs: tap i meets sample n - order + 1 + i, so with a period of `order`
    every order-th output sums |K| * full scale over the whole window — far beyond int32 for int16 samples (the wrap the
    byte-plane products must reproduce; int8 samples stay below it). Channels start at different phases."""
    taps = np.asarray(taps, np.int64).reshape(-1, 2)
    order = taps.shape[0]
    pr, pi = taps[:, 0] >= 0, taps[:, 1] < 0   # Re(K x) = Kr xr - Ki xi: xr with Kr's sign, xi against Ki's
    if kind == hc.CU8:
        hi, lo = cu8_bytes
        pat, dt = np.stack([np.where(pr, hi, lo), np.where(pi, hi, lo)], 1), np.uint8
    elif kind == hc.CS8:
        pat, dt = np.stack([np.where(pr, 127, -128), np.where(pi, 127, -128)], 1), np.int8
    else:
        pat, dt = np.stack([np.where(pr, 32767, -32768), np.where(pi, 32767, -32768)], 1), np.int16
    idx = (np.arange(n)[None, :] + 7 * np.arange(C)[:, None]) % order
    x = pat[idx].astype(dt)
    return np.ascontiguousarray(x[..., 0]) if kind == hc.REAL else x


def call_lengths(rng):
    """A long call (>= 3 hot tiles of the /8 form, >= 16 hot slices of the others, not tile-aligned), one too short for
    any hot tile, another long one, and the sign-aligned one."""
    return [int(rng.integers(12100, 12900)) | 1, int(rng.integers(900, 1900)), int(rng.integers(12000, 12800)) + 3, 12291]


def check_plan(node, form, kind, S, R, L, taps):
    p = node.plan_info
    got = (p["S"], p["S0"], p["NH"], p["NW"], p["L0"], p["NL"], p["kind"])
    assert got == (S, R[0], R[1], R[2], L[0], L[1], kind), got
    ah, al = hc.masks(S, kind, taps)
    assert hc.pick(S, ah, al, p["path"] == 1) == (hc.RANGES[S].index(R), R, (p["L0"], p["NL"])), "the range model drifted from pick_hot_ranges"
    return p


def run_case(ctx, orc, cu8_bytes, form, kind, S, taps, plans, seed, expect=None):
    """plans: [(Fc, D, epi)]; every plan against the oracle of its rotation over the same calls. expect: (R, L) to assert."""
    rng = np.random.default_rng(seed)
    C = channels(S)
    lens = call_lengths(rng)
    nodes, oracles = [], {}
    for Fc, Dp, epi in plans:
        node = make_node(ctx, kind, taps, Fc, Dp, C, max(lens), epi)
        if expect is not None:
            check_plan(node, form, kind, S, expect[0], expect[1], taps)
        names = node.kernel_names
        assert names[0] == hc.KERNEL[hc.ANYD if Dp == D_PARTIAL else form], (Fc, Dp, epi, names)
        nodes.append((node, Fc, Dp, epi))
        oracles.setdefault((Fc, Dp), Oracle(orc, kind, taps, Fc, Dp, C))
    before = RedZone.calls
    for k, n in enumerate(lens):
        x = aligned_input(kind, taps, C, n, cu8_bytes) if k == 3 else random_input(rng, kind, C, n)
        want = {key: o.run(x) for key, o in oracles.items()}
        for node, Fc, Dp, epi in nodes:
            y = node.process(x)
            for c in range(C):
                r = want[(Fc, Dp)][epi][c]
                assert y[c].shape == r.shape and np.array_equal(y[c], r), (Fc, Dp, epi, "call", k, n, "channel", c)
    assert RedZone.active and RedZone.calls >= before + len(lens) * len(nodes)


def case_decim(form, cid):
    ds = DECIMS[form]
    return ds[hc.case_seed(cid) % len(ds)]


@pytest.mark.parametrize("case", hc.cases(), ids=lambda c: c[0])
def test_hot_instance_vs_oracle(ctx, orc, cu8_bytes, case):
    cid, form, kind, S, R, L, per_rot = case
    seed = hc.case_seed(cid)
    taps = hc.taps_for(S, kind, hc.largest_order(S, kind), range(R[0], R[0] + R[1]), range(L[0], L[0] + L[1]), seed=seed)
    D = case_decim(form, cid)
    plans = []
    for rot, epis in per_rot.items():
        for i, Fc in enumerate(FC_ROT if rot else (0.0,)):
            plans += [(Fc, D, e) for e in epis if e != hc.EPI_PARTIAL]
            if hc.EPI_PARTIAL in epis:   # (one large-decimation plan per rotation: its epilogue is the finishing step's)
                plans.append((Fc, D_PARTIAL, (hc.EPI_FM, hc.EPI_USB, hc.EPI_AM)[i + (0 if rot else 2)]))
    run_case(ctx, orc, cu8_bytes, form, kind, S, taps, plans, seed, expect=(R, L))


@pytest.mark.parametrize("cls", hc.classes(), ids=lambda c: "%s-%s-S%d" % (hc.FORMS[c[0]], hc.KINDS[c[1]], c[2]))
def test_hot_class_smallest_order_vs_oracle(ctx, orc, cu8_bytes, cls):
    """The class's smallest order: the longest zero front pad in the window."""
    form, kind, S = cls
    order = hc.smallest_order(S, kind)
    steps = hc.reachable(S, kind, order)
    cid = "small-%s-%s-S%d" % (hc.FORMS[form], hc.KINDS[kind], S)
    seed = hc.case_seed(cid)
    taps = hc.taps_for(S, kind, order, steps, steps, seed=seed, anchors=False)
    ah, al = hc.masks(S, kind, taps)
    _, R, L = hc.pick(S, ah, al, form == hc.D8 and kind != hc.REAL)
    assert (hc.KERNEL[form], S, R[0], R[1], True, hc.EPI_FM, kind) + tuple(L) in hc.MATRIX
    D = case_decim(form, cid)
    run_case(ctx, orc, cu8_bytes, form, kind, S, taps, [(FC_ROT[0], D, hc.EPI_FM)], seed, expect=(R, L))


def _walk_classes():
    out = []
    for form in (hc.D8, hc.ANYD, hc.SD):
        for kind in (hc.CS16, hc.CU8):   # (the oracle's set_taps: IQBaseBand<int16_t>)
            for S in hc.STEPS:
                cs = [c for c in hc.cases() if c[1:4] == (form, kind, S) and True in c[6]]
                if len(cs) > 1:
                    out.append(("%s-%s-S%d" % (hc.FORMS[form], hc.KINDS[kind], S), form, kind, S, cs))
    return out


@pytest.mark.parametrize("walk", _walk_classes(), ids=lambda w: w[0])
def test_retap_walks_every_range_midstream(ctx, orc, walk):
    """One stream, set_taps through every range of the class (narrow -> widest -> narrow; S = 17 crosses from 8- to 16-wave
    workgroups, S = 9 the /8 form's low-plane ranges), the oracle retapped at the same sample: bit-exact throughout."""
    wid, form, kind, S, cs = walk
    seq = cs + cs[-2::-1]
    order = hc.largest_order(S, kind)
    tapsets = [hc.taps_for(S, kind, order, range(c[4][0], c[4][0] + c[4][1]), range(c[5][0], c[5][0] + c[5][1]), seed=hc.case_seed(c[0]) + 1)
               for c in seq]
    D = {hc.D8: 8, hc.ANYD: 62, hc.SD: 5}[form]
    C, Fc = 2, FC_ROT[0]
    rng = np.random.default_rng(hc.case_seed("walk-" + wid))
    lens = [int(rng.integers(12000, 13000)) for _ in seq]
    node = make_node(ctx, kind, tapsets[0], Fc, D, C, max(lens), sa.EPI_FM)
    ref = Oracle(orc, kind, tapsets[0], Fc, D, C)
    for k, (c, taps, n) in enumerate(zip(seq, tapsets, lens)):
        if k:
            node.set_taps(taps)
            ref.set_taps(taps)
        check_plan(node, form, kind, S, c[4], c[5], taps)
        assert node.kernel_names[0] == hc.KERNEL[form]
        x = random_input(rng, kind, C, n)
        y, want = node.process(x), ref.run(x)[hc.EPI_FM]
        for ch in range(C):
            assert np.array_equal(y[ch], want[ch]), (c[0], "step", k, "channel", ch)


def _wide_taps(kind):
    S = 9
    taps = hc.taps_for(S, kind, hc.largest_order(S, kind), range(S), range(S), seed=77).copy()
    taps[40, 0] = 32640   # one past the plane limit: 32640 = 128 * 256 - 128, its high byte 128 does not fit int8
    return taps


@pytest.mark.parametrize("kind", [hc.CS16, hc.REAL], ids=["cs16", "real"])
def test_plane_limit_at_create_runs_valu(ctx, orc, cu8_bytes, kind):
    taps = _wide_taps(kind)
    C, Fc = 2, FC_ROT[0]
    node = make_node(ctx, kind, taps, Fc, 8, C, 13000, sa.EPI_NONE)
    assert node.path == 0 and node.kernel_names == ["iqbb_i16_kernel"]
    ref = Oracle(orc, kind, taps, Fc, 8, C)
    rng = np.random.default_rng(5)
    for k, n in enumerate((12345, 1000, 12291)):
        x = aligned_input(kind, taps, C, n, cu8_bytes) if k == 2 else random_input(rng, kind, C, n)
        y, want = node.process(x), ref.run(x)[hc.EPI_NONE]
        for c in range(C):
            assert np.array_equal(y[c], want[c]), (k, c)


@pytest.mark.parametrize("kind", [hc.CS16, hc.REAL], ids=["cs16", "real"])
def test_plane_limit_at_set_taps_is_refused(ctx, orc, kind):
    S = 9
    taps = hc.taps_for(S, kind, hc.largest_order(S, kind), range(S), range(S), seed=78)
    C, Fc = 2, FC_ROT[0]
    node = make_node(ctx, kind, taps, Fc, 8, C, 13000, sa.EPI_FM)
    assert node.path in (1, 4) and node.kernel_names == ["iqbb_hot_kernel"]
    info = node.plan_info
    ref = Oracle(orc, kind, taps, Fc, 8, C)
    rng = np.random.default_rng(6)
    for k, n in enumerate((12345, 1000, 12301)):
        if k == 1:
            with pytest.raises(sa.abi.SdrHipError) as e:
                node.set_taps(_wide_taps(kind))
            assert e.value.code == sa.abi.E_UNSUPPORTED and "byte planes" in str(e.value)
            assert node.plan_info == info
        x = random_input(rng, kind, C, n)
        y, want = node.process(x), ref.run(x)[hc.EPI_FM]
        for c in range(C):
            assert np.array_equal(y[c], want[c]), (k, c)
