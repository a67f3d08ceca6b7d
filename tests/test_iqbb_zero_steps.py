"""The /8 hot kernel's low-plane K-step range: K steps whose low-byte tap fragments are all zero are not issued (plan_info
slots 9 and 10). Every tap set below runs against the CPU oracle and bit for bit against the same plan with the full range
(SDRHIP_IQBB_TRIM=0). Run with `pytest -m gpu` on an MI355X."""
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

FS = 2.4e6
C = 3
N = 20000   # samples per call: long enough for the hot kernel (>= 3 tiles of hot slices)


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def headline_taps():
    return np.asarray(sa.design_iqbb_taps(100e3, 50e3, FS, 127), np.int32).reshape(-1, 2)


# 127 taps behind a 2-tap front pad in the 9-step window: tap i sits at window index i + 2, and K step s multiplies window
# indices 16s - 15 ... 16s + 15. Step 0 holds taps 0 ... 13 alone, step 8 taps 111 ... 126 alone.
def tapset(name):
    t = headline_taps().copy()
    if name == "headline":             # steps 0 and 8 zero
        pass
    elif name == "left_edge_live":     # step 0 live, step 8 zero: the full range
        t[4] = (3, -2)
    elif name == "right_edge_live":    # step 8 live: the full range
        t[122] = (0, 5)
    elif name == "one_tap_first":      # a single low-plane unit in the first tap: must not trim
        t[0] = (1, 0)
    elif name == "one_tap_last":       # ... in the last tap, imaginary part only
        t[126] = (0, -1)
    elif name == "high_byte_only":     # an edge tap with a zero low byte: the high plane needs step 0, the low plane does not
        t[1] = (256, 0)
    elif name == "narrow":             # only taps 40 ... 90: steps 2 ... 6, inside the trimmed range
        t[:40] = 0
        t[91:] = 0
    else:
        raise ValueError(name)
    return t


EXPECT_TRIM = {"headline": True, "left_edge_live": False, "right_edge_live": False, "one_tap_first": False, "one_tap_last": False,
               "high_byte_only": False, "narrow": True}


def make(ctx, taps, epi, cu8, trim, monkeypatch, Fc=100e3):
    if trim:
        monkeypatch.delenv("SDRHIP_IQBB_TRIM", raising=False)
    else:
        monkeypatch.setenv("SDRHIP_IQBB_TRIM", "0")
    monkeypatch.delenv("SDRHIP_IQBB_HOT", raising=False)
    monkeypatch.delenv("SDRHIP_IQBB_PATH", raising=False)
    lut, inc = sa.design_freqshift_lut_i16(), sa.design_freqshift_inc(Fc, FS)
    node = sa.IQBaseBandI16(ctx, taps, lut, inc, Fc < 0, 8, channels=C, max_in=4 * N, epilogue=epi)
    if cu8:
        node.set_input_format(sa.abi.IN_CU8)
    monkeypatch.delenv("SDRHIP_IQBB_TRIM", raising=False)
    return node


def oracle_chain(orc, taps, epi, Fc=100e3):
    lut, inc = orc.freqshift_lut_i16(), orc.freqshift_inc(Fc, FS)
    bb, fm = orc.IQBaseBandI16(taps, lut, inc, Fc < 0, 8), orc.FMDemodI16()

    def run(x):
        r = bb.process(x)
        if epi == sa.EPI_FM:
            return fm.process(r) if len(r) else np.zeros(0, np.int16)
        return orc.am_i16(r) if epi == sa.EPI_AM else orc.usb_i16(r) if epi == sa.EPI_USB else r
    return bb, run


def gen(rng, cu8, n):
    return rng.integers(0, 256, (C, n, 2), dtype=np.uint8) if cu8 else rng.integers(-32768, 32768, (C, n, 2), dtype=np.int16)


def test_headline_plan_reports_low_range(ctx, monkeypatch):
    node = make(ctx, headline_taps(), sa.EPI_FM, False, True, monkeypatch)
    p = node.plan_info
    assert (p["path"], p["S"], p["S0"], p["NH"], p["L0"], p["NL"]) == (1, 9, 2, 5, 1, 7)
    assert node.kernel_names == ["iqbb_hot_kernel"]
    full = make(ctx, headline_taps(), sa.EPI_FM, False, False, monkeypatch).plan_info
    assert (full["S0"], full["NH"], full["L0"], full["NL"]) == (2, 5, 0, 9)


@pytest.mark.parametrize("cu8", [False, True])
@pytest.mark.parametrize("epi", [sa.EPI_FM, sa.EPI_USB, sa.EPI_AM, sa.EPI_NONE])
@pytest.mark.parametrize("name", sorted(EXPECT_TRIM))
def test_tap_classes_vs_oracle_and_full_range(ctx, orc, monkeypatch, name, epi, cu8):
    taps = tapset(name)
    node = make(ctx, taps, epi, cu8, True, monkeypatch)
    full = make(ctx, taps, epi, cu8, False, monkeypatch)
    p = node.plan_info
    assert p["path"] == 1 and p["S"] == 9
    assert ((p["L0"], p["NL"]) == (1, 7)) == EXPECT_TRIM[name], p
    assert p["L0"] <= p["S0"] and p["S0"] + p["NH"] <= p["L0"] + p["NL"]
    assert (full.plan_info["L0"], full.plan_info["NL"]) == (0, 9)
    refs = [oracle_chain(orc, taps, epi)[1] for _ in range(C)]
    rng = np.random.default_rng(len(name) * 7 + epi + 10 * int(cu8))
    for n in (N, N + 13, 3 * N):
        x = gen(rng, cu8, n)
        y, yf = node.process(x), full.process(x)
        assert np.array_equal(y, yf), (name, n)
        for c in range(C):
            r = refs[c](orc.autocast_cu8_cs16(x[c]) if cu8 else x[c])
            assert y[c].shape == r.shape and np.array_equal(y[c], r), (name, n, c)


@pytest.mark.parametrize("cu8", [False, True])
def test_retap_moves_support_across_classes_midstream(ctx, orc, monkeypatch, cu8):
    """set_taps between calls re-selects the range: trimmed -> full (an edge tap) -> trimmed -> full (high byte at the edge)."""
    epi = sa.EPI_FM
    seq = ["headline", "one_tap_first", "narrow", "high_byte_only", "headline"]
    node = make(ctx, tapset(seq[0]), epi, cu8, True, monkeypatch)
    full = make(ctx, tapset(seq[0]), epi, cu8, False, monkeypatch)
    chains = [oracle_chain(orc, tapset(seq[0]), epi) for _ in range(C)]
    rng = np.random.default_rng(5 + int(cu8))
    for k, name in enumerate(seq):
        if k:
            node.set_taps(tapset(name))
            full.set_taps(tapset(name))
            for bb, _ in chains:
                bb.set_taps(tapset(name))
        p = node.plan_info
        assert ((p["L0"], p["NL"]) == (1, 7)) == EXPECT_TRIM[name], (name, p)
        assert (full.plan_info["L0"], full.plan_info["NL"]) == (0, 9)
        x = gen(rng, cu8, N + 37 * k)
        y, yf = node.process(x), full.process(x)
        assert np.array_equal(y, yf), name
        for c in range(C):
            r = chains[c][1](orc.autocast_cu8_cs16(x[c]) if cu8 else x[c])
            assert np.array_equal(y[c], r), (name, c)


@pytest.mark.parametrize("cu8", [False, True])
@pytest.mark.parametrize("epi", [sa.EPI_FM, sa.EPI_USB])
def test_multi_buffer_calls_trimmed(ctx, orc, monkeypatch, epi, cu8):
    """process_multi (buffer boundaries kept, FMDemod restarting per buffer) with the trimmed plan: equal to the full range
    and to the oracle fed buffer by buffer."""
    taps = tapset("headline")
    node = make(ctx, taps, epi, cu8, True, monkeypatch)
    full = make(ctx, taps, epi, cu8, False, monkeypatch)
    assert (node.plan_info["L0"], node.plan_info["NL"]) == (1, 7)
    lut, inc = orc.freqshift_lut_i16(), orc.freqshift_inc(100e3, FS)
    bbs = [orc.IQBaseBandI16(taps, lut, inc, False, 8) for _ in range(C)]
    fms = [orc.FMDemodI16() for _ in range(C)]   # (FMDemod's index 1 of a buffer takes the previous buffer's last angle)
    rng = np.random.default_rng(11 + epi + int(cu8))
    for B, nb in ((4, 16384), (3, 23333)):
        x = gen(rng, cu8, B * nb)
        (y, counts), (yf, countsf) = node.process_multi(x, B), full.process_multi(x, B)
        assert counts == countsf and np.array_equal(y, yf), (B, nb)
        for c in range(C):
            rs = []
            for j in range(B):
                xb = x[c, j * nb:(j + 1) * nb]
                r = bbs[c].process(orc.autocast_cu8_cs16(xb) if cu8 else xb)
                if epi == sa.EPI_FM:
                    r = fms[c].process(r) if len(r) else np.zeros(0, np.int16)
                else:
                    r = orc.usb_i16(r)
                rs.append(r)
            assert counts == [len(r) for r in rs]
            assert np.array_equal(y[c], np.concatenate(rs)), (B, nb, c)
