"""CPU checks of the symbol path (FSKDetector, ASKDetector<int16_t>, BitStream): the numpy restatement
(tests/fsk_restatement.py) reproduces every g18 fixture cut from the reference (tools/golden_fsk) with zero differing symbols
and bits and identical per-buffer bit counts, and the product's LUT designer equals the fixture LUTs bit for bit."""
import json
import os

import numpy as np
import pytest

import fsk_restatement as fr
from abi_checks import kernel_scratch
from libsdr_amd import abi, nodes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_DT = {"u8": np.uint8, "i16": np.int16, "i32": np.int32, "cf32": np.float32}


class G18:
    def __init__(self):
        with open(os.path.join(GOLDEN, "manifest_fsk.json")) as f:
            self.manifest = json.load(f)

    def meta(self, name):
        return self.manifest[name]

    def load(self, name):
        m = self.manifest[name]
        a = np.fromfile(os.path.join(GOLDEN, m["file"]), dtype=_DT[m["dtype"]])
        assert a.size == m["count"], name
        return a.reshape(-1, 2) if m["dtype"] == "cf32" else a


@pytest.fixture(scope="module")
def g18():
    return G18()


def split(x, lens):
    out, off = [], 0
    for n in lens:
        out.append(x[off:off + n])
        off += n
    return out


FSK_CASES = ["g18_ax25", "g18_rtty", "g18_reconf"]
MODES = {"normal": fr.NORMAL, "transition": fr.TRANSITION}


def test_manifest_is_complete_and_small(g18):
    biggest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("g18_") and f.endswith(".bin"))
    for name, m in g18.manifest.items():
        assert name.startswith("g18_") and set(m) >= {"file", "dtype", "count"}
        assert os.path.getsize(os.path.join(GOLDEN, m["file"])) <= biggest
    on_disk = sorted(f for f in os.listdir(GOLDEN) if f.startswith("g18_"))
    assert on_disk == sorted(m["file"] for m in g18.manifest.values())
    assert g18.meta("g18_ax25_x")["corr_len"] == 18 and g18.meta("g18_rtty_x")["corr_len"] == 242
    assert 0 in g18.meta("g18_ax25_x")["lens"] and 1 in g18.meta("g18_ax25_x")["lens"]


@pytest.mark.parametrize("case", FSK_CASES)
def test_fsk_symbols_and_bits_restated(g18, case):
    m = g18.meta(case + "_x")
    x, lens = g18.load(case + "_x"), m["lens"]
    want_sym = g18.load(case + "_sym")
    assert fr.corr_len(m["Fs"], m["baud"]) == m["corr_len"]
    for mode_name, mode in MODES.items():
        det = fr.FSKDetector(g18.load(case + "_lut_mark"), g18.load(case + "_lut_space"))
        bits = fr.BitStream(m["Fs"], m["baud"], mode)
        sym, out, counts = [], [], []
        for b, buf in enumerate(split(x, lens)):
            if b == m["reconf_at"]:
                det.reset()
                bits.reset()
            s = det.process(buf)[0]
            o = bits.process(s)[0]
            sym.append(s)
            out.append(o)
            counts.append(o.size)
        sym, out = np.concatenate(sym), np.concatenate(out)
        assert sym.size == want_sym.size and int((sym != want_sym).sum()) == 0
        want = g18.load("%s_bits_%s" % (case, mode_name))
        assert counts == list(g18.load("%s_bits_%s_counts" % (case, mode_name)))
        assert out.size == want.size and int((out != want).sum()) == 0
        assert want.size > 20 and 0 < int(want.sum()) < want.size   # a fixture that is neither empty nor constant


def test_fixture_inputs_cover_the_edges(g18):
    x = g18.load("g18_ax25_x")
    assert x.max() == 32767 and x.min() == -32768                    # full-scale samples
    assert np.flatnonzero(x == 0).size >= 700                        # exact silence ...
    sym = g18.load("g18_ax25_sym")
    assert not sym[2500 + 18:2500 + 700].any()                       # ... gives f == 0: symbol 0
    assert sym.any() and g18.load("g18_ax25_bits_normal_counts")[5] == 0   # the empty buffer produced no bits


def test_ask_restated(g18):
    m = g18.meta("g18_ask_x")
    x = g18.load("g18_ask_x")
    for inv in (0, 1):
        sym = fr.ask_detect(x, bool(inv))
        assert np.array_equal(sym, g18.load("g18_ask_inv%d_sym" % inv))
        bits = fr.BitStream(m["Fs"], m["baud"], fr.NORMAL)
        out = [bits.process(s)[0] for s in split(sym, m["lens"])]
        assert [o.size for o in out] == list(g18.load("g18_ask_inv%d_bits_normal_counts" % inv))
        assert np.array_equal(np.concatenate(out), g18.load("g18_ask_inv%d_bits_normal" % inv))
    assert np.array_equal(g18.load("g18_ask_inv0_sym") ^ 1, g18.load("g18_ask_inv1_sym"))


def test_restatement_is_independent_of_buffering(g18):
    """One long call and sample-by-sample calls give the ragged fixture's symbols: the carried state is complete."""
    x, want = g18.load("g18_ax25_x")[:600], g18.load("g18_ax25_sym")[:600]
    lm, ls = g18.load("g18_ax25_lut_mark"), g18.load("g18_ax25_lut_space")
    assert np.array_equal(fr.FSKDetector(lm, ls).process(x)[0], want)
    det = fr.FSKDetector(lm, ls)
    assert np.array_equal(np.concatenate([det.process(x[i:i + 1])[0] for i in range(600)]), want)


@pytest.mark.parametrize("case,tone", [(c, t) for c in ("g18_ax25", "g18_rtty") for t in ("mark", "space")])
def test_product_designer_fsk_lut(g18, case, tone):
    """The product's host designer against the reference node's own LUT, bit for bit (as the fftfilt and tap designers are)."""
    m = g18.meta("%s_lut_%s" % (case, tone))
    lut = nodes.design_fsk_lut(m["Fs"], m["baud"], m["F" + tone])
    want = g18.load("%s_lut_%s" % (case, tone))
    assert lut.shape == (m["corr_len"], 2) and lut.dtype == np.float32
    assert np.array_equal(lut.view(np.uint32), want.view(np.uint32))


def test_designer_argument_checks():
    import ctypes as C
    L = abi.lib()
    n = C.c_int(0)
    assert L.sdrhip_design_fsk_lut(22050.0, 1200.0, 1200.0, C.byref(n), None, 0) == abi.OK and n.value == 18
    buf = (C.c_float * 8)()
    assert L.sdrhip_design_fsk_lut(22050.0, 1200.0, 1200.0, C.byref(n), buf, 4) == abi.E_SIZE
    assert L.sdrhip_design_fsk_lut(0.0, 1200.0, 1200.0, C.byref(n), None, 0) == abi.E_INVALID
    assert L.sdrhip_design_fsk_lut(22050.0, 1200.0, 1200.0, None, None, 0) == abi.E_INVALID


def test_new_entry_points_are_declared_and_exported():
    L = abi.lib()
    new = [f for f in abi.header_functions() if f.startswith(("sdrhip_detector_", "sdrhip_bits_", "sdrhip_design_fsk_"))]
    assert len(new) == 15, new
    assert all(hasattr(L, f) for f in new) and set(new) <= set(L._declared)
    blob = open(abi.SO_PATH, "rb").read()
    for k in (b"fsk_detect_kernel", b"ask_detect_kernel", b"bits_flags_kernel", b"bits_pll_kernel"):
        assert k in blob


def test_symbol_kernels_keep_out_of_scratch(tmp_path):
    """The detector serves L = 18 and L = 242 from one kernel whose ring lives in LDS (L is a run-time argument): no
    scratch, whatever L. Read from the code object's own metadata, as tests/test_abi.py does for the hot kernels."""
    seen = kernel_scratch(tmp_path, "fsk_detect|ask_detect|bits_flags|bits_pll")
    assert len(seen) == 4 and not any(seen.values()), seen
