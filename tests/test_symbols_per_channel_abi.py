"""The per-channel symbol path's C calls (sdrhip_detectorbank_create / _set_channel, sdrhip_bitsbank_create /
_set_channel / _channel_info), what can be checked without a GPU: declared in include/sdrhip.h, bound in libsdr_amd/abi.py,
exported by libsdrhip.so; every argument rule of the create calls answers with its error code and a sdrhip_last_error text
BEFORE the context is looked at, so on a machine without a device too; the no-device answer; set_channel on a NULL handle; the
new kernels exist for gfx950 under names of their own, beside the one-parameter kernels, and none uses scratch."""
import ctypes as C
import re

import numpy as np
import pytest

from abi_checks import kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes

NEW = ["sdrhip_detectorbank_create", "sdrhip_detectorbank_set_channel", "sdrhip_bitsbank_create",
       "sdrhip_bitsbank_set_channel", "sdrhip_bitsbank_channel_info"]
ip, f32p = C.POINTER(C.c_int), C.POINTER(C.c_float)


def test_new_calls_are_declared_bound_and_exported():
    L = abi.lib()
    declared = abi.header_functions()
    fresh = C.CDLL(abi.SO_PATH)   # (looked up by name in the library's own export table, not through the binding)
    for f in NEW:
        assert f in declared, f
        assert f in L._declared and hasattr(L, f), f
        assert C.cast(getattr(fresh, f), C.c_void_p).value, f
    assert sorted(L._declared) == declared
    assert hasattr(nodes, "SymbolDetectorBank") and hasattr(nodes, "BitStreamBank")
    import libsdr_amd
    assert libsdr_amd.SymbolDetectorBank is nodes.SymbolDetectorBank and libsdr_amd.BitStreamBank is nodes.BitStreamBank
    assert callable(nodes.SymbolDetectorBank.set_channel) and callable(nodes.BitStreamBank.set_channel)


def _det(kinds=(abi.DET_FSK, abi.DET_ASK, abi.DET_FSK), lens=(18, 0, 5), max_corr_len=0, channels=None, max_in=4096, null=()):
    """(code, *out) of sdrhip_detectorbank_create with a NULL context; `null` names pointer arguments passed as NULL."""
    kinds, lens = np.ascontiguousarray(kinds, np.intc), np.ascontiguousarray(lens, np.intc)
    inv = np.zeros(kinds.size, np.intc)
    n = int(sum(max(int(l), 0) for k, l in zip(kinds, lens) if k == abi.DET_FSK))
    m, s = np.ones((max(n, 1), 2), np.float32), np.ones((max(n, 1), 2), np.float32)
    arg = {"kinds": kinds.ctypes.data_as(ip), "lens": lens.ctypes.data_as(ip), "inv": inv.ctypes.data_as(ip),
           "mark": m.ctypes.data_as(f32p), "space": s.ctypes.data_as(f32p)}
    a = lambda k: None if k in null else arg[k]
    h = C.c_void_p(0x1)
    code = abi.lib().sdrhip_detectorbank_create(None, a("kinds"), a("lens"), a("inv"), a("mark"), a("space"), max_corr_len,
                                                        kinds.size if channels is None else channels, max_in,
                                                        None if "out" in null else C.byref(h))
    return code, h.value


def _bits(bauds=(1200.0, 90.90, 2400.0), modes=(abi.BITS_NORMAL, abi.BITS_TRANSITION, abi.BITS_NORMAL), Fs=22050.0, max_corr_len=0,
          channels=None, max_in=4096, null=()):
    bauds, modes = np.ascontiguousarray(bauds, np.float32), np.ascontiguousarray(modes, np.intc)
    h = C.c_void_p(0x1)
    code = abi.lib().sdrhip_bitsbank_create(None, Fs, None if "baud" in null else bauds.ctypes.data_as(f32p),
                                                    None if "mode" in null else modes.ctypes.data_as(ip),
                                                    bauds.size if channels is None else channels, max_in, max_corr_len,
                                                    None if "out" in null else C.byref(h))
    return code, h.value


def test_null_context():
    """Valid arguments and no context: SDRHIP_E_NODEVICE where no device exists (there is no CPU fallback), the invalid
    argument it is in every create call elsewhere; *out is NULL."""
    for make in (_det, _bits):
        code, h = make()
        assert code == no_ctx_code() and h is None, make
        if nodes.device_count() == 0:
            assert "no CPU fallback" in last_error()
    # an ASK-only bank needs no LUTs
    code, h = _det(kinds=(abi.DET_ASK, abi.DET_ASK), lens=(0, 0), null=("mark", "space"))
    assert code == no_ctx_code() and h is None
    # max_corr_len = 2048 and corr_len = 2048 are the limits
    assert _det(kinds=(abi.DET_FSK,), lens=(2048,), max_corr_len=2048)[0] == no_ctx_code()
    assert _bits(bauds=(22050.0 / 2048,), modes=(0,), max_corr_len=2048)[0] == no_ctx_code()
    # 8192 channels x 2048 entries = 2^24: the largest LUT buffer a detector bank may ask for
    assert _det(kinds=(abi.DET_ASK,) * 8192, lens=(0,) * 8192, max_corr_len=2048, null=("mark", "space"))[0] == no_ctx_code()


DET_RULES = [
    (dict(null=("kinds",)), abi.E_INVALID, "NULL"), (dict(null=("lens",)), abi.E_INVALID, "NULL"),
    (dict(null=("inv",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(null=("mark",)), abi.E_INVALID, "LUT"), (dict(null=("space",)), abi.E_INVALID, "LUT"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=65536), abi.E_INVALID, "channels"),
    (dict(max_in=0), abi.E_SIZE, "max_in"),
    (dict(kinds=(abi.DET_FSK, 2, abi.DET_ASK)), abi.E_INVALID, "channel 1: bad kind 2"),
    (dict(kinds=(abi.DET_FSK, abi.DET_ASK, -1)), abi.E_INVALID, "channel 2: bad kind -1"),
    (dict(lens=(18, 0, 0)), abi.E_INVALID, "channel 2: corr_len 0 < 1"),
    (dict(lens=(-3, 0, 5)), abi.E_INVALID, "channel 0: corr_len -3 < 1"),
    (dict(lens=(18, 0, 2049)), abi.E_UNSUPPORTED, "channel 2: corr_len 2049"),
    (dict(max_corr_len=17), abi.E_UNSUPPORTED, "channel 0: corr_len 18 > max_corr_len 17"),
    (dict(max_corr_len=2049), abi.E_UNSUPPORTED, "max_corr_len 2049"),
    (dict(max_corr_len=-1), abi.E_INVALID, "max_corr_len -1"),
    # a LUT slot of max_corr_len float4 entries per channel: 8193 x 2048 > 2^24 entries (256 MiB)
    (dict(kinds=(abi.DET_ASK,) * 8193, lens=(0,) * 8193, max_corr_len=2048), abi.E_UNSUPPORTED, "LUT entries"),
]


@pytest.mark.parametrize("kw,want,text", DET_RULES, ids=[str(i) for i in range(len(DET_RULES))])
def test_detector_argument_rules_come_before_the_context(kw, want, text):
    code, h = _det(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


BITS_RULES = [
    (dict(null=("baud",)), abi.E_INVALID, "NULL"), (dict(null=("mode",)), abi.E_INVALID, "NULL"),
    (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=65536), abi.E_INVALID, "channels"),
    (dict(max_in=0), abi.E_SIZE, "max_in"),
    (dict(modes=(0, 2, 1)), abi.E_INVALID, "bad mode 2"), (dict(modes=(0, 1, -1)), abi.E_INVALID, "bad mode -1"),
    (dict(bauds=(1200.0, 0.0, 2400.0)), abi.E_INVALID, "positive"), (dict(Fs=0.0), abi.E_INVALID, "positive"),
    (dict(bauds=(1200.0, 90.90, 22051.0)), abi.E_INVALID, "fewer than one symbol per bit"),
    (dict(bauds=(1200.0, 10.0, 2400.0)), abi.E_UNSUPPORTED, "more than 2048 symbols per bit"),
    (dict(max_corr_len=241), abi.E_UNSUPPORTED, "more than 241 symbols per bit"),
    (dict(max_corr_len=2049), abi.E_UNSUPPORTED, "max_corr_len 2049"),
    (dict(max_corr_len=-1), abi.E_INVALID, "max_corr_len -1"),
]


@pytest.mark.parametrize("kw,want,text", BITS_RULES, ids=[str(i) for i in range(len(BITS_RULES))])
def test_bits_argument_rules_come_before_the_context(kw, want, text):
    code, h = _bits(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    L = abi.lib()
    lut = np.ones((18, 2), np.float32).ctypes.data_as(f32p)
    assert L.sdrhip_detectorbank_set_channel(None, 0, abi.DET_FSK, lut, lut, 18, 0) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_detectorbank_set_channel(None, 0, abi.DET_ASK, None, None, 0, 1) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_bitsbank_set_channel(None, 0, 1200.0, abi.BITS_NORMAL) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_bitsbank_channel_info(None, 0, 16, None, None, None, None) == abi.E_INVALID and "NULL" in last_error()


def test_per_channel_kernels_exist_beside_the_one_parameter_kernels(tmp_path):
    """Entry points of their own, the parent's kernels under their names, and no scratch in any of them."""
    scratch = {}
    want = ["detectorbank_kernel", "bitsbank_flags_kernel", "bitsbank_pll_kernel", "bitsbank_fill_kernel",
            "fsk_detect_kernel", "ask_detect_kernel", "bits_flags_kernel", "bits_pll_kernel", "bits_fill_kernel"]
    for name, b in kernel_scratch(tmp_path, r"\d(?:%s)[A-Z]" % "|".join(want)).items():   # (the mangled name: <length><name>E...)
        scratch.setdefault(re.search("|".join(want), name).group(0), []).append(b)
    assert sorted(scratch) == sorted(want), sorted(scratch)
    assert all(v == [0] for v in scratch.values()), scratch
