"""The real-input tuner bank's create calls (sdrhip_tunerbb_i16_create / sdrhip_tunermodes_bb_i16_create: C BaseBand<int16_t>
channels over ONE row of real int16 samples), what can be checked without a GPU: declared in include/sdrhip.h with the complex
bank's parameter lists, bound in libsdr_amd/abi.py, exported by libsdrhip.so; their argument rules, which are checked before
the context and so answer on a machine without a device too; the no-device answer; the kernels exist for gfx950 under names of
their own; nodes.TunerBankI16 has the real form."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from abi_checks import kernel_scratch, no_ctx_code
from libsdr_amd import abi, nodes

REAL_FUNCTIONS = {"sdrhip_tunerbb_i16_create": "sdrhip_tuner_i16_create", "sdrhip_tunermodes_bb_i16_create": "sdrhip_tunermodes_i16_create"}

ORDER, CHANNELS = 21, 3
i32p, u32p, ip = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)


def _declaration(name):
    src = re.sub(r"/\*.*?\*/", "", open(abi.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_real_create_calls_are_declared_bound_and_exported():
    L = abi.lib()
    declared = abi.header_functions()
    fresh = C.CDLL(abi.SO_PATH)   # (looked up by name in the library's own export table, not through the binding)
    for f, twin in REAL_FUNCTIONS.items():
        assert f in declared, f
        assert f in L._declared and hasattr(L, f), f
        assert C.cast(getattr(fresh, f), C.c_void_p).value, f
        # the complex bank's parameter list, in the header and in the binding
        assert _declaration(f) == _declaration(twin), f
        assert getattr(L, f).argtypes == getattr(L, twin).argtypes and getattr(L, f).restype == getattr(L, twin).restype, f
    assert _declaration("sdrhip_tunerbb_i16_create")[-1] == "sdrhip_tuner_i16 **out"


def test_python_node_has_the_real_form():
    p = inspect.signature(nodes.TunerBankI16.__init__).parameters
    assert "real" in p and p["real"].default is False
    assert "modes" in p


def _args(taps=None, order=ORDER, decim=8, channels=CHANNELS, max_in=4096):
    if taps is None:
        taps = np.stack([nodes.design_bb_taps(1e3 * (c + 1), 3e3, 2.0e6, ORDER).reshape(-1, 2) for c in range(CHANNELS)])
    taps = np.ascontiguousarray(taps, np.int32)
    lut = np.ascontiguousarray(nodes.design_freqshift_lut_i16(), np.int32)
    inc, neg = np.arange(1, CHANNELS + 1, dtype=np.uint32), np.zeros(CHANNELS, np.intc)
    return dict(taps=taps, order=order, lut=lut, inc=inc, neg=neg, decim=decim, channels=channels, max_in=max_in)


def _create(a, epilogue=abi.EPI_NONE, modes=None, null=()):
    """(code, *out) of the create call with a NULL context; `null` names the pointer arguments passed as NULL."""
    p = lambda k, t: None if k in null else a[k].ctypes.data_as(t)
    h = C.c_void_p(0x1)
    out = None if "out" in null else C.byref(h)
    if modes is None:
        code = abi.lib().sdrhip_tunerbb_i16_create(None, p("taps", i32p), a["order"], p("lut", i32p), p("inc", u32p), p("neg", ip),
                                                   a["decim"], a["channels"], a["max_in"], epilogue, out)
    else:
        m = None if "modes" in null else np.ascontiguousarray(modes, np.intc).ctypes.data_as(ip)
        code = abi.lib().sdrhip_tunermodes_bb_i16_create(None, p("taps", i32p), a["order"], p("lut", i32p), p("inc", u32p), p("neg", ip), m,
                                                         a["decim"], a["channels"], a["max_in"], out)
    return code, h.value


MODES = [abi.EPI_FM, abi.EPI_AM, abi.EPI_USB]


@pytest.mark.parametrize("per_channel", [False, True], ids=["one_epilogue", "modes"])
def test_null_context(per_channel):
    """Valid arguments and no context: SDRHIP_E_NODEVICE where no device exists (there is no CPU fallback), the invalid argument
    it is in every create call elsewhere; *out is NULL."""
    code, h = _create(_args(), modes=MODES if per_channel else None)
    assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert b"no CPU fallback" in abi.lib().sdrhip_last_error()


@pytest.mark.parametrize("per_channel", [False, True], ids=["one_epilogue", "modes"])
def test_argument_rules_come_before_the_context(per_channel):
    modes = MODES if per_channel else None
    for null in ("taps", "lut", "inc", "neg", "out") + (("modes",) if per_channel else ()):
        code, h = _create(_args(), modes=modes, null=(null,))
        assert code == abi.E_INVALID and (h is None or null == "out"), null
    for kw, want in ((dict(order=0), abi.E_UNSUPPORTED), (dict(order=514), abi.E_UNSUPPORTED),
                     (dict(decim=0), abi.E_INVALID), (dict(decim=513), abi.E_UNSUPPORTED),
                     (dict(channels=0), abi.E_INVALID), (dict(channels=8193), abi.E_INVALID), (dict(max_in=0), abi.E_SIZE)):
        a = _args(**kw)
        if "order" in kw and kw["order"] > ORDER:   # (the array the call reads: order x channels taps)
            a["taps"] = np.zeros((CHANNELS, kw["order"], 2), np.int32)
        code, h = _create(a, modes=modes)
        assert code == want and h is None, (kw, code)
    # taps: any |component| < 2^23, as sdrhip_bb_i16_create
    for v, ok in ((1 << 23, False), (-(1 << 23), False), ((1 << 23) - 1, True), (-(1 << 23) + 1, True)):
        for comp in (0, 1):
            a = _args()
            a["taps"][CHANNELS - 1, ORDER - 1, comp] = v
            code, h = _create(a, modes=modes)
            assert code == (no_ctx_code() if ok else abi.E_UNSUPPORTED) and h is None, (v, comp, code)
    if per_channel:
        for bad in ([abi.EPI_NONE] + MODES[1:], MODES[:2] + [7], MODES[:2] + [-1]):
            code, h = _create(_args(), modes=bad)
            assert code == abi.E_INVALID and h is None, bad
    else:
        for epi in (-1, 4):
            code, h = _create(_args(), epilogue=epi)
            assert code == abi.E_INVALID and h is None, epi


def test_real_bank_kernels_exist_under_their_own_names(tmp_path):
    """Both forms x four epilogues, and one instance per form that reads the demodulator per channel: tuner_bb_i16_* — no name
    of the complex bank's set (tests/test_tuner_cpu.py, tests/test_tuner_modes_abi.py count those)."""
    names = set(kernel_scratch(tmp_path, "tuner_bb_i16_"))
    for form in ("valu", "mfma"):
        assert sum("tuner_bb_i16_%s_kernel" % form in n for n in names) == 4, sorted(names)
        assert sum("tuner_bb_i16_modes_%s_kernel" % form in n for n in names) == 1, sorted(names)
    assert len(names) == 10, sorted(names)
