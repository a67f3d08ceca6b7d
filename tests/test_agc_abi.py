"""The AGC bank's C calls (include/sdrhip_agc.h), what can be checked without a GPU: every function of the header is exported by
libsdrhip.so and has a prototype in libsdr_amd/abi_agc.py, and nothing else of the family is exported (tests/test_side_headers.py holds what the
headers' bindings owe each other); the designers give the reference's numbers; every argument rule of the two create calls answers BEFORE the
context is looked at, in the header's order; the calls on a handle refuse a NULL one; both kernels exist for gfx950 and use no
scratch."""
import ctypes as C

import numpy as np
import pytest

import agc_restatement as R
from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes

NEW = ["sdrhip_agc_create", "sdrhip_agc_destroy", "sdrhip_agc_get_state", "sdrhip_agc_kernel_names", "sdrhip_agc_plan_info", "sdrhip_agc_process",
       "sdrhip_agc_process_dev", "sdrhip_agc_reset", "sdrhip_agc_set_channel", "sdrhip_agc_set_enabled", "sdrhip_agc_set_gain",
       "sdrhip_agc_set_lambda", "sdrhip_agcbank_create", "sdrhip_design_agc_lambda", "sdrhip_design_agc_target"]
ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_agc
    assert_header_binding(abi_agc, NEW, r"\b(sdrhip_(?:design_)?agc[a-z0-9_]*)\b")


def test_the_package_exports_this_modules_classes():
    import libsdr_amd
    from libsdr_amd import agc
    assert libsdr_amd.AGC is agc.AGC and libsdr_amd.AGCBank is agc.AGCBank
    assert issubclass(agc.AGCBank, nodes._EqualLength) and issubclass(agc.AGC, agc.AGCBank)


@pytest.mark.parametrize("tau,Fs", [(0.1, 22050.0), (0.02, 22050.0), (0.002, 48000.0), (0.001, 8000.0), (0.25, 2.4e6 / 8)])
def test_designers(tau, Fs):
    from libsdr_amd import abi_agc
    L, v = abi_agc.lib(), C.c_float(0)
    assert L.sdrhip_design_agc_lambda(tau, Fs, C.byref(v)) == abi.OK
    assert np.float32(v.value).view(np.uint32) == R.design_lambda(tau, Fs).view(np.uint32)
    assert L.sdrhip_design_agc_target(0, C.byref(v)) == abi.OK and v.value == 16000.0
    assert L.sdrhip_design_agc_target(1, C.byref(v)) == abi.OK and v.value == 0.5
    assert L.sdrhip_design_agc_target(2, C.byref(v)) == abi.E_INVALID and "dtype" in last_error()
    assert L.sdrhip_design_agc_lambda(tau, Fs, None) == abi.E_INVALID and L.sdrhip_design_agc_target(0, None) == abi.E_INVALID
    assert L.sdrhip_design_agc_lambda(0.0, Fs, C.byref(v)) == abi.E_INVALID and L.sdrhip_design_agc_lambda(tau, -1.0, C.byref(v)) == abi.E_INVALID


def test_designed_lambda_matches_the_fixtures():
    from libsdr_amd import agc
    for name, m in R.manifest().items():
        assert np.float32(agc.design_agc_lambda(m["tau"], m["Fs"])).view(np.uint32) == m["lambda_bits"], name


def _bank(dtype=0, lam=(0.5, 0.0, 0.99), target=(1.0, 2.0, 16000.0), enabled=(1, 0, 1), channels=None, max_in=1024, null=()):
    """(code, out) of sdrhip_agcbank_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_agc
    lam, target, en = np.ascontiguousarray(lam, np.float32), np.ascontiguousarray(target, np.float32), np.ascontiguousarray(enabled, np.intc)
    h = C.c_void_p(0x1)
    code = abi_agc.lib().sdrhip_agcbank_create(None, dtype, None if "lambda" in null else lam.ctypes.data_as(fp),
                                               None if "target" in null else target.ctypes.data_as(fp),
                                               None if "enabled" in null else en.ctypes.data_as(ip), lam.size if channels is None else channels,
                                               max_in, None if "out" in null else C.byref(h))
    return code, h.value


def _one(dtype=0, lam=0.5, target=16000.0, channels=3, max_in=1024, null=()):
    from libsdr_amd import abi_agc
    h = C.c_void_p(0x1)
    return abi_agc.lib().sdrhip_agc_create(None, dtype, lam, target, channels, max_in, None if "out" in null else C.byref(h)), h.value


def test_create_without_a_context():
    for code, h in (_bank(), _one(), _bank(dtype=1), _one(dtype=1), _one(lam=0.0), _one(channels=1), _one(channels=65535), _one(max_in=1),
                    _one(max_in=(1 << 30) - 1), _one(lam=float(np.nextafter(np.float32(1), np.float32(0))))):
        assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


INF, NAN = float("inf"), float("nan")
BANK_RULES = [
    (dict(null=("lambda",)), abi.E_INVALID, "NULL"), (dict(null=("target",)), abi.E_INVALID, "NULL"), (dict(null=("enabled",)), abi.E_INVALID, "NULL"),
    (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(dtype=2), abi.E_INVALID, "dtype"), (dict(dtype=-1), abi.E_INVALID, "dtype"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=65536), abi.E_INVALID, "channels"),
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(max_in=1 << 30), abi.E_SIZE, "max_in"),
    (dict(lam=(0.5, 1.0, 0.5)), abi.E_INVALID, "lambda"), (dict(lam=(0.5, 0.5, -0.001)), abi.E_INVALID, "lambda"), (dict(lam=(NAN, 0.5, 0.5)), abi.E_INVALID, "lambda"),
    (dict(target=(1.0, 0.0, 1.0)), abi.E_INVALID, "target"), (dict(target=(1.0, 1.0, -2.0)), abi.E_INVALID, "target"),
    (dict(target=(INF, 1.0, 1.0)), abi.E_INVALID, "target"), (dict(target=(1.0, NAN, 1.0)), abi.E_INVALID, "target"),
    # in the header's order
    (dict(null=("out",), dtype=2), abi.E_INVALID, "NULL"), (dict(dtype=2, channels=0), abi.E_INVALID, "dtype"),
    (dict(channels=0, max_in=0), abi.E_INVALID, "channels"), (dict(max_in=0, lam=(1.0, 1.0, 1.0)), abi.E_SIZE, "max_in"),
    (dict(lam=(0.5, 1.0, 0.5), target=(0.0, 1.0, 1.0)), abi.E_INVALID, "lambda"),
]
ONE_RULES = [
    (dict(null=("out",)), abi.E_INVALID, "NULL"), (dict(dtype=2), abi.E_INVALID, "dtype"), (dict(channels=0), abi.E_INVALID, "channels"),
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(lam=1.0), abi.E_INVALID, "lambda"), (dict(lam=-0.5), abi.E_INVALID, "lambda"),
    (dict(target=0.0), abi.E_INVALID, "target"), (dict(target=INF), abi.E_INVALID, "target"), (dict(target=-1.0), abi.E_INVALID, "target"),
]


@pytest.mark.parametrize("kw,want,text", BANK_RULES, ids=[str(i) for i in range(len(BANK_RULES))])
def test_bank_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _bank(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


@pytest.mark.parametrize("kw,want,text", ONE_RULES, ids=[str(i) for i in range(len(ONE_RULES))])
def test_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _one(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_agc
    L = abi_agc.lib()
    g, e, t = (C.c_float * 4)(), (C.c_int * 4)(), C.c_int(7)
    buf = C.create_string_buffer(64)
    assert L.sdrhip_agc_process_dev(None, None, 0, 0, None, 0) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_agc_process(None, None, 0, 0, None, 0) == abi.E_INVALID and "NULL" in last_error()
    for call in (lambda: L.sdrhip_agc_set_channel(None, 0, 0.5, 1.0), lambda: L.sdrhip_agc_set_lambda(None, 0, 0.5),
                 lambda: L.sdrhip_agc_set_enabled(None, 0, 1), lambda: L.sdrhip_agc_set_gain(None, 0, 1.0),
                 lambda: L.sdrhip_agc_get_state(None, g, g, e, 4), lambda: L.sdrhip_agc_reset(None),
                 lambda: L.sdrhip_agc_kernel_names(None, buf, 64)):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_agc_plan_info(None, 16, C.byref(t), None) == abi.E_INVALID and t.value == 7
    assert L.sdrhip_agc_destroy(None) == abi.OK


def test_both_kernels_exist_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(agc_[a-z0-9_]+_kernel)")
    assert seen == {"agc_i16_kernel": 0, "agc_f32_kernel": 0}, seen
