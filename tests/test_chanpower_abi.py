"""The channel power monitor's C calls (include/sdrhip_chanpower.h), what can be checked without a GPU: every function of the
header is exported by libsdrhip.so and has a prototype in libsdr_amd/abi_chanpower.py, and nothing else of the family is exported;
the header is registered in abi.LATER_SIDE_HEADERS and not in abi.SIDE_HEADERS, and its names are disjoint from every other
table's; the package exports the class; every argument rule of create — the channelizer's, then alpha — answers BEFORE the context
is looked at, in the header's order; the calls on a handle refuse a NULL one; and the three kernels exist for gfx950 and use no
scratch."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes

NEW = ["sdrhip_chanpower_create", "sdrhip_chanpower_destroy", "sdrhip_chanpower_get_levels", "sdrhip_chanpower_get_occupied",
       "sdrhip_chanpower_get_state", "sdrhip_chanpower_kernel_names", "sdrhip_chanpower_out_count", "sdrhip_chanpower_plan_info",
       "sdrhip_chanpower_process", "sdrhip_chanpower_process_dev", "sdrhip_chanpower_reset", "sdrhip_chanpower_set_alpha",
       "sdrhip_chanpower_set_taps", "sdrhip_chanpower_set_thresholds"]
dp = C.POINTER(C.c_double)
INF, NAN = float("inf"), float("nan")


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_chanpower
    assert_header_binding(abi_chanpower, NEW, r"\b(sdrhip_chanpower[a-z0-9_]*)\b")


def test_the_header_is_in_the_second_table_only():
    import libsdr_amd  # noqa: F401   (the package imports every side header's module)
    from libsdr_amd import abi_chanpower
    assert "sdrhip_chanpower.h" in abi.LATER_SIDE_HEADERS and "sdrhip_chanpower.h" not in abi.SIDE_HEADERS
    assert abi.LATER_SIDE_HEADERS["sdrhip_chanpower.h"].SIGNATURES is abi_chanpower.SIGNATURES
    assert not set(abi_chanpower.SIGNATURES) & set(abi.SIGNATURES)
    for name, side in list(abi.SIDE_HEADERS.items()) + list(abi.LATER_SIDE_HEADERS.items()):
        if name != "sdrhip_chanpower.h":
            assert not set(abi_chanpower.SIGNATURES) & set(side.SIGNATURES), name
    assert sorted(abi.lib()._declared) == abi.header_functions()
    assert abi.LATER_SIDE_HEADERS["sdrhip_chanpower.h"].header_functions() == sorted(NEW)


def test_the_package_exports_the_class():
    import libsdr_amd
    from libsdr_amd import chanpower
    assert libsdr_amd.ChannelPower is chanpower.ChannelPower and issubclass(chanpower.ChannelPower, nodes._Counted)


def _create(dtype=0, M=8, D=4, taps=None, n_taps=None, max_in=1024, alpha=0.5, null=()):
    """(code, out) of sdrhip_chanpower_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_chanpower
    t = np.ascontiguousarray(np.linspace(0.1, 1.0, 24) if taps is None else taps, np.float64)
    h = C.c_void_p(0x1)
    code = abi_chanpower.lib().sdrhip_chanpower_create(None, dtype, M, D, None if "taps" in null else t.ctypes.data_as(dp),
                                                       t.size if n_taps is None else n_taps, max_in, alpha, None if "out" in null else C.byref(h))
    return code, h.value


def test_create_without_a_context():
    for code, h in (_create(), _create(dtype=1), _create(M=2, D=1), _create(M=2, D=2, taps=[1.0]), _create(M=4096, D=4096),
                    _create(M=1000, D=500), _create(M=13 * 11 * 7, D=3), _create(max_in=1), _create(max_in=(1 << 30) - 1),
                    _create(alpha=1.0), _create(alpha=1e-300), _create(alpha=np.nextafter(1.0, 0.0))):
        assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


def _bad_taps(v):
    t = np.linspace(0.1, 1.0, 24)
    t[13] = v
    return t


RULES = [
    (dict(null=("taps",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(dtype=2), abi.E_INVALID, "dtype"), (dict(dtype=-1), abi.E_INVALID, "dtype"),
    (dict(M=1, D=1), abi.E_SIZE, "M 1"), (dict(M=4097), abi.E_SIZE, "M 4097"),
    (dict(M=17), abi.E_INVALID, "prime factor 17"), (dict(M=4093), abi.E_INVALID, "prime factor"),
    (dict(D=0), abi.E_INVALID, "D 0"), (dict(D=9), abi.E_INVALID, "D 9"),
    (dict(n_taps=0), abi.E_SIZE, "n_taps"), (dict(M=2, D=1, taps=np.ones(129)), abi.E_SIZE, "n_taps"),
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(max_in=1 << 30), abi.E_SIZE, "max_in"),
    (dict(taps=_bad_taps(NAN)), abi.E_INVALID, "tap 13"), (dict(taps=_bad_taps(1e39)), abi.E_INVALID, "tap 13"),
    (dict(alpha=0.0), abi.E_INVALID, "alpha"), (dict(alpha=-0.25), abi.E_INVALID, "alpha"), (dict(alpha=np.nextafter(1.0, 2.0)), abi.E_INVALID, "alpha"),
    (dict(alpha=NAN), abi.E_INVALID, "alpha"), (dict(alpha=INF), abi.E_INVALID, "alpha"),
    # in the header's order
    (dict(null=("out",), dtype=2), abi.E_INVALID, "NULL"), (dict(dtype=2, M=1), abi.E_INVALID, "dtype"), (dict(M=1, D=0), abi.E_SIZE, "M 1"),
    (dict(M=17, D=0), abi.E_INVALID, "prime"), (dict(D=0, n_taps=0), abi.E_INVALID, "D 0"), (dict(n_taps=0, max_in=0), abi.E_SIZE, "n_taps"),
    (dict(max_in=0, taps=_bad_taps(NAN)), abi.E_SIZE, "max_in"), (dict(taps=_bad_taps(NAN), alpha=0.0), abi.E_INVALID, "tap 13"),
]


@pytest.mark.parametrize("kw,want,text", RULES, ids=[str(i) for i in range(len(RULES))])
def test_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _create(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_chanpower
    L = abi_chanpower.lib()
    g, d, idx, t, sz, u = (C.c_float * 16)(), (C.c_double * 16)(), (C.c_int * 4)(0, 1, 2, 3), C.c_int(7), C.c_size_t(9), C.c_uint64(5)
    flags, buf = (C.c_ubyte * 16)(), C.create_string_buffer(64)
    for call in (lambda: L.sdrhip_chanpower_process_dev(None, None, 0, None, C.byref(sz)),
                 lambda: L.sdrhip_chanpower_process(None, None, 0, None, None),
                 lambda: L.sdrhip_chanpower_set_thresholds(None, d, d), lambda: L.sdrhip_chanpower_set_alpha(None, 0.5),
                 lambda: L.sdrhip_chanpower_set_taps(None, d), lambda: L.sdrhip_chanpower_reset(None),
                 lambda: L.sdrhip_chanpower_get_levels(None, d, flags, 16), lambda: L.sdrhip_chanpower_get_occupied(None, idx, 4, C.byref(t)),
                 lambda: L.sdrhip_chanpower_get_state(None, C.byref(u), g, 8, C.byref(u)), lambda: L.sdrhip_chanpower_kernel_names(None, buf, 64),
                 lambda: L.sdrhip_chanpower_plan_info(None, C.byref(t), None, None, None, None)):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert sz.value == 0 and t.value == 7 and u.value == 5
    sz.value = 9
    assert L.sdrhip_chanpower_out_count(None, 16, C.byref(sz)) == abi.E_INVALID and sz.value == 9
    assert L.sdrhip_chanpower_destroy(None) == abi.OK


def test_the_three_kernels_exist_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(chanpower_[a-z0-9]+_kernel)")
    assert seen == {"chanpower_cs16_kernel": 0, "chanpower_cf32_kernel": 0, "chanpower_finish_kernel": 0}, seen
