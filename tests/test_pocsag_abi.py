"""The POCSAG decoder bank's C calls (include/sdrhip_pocsag.h), what can be checked without a GPU: every function of the header is
exported by libsdrhip.so and has a prototype in libsdr_amd/abi_pocsag.py, and nothing else of the family is exported; the
wrappers live in a module of their own (what the headers' bindings owe each other: tests/test_side_headers.py); every
argument rule of create answers BEFORE the context is looked at, in the header's order; the calls on a handle refuse a NULL one;
the kernel exists for gfx950 and uses no scratch."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes

NEW = ["sdrhip_pocsag_channel_state", "sdrhip_pocsag_create", "sdrhip_pocsag_destroy", "sdrhip_pocsag_get_enabled", "sdrhip_pocsag_kernel_names",
       "sdrhip_pocsag_out_capacity", "sdrhip_pocsag_process", "sdrhip_pocsag_process_dev", "sdrhip_pocsag_reset", "sdrhip_pocsag_reset_channel",
       "sdrhip_pocsag_set_enabled"]
ip = C.POINTER(C.c_int)


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_pocsag
    assert_header_binding(abi_pocsag, NEW, r"\b(sdrhip_pocsag_[a-z0-9_]+)\b")


def test_the_wrappers_live_in_a_module_of_their_own():
    import libsdr_amd
    from libsdr_amd import pocsag
    assert not hasattr(nodes, "POCSAGBank") and not hasattr(nodes, "MessageAssembler")
    assert libsdr_amd.POCSAGBank is pocsag.POCSAGBank and libsdr_amd.MessageAssembler is pocsag.MessageAssembler


def test_out_capacity_is_the_headers_formula():
    from libsdr_amd import abi_pocsag
    L = abi_pocsag.lib()
    for n in (0, 1, 31, 32, 255, 256, 446, 2048, 65536):
        assert L.sdrhip_pocsag_out_capacity(n) == n // 32 + n // 256 + 4


def _create(enabled=(1, 0, 1), channels=None, max_bits=2048, null=()):
    """(code, out) of sdrhip_pocsag_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_pocsag
    en = np.ascontiguousarray(enabled, np.intc)
    h = C.c_void_p(0x1)
    code = abi_pocsag.lib().sdrhip_pocsag_create(None, None if "enabled" in null else en.ctypes.data_as(ip),
                                                 en.size if channels is None else channels, max_bits, None if "out" in null else C.byref(h))
    return code, h.value


def test_create_without_a_context():
    code, h = _create()
    assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()
    # the limits are valid: 1 and 8192 channels, 1 and 65536 bits
    assert _create(enabled=(1,))[0] == no_ctx_code() and _create(enabled=(1,) * 8192)[0] == no_ctx_code()
    assert _create(max_bits=1)[0] == no_ctx_code() and _create(max_bits=65536)[0] == no_ctx_code()


RULES = [
    (dict(null=("enabled",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=-1), abi.E_INVALID, "channels"),
    (dict(enabled=(1,) * 8193), abi.E_INVALID, "channels"),
    (dict(max_bits=0), abi.E_SIZE, "max_bits"), (dict(max_bits=65537), abi.E_SIZE, "max_bits"),
    # in the header's order: the pointers before channels, channels before max_bits
    (dict(null=("enabled",), channels=0), abi.E_INVALID, "NULL"), (dict(null=("out",), max_bits=0), abi.E_INVALID, "NULL"),
    (dict(channels=0, max_bits=0), abi.E_INVALID, "channels"),
]


@pytest.mark.parametrize("kw,want,text", RULES, ids=[str(i) for i in range(len(RULES))])
def test_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _create(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_pocsag
    L = abi_pocsag.lib()
    e, s = (C.c_int * 4)(), C.c_int(7)
    buf = C.create_string_buffer(64)
    assert L.sdrhip_pocsag_process_dev(None, None, 0, None, None, 0, None, None) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_pocsag_process(None, None, 0, None, None, 0, None) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_pocsag_set_enabled(None, 0, 1) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_pocsag_get_enabled(None, e, 4) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_pocsag_reset(None) == abi.E_INVALID and L.sdrhip_pocsag_reset_channel(None, 0) == abi.E_INVALID
    assert L.sdrhip_pocsag_channel_state(None, 0, C.byref(s), None, None, None) == abi.E_INVALID and s.value == 7
    assert L.sdrhip_pocsag_kernel_names(None, buf, 64) == abi.E_INVALID
    assert L.sdrhip_pocsag_destroy(None) == abi.OK


def test_the_kernel_exists_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(pocsag_[a-z0-9_]+_kernel)")
    assert seen == {"pocsag_decode_kernel": 0}, seen
