"""The receiver bank's C calls (include/sdrhip_rx.h), what can be checked without a GPU: every function of the header is
exported by libsdrhip.so and has a prototype in libsdr_amd/abi_rx.py, and nothing else has; the argument rules of the two new
create calls that answer BEFORE the context is looked at, so on a machine without a device too; the calls that exist for a bank
only refuse a NULL handle; the wrappers live in a module of their own (what the headers' bindings owe each other:
tests/test_side_headers.py); the de-emphasis kernels exist in both instances and none uses scratch."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes

NEW = ["sdrhip_deemphbank_i16_create", "sdrhip_deemphbank_i16_get_enabled", "sdrhip_deemphbank_i16_set_enabled", "sdrhip_rxbank_create",
       "sdrhip_rxbank_destroy", "sdrhip_rxbank_process", "sdrhip_rxbank_process_dev", "sdrhip_rxbank_sizes"]
ip = C.POINTER(C.c_int)


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_rx
    assert_header_binding(abi_rx, NEW, r"\b(sdrhip_(?:rxbank|deemphbank)_[a-z0-9_]+)\b")


def test_the_wrappers_live_in_a_module_of_their_own():
    import libsdr_amd
    from libsdr_amd import receiver
    assert not hasattr(nodes, "ReceiverBank") and not hasattr(nodes, "FMDeemphBankI16")
    assert libsdr_amd.ReceiverBank is receiver.ReceiverBank and libsdr_amd.FMDeemphBankI16 is receiver.FMDeemphBankI16
    assert issubclass(receiver.FMDeemphBankI16, nodes.FMDeemphI16)


def _deemph(alpha=2, enabled=(1, 0, 1), channels=None, max_in=4096, null=()):
    """(code, *out) of sdrhip_deemphbank_i16_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_rx
    en = np.ascontiguousarray(enabled, np.intc)
    h = C.c_void_p(0x1)
    code = abi_rx.lib().sdrhip_deemphbank_i16_create(None, alpha, None if "enabled" in null else en.ctypes.data_as(ip),
                                                     en.size if channels is None else channels, max_in,
                                                     None if "out" in null else C.byref(h))
    return code, h.value


def test_deemph_bank_without_a_context():
    code, h = _deemph()
    assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()
    # the limits are valid: alpha 1 and 32767, 8192 channels
    assert _deemph(alpha=1)[0] == no_ctx_code() and _deemph(alpha=32767)[0] == no_ctx_code()
    assert _deemph(enabled=(1,) * 8192)[0] == no_ctx_code()


DEEMPH_RULES = [
    (dict(null=("enabled",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(alpha=0), abi.E_INVALID, "alpha 0"), (dict(alpha=32768), abi.E_INVALID, "alpha 32768"), (dict(alpha=-3), abi.E_INVALID, "alpha -3"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(enabled=(1,) * 8193), abi.E_INVALID, "channels"),
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(max_in=1 << 30), abi.E_SIZE, "max_in"),
    # in the issue's order: the pointers before alpha, alpha before channels, channels before max_in
    (dict(null=("enabled",), alpha=0), abi.E_INVALID, "NULL"), (dict(alpha=0, channels=0), abi.E_INVALID, "alpha"),
    (dict(channels=0, max_in=0), abi.E_INVALID, "channels"),
]


@pytest.mark.parametrize("kw,want,text", DEEMPH_RULES, ids=[str(i) for i in range(len(DEEMPH_RULES))])
def test_deemph_bank_argument_rules_come_before_the_context(kw, want, text):
    code, h = _deemph(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_receiver_bank_create_rules_without_a_device():
    """A NULL tuner, detector, bits or out is SDRHIP_E_INVALID before anything is dereferenced (the other pointers here are
    never followed); with all four present, the NULL context answers next."""
    from libsdr_amd import abi_rx
    L = abi_rx.lib()
    fake = C.c_void_p(0x1000)
    out = C.c_void_p(0x1)
    for t, d, b, o in ((None, fake, fake, C.byref(out)), (fake, None, fake, C.byref(out)), (fake, fake, None, C.byref(out)),
                       (fake, fake, fake, None)):
        assert L.sdrhip_rxbank_create(None, t, None, d, b, o) == abi.E_INVALID and "NULL" in last_error()
    assert out.value is None
    out = C.c_void_p(0x1)
    assert L.sdrhip_rxbank_create(None, fake, None, fake, fake, C.byref(out)) == no_ctx_code() and out.value is None


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_rx
    L = abi_rx.lib()
    e = (C.c_int * 4)()
    n = C.c_size_t(7)
    assert L.sdrhip_deemphbank_i16_set_enabled(None, 0, 1) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_deemphbank_i16_get_enabled(None, e, 4) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_rxbank_sizes(None, 16, C.byref(n), None) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_rxbank_process_dev(None, None, 0, None, 0, None, None, 0, None) == abi.E_INVALID
    assert L.sdrhip_rxbank_process(None, None, 0, None, 0, None, None, 0, None) == abi.E_INVALID
    assert L.sdrhip_rxbank_destroy(None) == abi.OK


def test_deemph_kernels_exist_in_both_instances_without_scratch(tmp_path):
    """One body, two instances: deemph_i16_{seq,spec,copy}_kernel<false> (the one-parameter handle's) and <true> (the bank's)."""
    seen = kernel_scratch(tmp_path, r"\d(deemph_i16_(?:seq|spec|copy)_kernel)ILb([01])E")
    seen = {(k, int(b)): v for (k, b), v in seen.items()}
    assert sorted(seen) == [("deemph_i16_%s_kernel" % k, b) for k in ("copy", "seq", "spec") for b in (0, 1)], sorted(seen)
    assert not any(seen.values()), seen
