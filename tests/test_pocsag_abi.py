"""The POCSAG decoder bank's C calls (include/sdrhip_pocsag.h), what can be checked without a GPU: every function of the header is
exported by libsdrhip.so and has a prototype in libsdr_amd/abi_pocsag.py, and nothing else of the family is exported; sdrhip.h's and
sdrhip_rx.h's bindings and the wrapper set of nodes.py are what they were — the new surface lives in files of its own; every
argument rule of create answers BEFORE the context is looked at, in the header's order; the calls on a handle refuse a NULL one;
the kernel exists for gfx950 and uses no scratch."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from libsdr_amd import abi, nodes

LLVM = "/opt/rocm/lib/llvm/bin/"
NEW = ["sdrhip_pocsag_channel_state", "sdrhip_pocsag_create", "sdrhip_pocsag_destroy", "sdrhip_pocsag_get_enabled", "sdrhip_pocsag_kernel_names",
       "sdrhip_pocsag_out_capacity", "sdrhip_pocsag_process", "sdrhip_pocsag_process_dev", "sdrhip_pocsag_reset", "sdrhip_pocsag_reset_channel",
       "sdrhip_pocsag_set_enabled"]
ip = C.POINTER(C.c_int)
NO_CTX = lambda: abi.E_NODEVICE if nodes.device_count() == 0 else abi.E_INVALID


def _text():
    return abi.lib().sdrhip_last_error().decode()


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_pocsag
    declared = abi_pocsag.header_functions()
    assert declared == sorted(NEW)
    assert sorted(abi_pocsag.SIGNATURES) == declared
    fresh = C.CDLL(abi.SO_PATH)   # (looked up by name in the library's own export table, not through the binding)
    for f in declared:
        assert C.cast(getattr(fresh, f), C.c_void_p).value, f
    L = abi_pocsag.lib()
    assert L is abi.lib()
    for f, (res, args) in abi_pocsag.SIGNATURES.items():
        fn = getattr(L, f)
        assert fn.restype is res and list(fn.argtypes) == args, f
    syms = subprocess.run([LLVM + "llvm-readelf", "--dyn-syms", "-W", abi.SO_PATH], capture_output=True, text=True, check=True).stdout
    got = sorted(set(re.findall(r"\b(sdrhip_pocsag_[a-z0-9_]+)\b", syms)))
    assert got == declared


def test_the_frozen_surface_is_unchanged_by_this_module():
    from libsdr_amd import abi_rx
    before_sig, before_rx, before_decl = dict(abi.SIGNATURES), dict(abi_rx.SIGNATURES), list(abi.lib()._declared)
    wrappers = sorted(k for k, v in vars(nodes).items() if isinstance(v, type))
    from libsdr_amd import abi_pocsag, pocsag
    abi_pocsag.lib()
    assert abi.SIGNATURES == before_sig and abi_rx.SIGNATURES == before_rx and abi.lib()._declared == before_decl
    assert sorted(abi.lib()._declared) == abi.header_functions()
    for other in (abi.header_functions(), abi.SIGNATURES, abi_rx.header_functions(), abi_rx.SIGNATURES):
        assert not set(NEW) & set(other)
    assert sorted(k for k, v in vars(nodes).items() if isinstance(v, type)) == wrappers
    assert not hasattr(nodes, "POCSAGBank") and not hasattr(nodes, "MessageAssembler")
    import libsdr_amd
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
    assert code == NO_CTX() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in _text()
    # the limits are valid: 1 and 8192 channels, 1 and 65536 bits
    assert _create(enabled=(1,))[0] == NO_CTX() and _create(enabled=(1,) * 8192)[0] == NO_CTX()
    assert _create(max_bits=1)[0] == NO_CTX() and _create(max_bits=65536)[0] == NO_CTX()


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
    assert text in _text(), (kw, _text())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_pocsag
    L = abi_pocsag.lib()
    e, s = (C.c_int * 4)(), C.c_int(7)
    buf = C.create_string_buffer(64)
    assert L.sdrhip_pocsag_process_dev(None, None, 0, None, None, 0, None, None) == abi.E_INVALID and "NULL" in _text()
    assert L.sdrhip_pocsag_process(None, None, 0, None, None, 0, None) == abi.E_INVALID and "NULL" in _text()
    assert L.sdrhip_pocsag_set_enabled(None, 0, 1) == abi.E_INVALID and "NULL" in _text()
    assert L.sdrhip_pocsag_get_enabled(None, e, 4) == abi.E_INVALID and "NULL" in _text()
    assert L.sdrhip_pocsag_reset(None) == abi.E_INVALID and L.sdrhip_pocsag_reset_channel(None, 0) == abi.E_INVALID
    assert L.sdrhip_pocsag_channel_state(None, 0, C.byref(s), None, None, None) == abi.E_INVALID and s.value == 7
    assert L.sdrhip_pocsag_kernel_names(None, buf, 64) == abi.E_INVALID
    assert L.sdrhip_pocsag_destroy(None) == abi.OK


def test_the_kernel_exists_for_gfx950_without_scratch(tmp_path):
    so = shutil.copy(abi.SO_PATH, tmp_path / "lib.so")
    subprocess.run([LLVM + "llvm-objdump", "--offloading", str(so)], capture_output=True, text=True, check=True, cwd=tmp_path)
    seen = {}
    for o in sorted(tmp_path.glob("lib.so.*gfx950")):
        notes = subprocess.run([LLVM + "llvm-readelf", "--notes", str(o)], capture_output=True, text=True).stdout
        for name, b in re.findall(r"\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)", notes):
            m = re.search(r"\d(pocsag_[a-z0-9_]+_kernel)", name)
            if m:
                seen[m.group(1)] = int(b)
    assert seen == {"pocsag_decode_kernel": 0}, seen
