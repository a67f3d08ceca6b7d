"""ctypes prototypes of include/sdrhip_psk31.h — the BPSK31 bank — applied to the function objects of the library abi.lib()
loaded. A module of its own beside abi.py, abi_rx.py, abi_pocsag.py and abi_agc.py, as the header is one beside sdrhip.h: their
SIGNATURES and the library's `_declared` list stay what they were."""
import ctypes as C
import os
import re

from . import abi

HEADER = os.path.join(abi.ROOT, "include", "sdrhip_psk31.h")

PSK31_CS16, PSK31_CF32 = 0, 1


def header_functions():
    """Names of every function include/sdrhip_psk31.h declares."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sdrhip_[a-z0-9_]+)\s*\(", src)))


def _signatures():
    vp, sz, i, d = C.c_void_p, C.c_size_t, C.c_int, C.c_double
    ip, fp, pvp, szp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    return {
        "sdrhip_design_inpol_taps": (i, [fp]),
        "sdrhip_psk31_create": (i, [vp, i, d, d, fp, i, sz, pvp]),
        "sdrhip_psk31bank_create": (i, [vp, i, d, fp, fp, i, sz, pvp]),
        "sdrhip_psk31_out_capacity": (i, [vp, sz, szp]),
        "sdrhip_psk31_process_dev": (i, [vp, vp, sz, sz, vp, sz, vp]),
        "sdrhip_psk31_process": (i, [vp, vp, sz, sz, vp, sz, vp]),
        "sdrhip_psk31_set_channel": (i, [vp, i, d]),
        "sdrhip_psk31_reset": (i, [vp]),
        "sdrhip_psk31_get_state": (i, [vp, fp, fp, fp, fp, ip, ip, i]),
        "sdrhip_psk31_plan_info": (i, [vp, sz, ip, ip]),
        "sdrhip_psk31_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_psk31_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_psk31.h declares
SIGNATURES = _signatures()

_applied = None


def lib():
    """abi.lib() with this header's prototypes on its function objects."""
    global _applied
    L = abi.lib()
    if _applied is not L:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _applied = L
    return L
