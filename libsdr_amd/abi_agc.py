"""ctypes prototypes of include/sdrhip_agc.h — the AGC bank — applied to the function objects of the library abi.lib() loaded.
A module of its own beside abi.py, abi_rx.py and abi_pocsag.py, as the header is one beside sdrhip.h: their SIGNATURES and the
library's `_declared` list stay what they were."""
import ctypes as C
import os
import re

from . import abi

HEADER = os.path.join(abi.ROOT, "include", "sdrhip_agc.h")

AGC_I16, AGC_F32 = 0, 1


def header_functions():
    """Names of every function include/sdrhip_agc.h declares."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sdrhip_[a-z0-9_]+)\s*\(", src)))


def _signatures():
    vp, sz, i, f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    ip, fp, pvp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_void_p)
    return {
        "sdrhip_design_agc_lambda": (i, [C.c_double, C.c_double, fp]),
        "sdrhip_design_agc_target": (i, [i, fp]),
        "sdrhip_agc_create": (i, [vp, i, f, f, i, sz, pvp]),
        "sdrhip_agcbank_create": (i, [vp, i, fp, fp, ip, i, sz, pvp]),
        "sdrhip_agc_process_dev": (i, [vp, vp, sz, sz, vp, sz]),
        "sdrhip_agc_process": (i, [vp, vp, sz, sz, vp, sz]),
        "sdrhip_agc_set_channel": (i, [vp, i, f, f]),
        "sdrhip_agc_set_lambda": (i, [vp, i, f]),
        "sdrhip_agc_set_enabled": (i, [vp, i, i]),
        "sdrhip_agc_set_gain": (i, [vp, i, f]),
        "sdrhip_agc_get_state": (i, [vp, fp, fp, ip, i]),
        "sdrhip_agc_plan_info": (i, [vp, sz, ip, ip]),
        "sdrhip_agc_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_agc_reset": (i, [vp]),
        "sdrhip_agc_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_agc.h declares
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
