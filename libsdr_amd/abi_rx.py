"""ctypes prototypes of include/sdrhip_rx.h — the receiver bank and the per-channel FMDeemph — applied to the function objects
of the library abi.lib() loaded. A module of its own beside abi.py, as the header is one beside sdrhip.h: abi.SIGNATURES and
the library's `_declared` list stay the binding of sdrhip.h alone."""
import ctypes as C
import os
import re

from . import abi

HEADER = os.path.join(abi.ROOT, "include", "sdrhip_rx.h")


def header_functions():
    """Names of every function include/sdrhip_rx.h declares."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sdrhip_[a-z0-9_]+)\s*\(", src)))


def _signatures():
    vp, sz, psz, ip = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)
    pvp = C.POINTER(C.c_void_p)
    return {
        "sdrhip_deemphbank_i16_create": (C.c_int, [vp, C.c_int, ip, C.c_int, sz, pvp]),
        "sdrhip_deemphbank_i16_set_enabled": (C.c_int, [vp, C.c_int, C.c_int]),
        "sdrhip_deemphbank_i16_get_enabled": (C.c_int, [vp, ip, C.c_int]),
        "sdrhip_rxbank_create": (C.c_int, [vp, vp, vp, vp, vp, pvp]),
        "sdrhip_rxbank_sizes": (C.c_int, [vp, sz, psz, psz]),
        "sdrhip_rxbank_process_dev": (C.c_int, [vp, vp, sz, vp, sz, vp, vp, sz, psz]),
        "sdrhip_rxbank_process": (C.c_int, [vp, vp, sz, vp, sz, vp, vp, sz, psz]),
        "sdrhip_rxbank_destroy": (C.c_int, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_rx.h declares
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
