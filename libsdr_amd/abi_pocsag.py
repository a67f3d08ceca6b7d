"""ctypes prototypes of include/sdrhip_pocsag.h — the POCSAG decoder bank — applied to the function objects of the library
abi.lib() loaded. A module of its own beside abi.py and abi_rx.py, as the header is one beside sdrhip.h: abi.SIGNATURES,
abi_rx.SIGNATURES and the library's `_declared` list stay what they were."""
import ctypes as C
import os
import re

from . import abi

HEADER = os.path.join(abi.ROOT, "include", "sdrhip_pocsag.h")

# event kinds (info[1:0]) and node states (sdrhip_pocsag_channel_state)
SYNC, WORD, END = 0, 1, 2
WAIT, RECEIVE, CHECK_CONTINUE = 0, 1, 2


def header_functions():
    """Names of every function include/sdrhip_pocsag.h declares."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sdrhip_[a-z0-9_]+)\s*\(", src)))


def _signatures():
    vp, sz, ip = C.c_void_p, C.c_size_t, C.POINTER(C.c_int)
    pvp = C.POINTER(C.c_void_p)
    return {
        "sdrhip_pocsag_create": (C.c_int, [vp, ip, C.c_int, sz, pvp]),
        "sdrhip_pocsag_out_capacity": (sz, [sz]),
        "sdrhip_pocsag_process_dev": (C.c_int, [vp, vp, sz, vp, vp, sz, vp, vp]),
        "sdrhip_pocsag_process": (C.c_int, [vp, vp, sz, vp, vp, sz, vp]),
        "sdrhip_pocsag_set_enabled": (C.c_int, [vp, C.c_int, C.c_int]),
        "sdrhip_pocsag_get_enabled": (C.c_int, [vp, ip, C.c_int]),
        "sdrhip_pocsag_reset": (C.c_int, [vp]),
        "sdrhip_pocsag_reset_channel": (C.c_int, [vp, C.c_int]),
        "sdrhip_pocsag_channel_state": (C.c_int, [vp, C.c_int, ip, ip, ip, C.POINTER(C.c_uint64)]),
        "sdrhip_pocsag_kernel_names": (C.c_int, [vp, C.c_char_p, sz]),
        "sdrhip_pocsag_destroy": (C.c_int, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_pocsag.h declares
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
