"""ctypes prototypes of include/sdrhip_pocsag.h — the POCSAG decoder bank — applied to the function objects of the library
abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h."""
import ctypes as C

from . import abi

# event kinds (info[1:0]) and node states (sdrhip_pocsag_channel_state)
SYNC, WORD, END = 0, 1, 2
WAIT, RECEIVE, CHECK_CONTINUE = 0, 1, 2


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
_binding = abi.bind_header("sdrhip_pocsag.h", SIGNATURES)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
