"""ctypes prototypes of include/sdrhip_baudot.h — the Baudot decoder bank — applied to the function objects of the library
abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h; registered in
abi.LATER_SIDE_HEADERS, the table of the headers added after abi.SIDE_HEADERS was pinned."""
import ctypes as C

from . import abi

# stop-bit settings and the node's tables (sdrhip_baudot_channel_state)
STOP1, STOP15, STOP2 = 0, 1, 2
LETTERS, FIGURES = 0, 1


def _signatures():
    vp, sz, i, ip = C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int)
    pvp = C.POINTER(C.c_void_p)
    return {
        "sdrhip_baudot_create": (i, [vp, i, i, sz, pvp]),
        "sdrhip_baudotbank_create": (i, [vp, ip, ip, i, sz, pvp]),
        "sdrhip_baudot_out_capacity": (sz, [sz]),
        "sdrhip_baudot_process_dev": (i, [vp, vp, sz, vp, vp, sz, vp, vp]),
        "sdrhip_baudot_process": (i, [vp, vp, sz, vp, vp, sz, vp]),
        "sdrhip_baudot_set_channel": (i, [vp, i, i]),
        "sdrhip_baudot_set_enabled": (i, [vp, i, i]),
        "sdrhip_baudot_get_channels": (i, [vp, ip, ip, i]),
        "sdrhip_baudot_reset": (i, [vp, i]),
        "sdrhip_baudot_reset_channel": (i, [vp, i, i]),
        "sdrhip_baudot_channel_state": (i, [vp, i, C.POINTER(C.c_uint16), C.POINTER(C.c_uint64), ip]),
        "sdrhip_baudot_set_channel_state": (i, [vp, i, C.c_uint16, C.c_uint64, i]),
        "sdrhip_baudot_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_baudot_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_baudot.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_baudot.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
