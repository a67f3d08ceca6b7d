"""ctypes prototypes of include/sdrhip_ax25.h — the AX.25 deframer bank — applied to the function objects of the library
abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h; registered in
abi.LATER_SIDE_HEADERS, the table of the headers added after abi.SIDE_HEADERS was pinned."""
import ctypes as C

from . import abi

RXBUFFER = 512   # SDRHIP_AX25_RXBUFFER


def _signatures():
    vp, sz, i, ip = C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int)
    pvp, u32, pu32, pu8 = C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    return {
        "sdrhip_ax25_create": (i, [vp, ip, i, sz, pvp]),
        "sdrhip_ax25_frames_capacity": (sz, [sz]),
        "sdrhip_ax25_bytes_capacity": (sz, [sz]),
        "sdrhip_ax25_process_dev": (i, [vp, vp, sz, vp, vp, sz, vp, sz, vp, vp]),
        "sdrhip_ax25_process": (i, [vp, vp, sz, vp, vp, sz, vp, sz, vp]),
        "sdrhip_ax25_set_enabled": (i, [vp, i, i]),
        "sdrhip_ax25_get_enabled": (i, [vp, ip, i]),
        "sdrhip_ax25_reset": (i, [vp]),
        "sdrhip_ax25_reset_channel": (i, [vp, i]),
        "sdrhip_ax25_channel_state": (i, [vp, i, pu32, pu32, ip, ip, pu8]),
        "sdrhip_ax25_set_channel_state": (i, [vp, i, u32, u32, i, i, pu8]),
        "sdrhip_ax25_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_ax25_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_ax25.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_ax25.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
