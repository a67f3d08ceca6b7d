"""ctypes prototypes of include/sdrhip_channelizer.h — the polyphase channelizer — applied to the function objects of the library
abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h; registered in
abi.LATER_SIDE_HEADERS beside abi_resample."""
import ctypes as C

from . import abi

CHAN_CS16, CHAN_CF32 = 0, 1


def _signatures():
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    ip, fp, dp, pvp, szp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    return {
        "sdrhip_channelizer_create": (i, [vp, i, i, i, dp, i, sz, pvp]),
        "sdrhip_channelizer_out_count": (i, [vp, sz, szp]),
        "sdrhip_channelizer_process_dev": (i, [vp, vp, sz, vp, sz, szp]),
        "sdrhip_channelizer_process": (i, [vp, vp, sz, vp, sz, szp]),
        "sdrhip_channelizer_set_channels": (i, [vp, ip, i]),
        "sdrhip_channelizer_set_taps": (i, [vp, dp]),
        "sdrhip_channelizer_reset": (i, [vp]),
        "sdrhip_channelizer_get_state": (i, [vp, C.POINTER(C.c_uint64), fp, sz]),
        "sdrhip_channelizer_plan_info": (i, [vp, ip, ip, ip, ip]),
        "sdrhip_channelizer_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_channelizer_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_channelizer.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_channelizer.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
