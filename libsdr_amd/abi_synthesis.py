"""ctypes prototypes of include/sdrhip_synthesis.h — the polyphase synthesis bank — applied to the function objects of the library
abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h; registered in
abi.LATER_SIDE_HEADERS beside abi_channelizer."""
import ctypes as C

from . import abi


def _signatures():
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    ip, fp, dp, pvp, szp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    return {
        "sdrhip_synthesis_create": (i, [vp, i, i, dp, i, sz, pvp]),
        "sdrhip_synthesis_out_count": (i, [vp, sz, szp]),
        "sdrhip_synthesis_process_dev": (i, [vp, vp, sz, sz, vp, szp]),
        "sdrhip_synthesis_process": (i, [vp, vp, sz, sz, vp, szp]),
        "sdrhip_synthesis_set_channels": (i, [vp, ip, i]),
        "sdrhip_synthesis_set_taps": (i, [vp, dp]),
        "sdrhip_synthesis_reset": (i, [vp]),
        "sdrhip_synthesis_get_state": (i, [vp, C.POINTER(C.c_uint64), fp, sz]),
        "sdrhip_synthesis_plan_info": (i, [vp, ip, ip, ip, ip]),
        "sdrhip_synthesis_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_synthesis_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_synthesis.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_synthesis.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
