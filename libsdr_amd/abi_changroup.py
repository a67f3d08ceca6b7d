"""ctypes prototypes of include/sdrhip_changroup.h — the channel group: several handles of the channelizer family in one launch —
applied to the function objects of the library abi.lib() loaded (abi.bind_header). A module of its own, as the header is one
beside sdrhip.h; registered in abi.LATER_SIDE_HEADERS beside abi_channelizer."""
import ctypes as C

from . import abi

CHANGROUP_MAX = 8


def _signatures():
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    ip, pvp, szp = C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    create = (i, [pvp, i, pvp])
    return {
        "sdrhip_changroup_channelizer_create": create,
        "sdrhip_changroup_audio_create": create,
        "sdrhip_changroup_power_create": create,
        "sdrhip_changroup_process_dev": (i, [vp, pvp, szp, pvp, szp, szp]),
        "sdrhip_changroup_power_process_dev": (i, [vp, pvp, szp, pvp, szp]),
        "sdrhip_changroup_plan_info": (i, [vp, ip, ip, ip]),
        "sdrhip_changroup_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_changroup_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_changroup.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_changroup.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
