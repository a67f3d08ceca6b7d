"""ctypes prototypes of include/sdrhip_chanreal.h — the channelizer family's create calls for a real-sampled antenna row —
applied to the function objects of the library abi.lib() loaded (abi.bind_header). The handles they return are served by the
calls of sdrhip_channelizer.h, sdrhip_chanaudio.h and sdrhip_chanpower.h, which their own modules bind. Registered in
abi.LATER_SIDE_HEADERS beside abi_chanpower."""
import ctypes as C

from . import abi

CHANREAL_S16, CHANREAL_F32 = 0, 1


def _signatures():
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    ip, fp, dp, pvp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_void_p)
    return {
        "sdrhip_chanreal_channelizer_create": (i, [vp, i, i, i, dp, i, sz, pvp]),
        "sdrhip_chanreal_audio_create": (i, [vp, i, i, i, dp, i, sz, ip, fp, pvp]),
        "sdrhip_chanreal_power_create": (i, [vp, i, i, i, dp, i, sz, C.c_double, pvp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_chanreal.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_chanreal.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
