"""ctypes prototypes of include/sdrhip_chanaudio.h — the audio channelizer — applied to the function objects of the library
abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h; registered in
abi.LATER_SIDE_HEADERS beside abi_channelizer."""
import ctypes as C

from . import abi

from .abi_channelizer import CHAN_CS16, CHAN_CF32  # noqa: F401   (the header takes sdrhip_channelizer.h's dtype codes)


def _signatures():
    vp, sz, i, f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    ip, fp, dp, pvp, szp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    return {
        "sdrhip_chanaudio_create": (i, [vp, i, i, i, dp, i, sz, ip, fp, pvp]),
        "sdrhip_chanaudio_out_count": (i, [vp, sz, szp]),
        "sdrhip_chanaudio_process_dev": (i, [vp, vp, sz, vp, sz, szp]),
        "sdrhip_chanaudio_process": (i, [vp, vp, sz, vp, sz, szp]),
        "sdrhip_chanaudio_set_channels": (i, [vp, ip, i]),
        "sdrhip_chanaudio_set_mode": (i, [vp, i, i]),
        "sdrhip_chanaudio_get_modes": (i, [vp, ip, i]),
        "sdrhip_chanaudio_set_gain": (i, [vp, i, f]),
        "sdrhip_chanaudio_get_gains": (i, [vp, fp, i]),
        "sdrhip_chanaudio_set_taps": (i, [vp, dp]),
        "sdrhip_chanaudio_reset": (i, [vp]),
        "sdrhip_chanaudio_get_state": (i, [vp, C.POINTER(C.c_uint64), fp, sz, ip, sz]),
        "sdrhip_chanaudio_plan_info": (i, [vp, ip, ip, ip, ip, ip, ip]),
        "sdrhip_chanaudio_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_chanaudio_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_chanaudio.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_chanaudio.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
