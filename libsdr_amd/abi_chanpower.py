"""ctypes prototypes of include/sdrhip_chanpower.h — the channel power monitor — applied to the function objects of the library
abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h; registered in
abi.LATER_SIDE_HEADERS beside abi_chanaudio."""
import ctypes as C

from . import abi

from .abi_channelizer import CHAN_CS16, CHAN_CF32  # noqa: F401   (the header takes sdrhip_channelizer.h's dtype codes)


def _signatures():
    vp, sz, i, d = C.c_void_p, C.c_size_t, C.c_int, C.c_double
    ip, fp, dp, pvp, szp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_ubyte)
    return {
        "sdrhip_chanpower_create": (i, [vp, i, i, i, dp, i, sz, d, pvp]),
        "sdrhip_chanpower_out_count": (i, [vp, sz, szp]),
        "sdrhip_chanpower_process_dev": (i, [vp, vp, sz, vp, szp]),
        "sdrhip_chanpower_process": (i, [vp, vp, sz, dp, szp]),
        "sdrhip_chanpower_set_thresholds": (i, [vp, dp, dp]),
        "sdrhip_chanpower_set_alpha": (i, [vp, d]),
        "sdrhip_chanpower_set_taps": (i, [vp, dp]),
        "sdrhip_chanpower_reset": (i, [vp]),
        "sdrhip_chanpower_get_levels": (i, [vp, dp, u8p, i]),
        "sdrhip_chanpower_get_occupied": (i, [vp, ip, i, ip]),
        "sdrhip_chanpower_get_state": (i, [vp, u64p, fp, sz, u64p]),
        "sdrhip_chanpower_plan_info": (i, [vp, ip, ip, ip, ip, ip]),
        "sdrhip_chanpower_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_chanpower_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_chanpower.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_chanpower.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
