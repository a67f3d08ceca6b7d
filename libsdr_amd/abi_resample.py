"""ctypes prototypes of include/sdrhip_resample.h — the interpolating resampler bank — applied to the function objects of the
library abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h; registered in
abi.LATER_SIDE_HEADERS, the table of the headers added after abi.SIDE_HEADERS was pinned."""
import ctypes as C

from . import abi

RESAMPLE_F32, RESAMPLE_CF32, RESAMPLE_I16, RESAMPLE_CS16_CF32 = 0, 1, 2, 3


def _signatures():
    vp, sz, i, f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    ip, fp, pvp, szp, hp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int16)
    return {
        "sdrhip_resample_create": (i, [vp, i, f, fp, i, sz, pvp]),
        "sdrhip_resamplebank_create": (i, [vp, i, fp, fp, i, sz, pvp]),
        "sdrhip_resample_out_capacity": (i, [vp, sz, szp]),
        "sdrhip_resample_process_dev": (i, [vp, vp, sz, sz, vp, sz, vp]),
        "sdrhip_resample_process": (i, [vp, vp, sz, sz, vp, sz, vp]),
        "sdrhip_resample_set_channel": (i, [vp, i, f]),
        "sdrhip_resample_reset": (i, [vp]),
        "sdrhip_resample_get_state": (i, [vp, fp, fp, fp, hp, i]),
        "sdrhip_resample_plan_info": (i, [vp, sz, ip, ip]),
        "sdrhip_resample_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_resample_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_resample.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_resample.h", SIGNATURES, registry=abi.LATER_SIDE_HEADERS)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
