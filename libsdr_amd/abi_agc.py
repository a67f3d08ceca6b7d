"""ctypes prototypes of include/sdrhip_agc.h — the AGC bank — applied to the function objects of the library abi.lib() loaded
(abi.bind_header). A module of its own, as the header is one beside sdrhip.h."""
import ctypes as C

from . import abi

AGC_I16, AGC_F32 = 0, 1


def _signatures():
    vp, sz, i, f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    ip, fp, pvp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_void_p)
    return {
        "sdrhip_design_agc_lambda": (i, [C.c_double, C.c_double, fp]),
        "sdrhip_design_agc_target": (i, [i, fp]),
        "sdrhip_agc_create": (i, [vp, i, f, f, i, sz, pvp]),
        "sdrhip_agcbank_create": (i, [vp, i, fp, fp, ip, i, sz, pvp]),
        "sdrhip_agc_process_dev": (i, [vp, vp, sz, sz, vp, sz]),
        "sdrhip_agc_process": (i, [vp, vp, sz, sz, vp, sz]),
        "sdrhip_agc_set_channel": (i, [vp, i, f, f]),
        "sdrhip_agc_set_lambda": (i, [vp, i, f]),
        "sdrhip_agc_set_enabled": (i, [vp, i, i]),
        "sdrhip_agc_set_gain": (i, [vp, i, f]),
        "sdrhip_agc_get_state": (i, [vp, fp, fp, ip, i]),
        "sdrhip_agc_plan_info": (i, [vp, sz, ip, ip]),
        "sdrhip_agc_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_agc_reset": (i, [vp]),
        "sdrhip_agc_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_agc.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_agc.h", SIGNATURES)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
