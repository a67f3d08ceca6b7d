"""ctypes prototypes of include/sdrhip_psk31.h — the BPSK31 bank — applied to the function objects of the library abi.lib()
loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h."""
import ctypes as C

from . import abi

PSK31_CS16, PSK31_CF32 = 0, 1


def _signatures():
    vp, sz, i, d = C.c_void_p, C.c_size_t, C.c_int, C.c_double
    ip, fp, pvp, szp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    return {
        "sdrhip_design_inpol_taps": (i, [fp]),
        "sdrhip_psk31_create": (i, [vp, i, d, d, fp, i, sz, pvp]),
        "sdrhip_psk31bank_create": (i, [vp, i, d, fp, fp, i, sz, pvp]),
        "sdrhip_psk31_out_capacity": (i, [vp, sz, szp]),
        "sdrhip_psk31_process_dev": (i, [vp, vp, sz, sz, vp, sz, vp]),
        "sdrhip_psk31_process": (i, [vp, vp, sz, sz, vp, sz, vp]),
        "sdrhip_psk31_set_channel": (i, [vp, i, d]),
        "sdrhip_psk31_reset": (i, [vp]),
        "sdrhip_psk31_get_state": (i, [vp, fp, fp, fp, fp, ip, ip, i]),
        "sdrhip_psk31_plan_info": (i, [vp, sz, ip, ip]),
        "sdrhip_psk31_kernel_names": (i, [vp, C.c_char_p, sz]),
        "sdrhip_psk31_destroy": (i, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_psk31.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_psk31.h", SIGNATURES)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
