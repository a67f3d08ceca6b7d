"""ctypes prototypes of include/sdrhip_rx.h — the receiver bank and the per-channel FMDeemph — applied to the function objects
of the library abi.lib() loaded (abi.bind_header). A module of its own, as the header is one beside sdrhip.h."""
import ctypes as C

from . import abi


def _signatures():
    vp, sz, psz, ip = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)
    pvp = C.POINTER(C.c_void_p)
    return {
        "sdrhip_deemphbank_i16_create": (C.c_int, [vp, C.c_int, ip, C.c_int, sz, pvp]),
        "sdrhip_deemphbank_i16_set_enabled": (C.c_int, [vp, C.c_int, C.c_int]),
        "sdrhip_deemphbank_i16_get_enabled": (C.c_int, [vp, ip, C.c_int]),
        "sdrhip_rxbank_create": (C.c_int, [vp, vp, vp, vp, vp, pvp]),
        "sdrhip_rxbank_sizes": (C.c_int, [vp, sz, psz, psz]),
        "sdrhip_rxbank_process_dev": (C.c_int, [vp, vp, sz, vp, sz, vp, vp, sz, psz]),
        "sdrhip_rxbank_process": (C.c_int, [vp, vp, sz, vp, sz, vp, vp, sz, psz]),
        "sdrhip_rxbank_destroy": (C.c_int, [vp]),
    }


# name -> (restype, argtypes) of every function include/sdrhip_rx.h declares
SIGNATURES = _signatures()
_binding = abi.bind_header("sdrhip_rx.h", SIGNATURES)
HEADER, header_functions, lib = _binding.HEADER, _binding.header_functions, _binding.lib
