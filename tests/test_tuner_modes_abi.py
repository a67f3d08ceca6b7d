"""The tuner bank's per-channel demodulator calls (sdrhip_tunermodes_i16_create / _set_mode / _get_modes), what can be
checked without a GPU: declared in include/sdrhip.h, bound in libsdr_amd/abi.py, exported by libsdrhip.so; the kernels behind
them exist for gfx950 and keep out of scratch; create_modes without a device says so."""
import ctypes as C
import re
import subprocess

import numpy as np

from abi_checks import LLVM, code_objects, kernels, no_ctx_code
from libsdr_amd import abi, nodes

MODE_FUNCTIONS = ["sdrhip_tunermodes_i16_create", "sdrhip_tunermodes_i16_get_modes", "sdrhip_tunermodes_i16_set_mode"]


def test_mode_calls_are_declared_bound_and_exported():
    L = abi.lib()
    declared = abi.header_functions()
    fresh = C.CDLL(abi.SO_PATH)   # (looked up by name in the library's own export table, not through the binding)
    for f in MODE_FUNCTIONS:
        assert f in declared, f
        assert f in L._declared and hasattr(L, f), f
        assert C.cast(getattr(fresh, f), C.c_void_p).value, f
    for m in ("set_mode", "modes"):
        assert hasattr(nodes.TunerBankI16, m), m
    assert "modes" in nodes.TunerBankI16.__init__.__code__.co_varnames


def test_create_modes_without_a_device():
    """No device: no context can exist, and create_modes answers SDRHIP_E_NODEVICE (there is no CPU fallback) with *out NULL.
    Where a device exists, a NULL context is the invalid argument it is in every create call."""
    order, channels = 21, 3
    taps = np.ascontiguousarray(np.stack([nodes.design_iqbb_taps(0.0, 15e3, 2.4e6, order).reshape(-1, 2)] * channels), np.int32)
    lut = np.ascontiguousarray(nodes.design_freqshift_lut_i16(), np.int32)
    inc, neg = np.zeros(channels, np.uint32), np.zeros(channels, np.intc)
    modes = np.array([abi.EPI_FM, abi.EPI_AM, abi.EPI_USB], np.intc)
    h = C.c_void_p(0x1)
    code = abi.lib().sdrhip_tunermodes_i16_create(None, taps.ctypes.data_as(C.POINTER(C.c_int32)), order, lut.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   inc.ctypes.data_as(C.POINTER(C.c_uint32)), neg.ctypes.data_as(C.POINTER(C.c_int)),
                                                   modes.ctypes.data_as(C.POINTER(C.c_int)), 8, channels, 4096, C.byref(h))
    assert code == no_ctx_code()
    assert h.value is None
    if nodes.device_count() == 0:
        assert b"no CPU fallback" in abi.lib().sdrhip_last_error()


def test_mode_kernels_exist_and_keep_out_of_scratch(tmp_path):
    """One instance per kernel form and input kind (cs16, cu8) reads the demodulator per channel; none of them uses scratch,
    and the matrix form is matrix code."""
    found = {name: (o, scratch) for o, name, scratch in kernels(code_objects(tmp_path)) if "tuner_i16_modes_" in name}
    assert sum("tuner_i16_modes_valu_kernel" in n for n in found) == 2, sorted(found)
    assert sum("tuner_i16_modes_mfma_kernel" in n for n in found) == 2, sorted(found)
    assert not {n: s for n, (_, s) in found.items() if s}
    with_mfma, cur = set(), None
    for o in {o for n, (o, _) in found.items() if "mfma" in n}:
        dis = subprocess.run([LLVM + "llvm-objdump", "-d", str(o)], capture_output=True, text=True, check=True).stdout
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
            elif cur and "tuner_i16_modes_mfma_kernel" in cur and re.search(r"v_mfma_i32_\w+_i8", line):
                with_mfma.add(cur)
    assert len(with_mfma) == 2, sorted(with_mfma)
