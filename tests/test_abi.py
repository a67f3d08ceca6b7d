"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/sdrhip.h declares,
its host-only designers match the golden vectors, and it fails loudly (no CPU fallback) when there
is no GPU.  No device compute here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abi_checks import LLVM, code_objects, kernels
from libsdr_amd import abi, nodes


def test_library_exports_every_declared_symbol():
    L = abi.lib()
    declared = abi.header_functions()
    assert len(declared) >= 60
    missing = [f for f in declared if not hasattr(L, f)]
    assert not missing, missing
    # the binding declares a prototype for every header function and nothing else
    assert sorted(L._declared) == declared
    assert L.sdrhip_version() == 100


def test_library_is_hip_code_for_gfx950():
    out = subprocess.run([LLVM + "llvm-readelf", "--notes", abi.SO_PATH], capture_output=True, text=True)
    blob = open(abi.SO_PATH, "rb").read()
    assert b"gfx950" in blob, out.stdout[:200]
    for k in (b"iqbb_i16_kernel", b"fir_cs16_exact_kernel", b"fftconv_kernel"):
        assert k in blob


def test_hot_kernels_keep_out_of_scratch(tmp_path):
    """No K1 hot kernel may spill vector registers: scratch is HBM traffic behind the kernel's back (a change that left 68
    bytes of it in the /8 USB kernels cost 11 % time and 28 % traffic before it was seen in a profile). Read from the
    code objects' own metadata; the one allowance is a cold-phase spill of three dwords in one any-D kernel."""
    objs = code_objects(tmp_path)
    assert len(objs) >= 15, objs
    hot = [(name, scratch) for _, name, scratch in kernels(objs) if "iqbb_hot" in name]
    assert len(hot) >= 400, len(hot)
    bad = [(name, scratch) for name, scratch in hot if scratch]
    assert len(bad) <= 1 and all("anyd" in n and b <= 12 for n, b in bad), bad


def test_last_kernels_entry_points():
    """The three *_last_kernels calls refuse a NULL handle or buffer without touching a device; the binding splits their answer
    at the commas outside template arguments."""
    L = abi.lib()
    b = C.create_string_buffer(16)
    for fn in (L.sdrhip_fftconv_last_kernels, L.sdrhip_fir_last_kernels, L.sdrhip_fbb_f32_last_kernels):
        assert fn(None, b, 16) == abi.E_INVALID
    assert nodes._split_kernels("") == []
    assert nodes._split_kernels("fftconv_fused_kernel<14,0,1024,0,4,2>,hist_roll_kernel,big_mul_kernel<double2>,...") == [
        "fftconv_fused_kernel<14,0,1024,0,4,2>", "hist_roll_kernel", "big_mul_kernel<double2>", "..."]


def test_strerror_and_errors_without_device():
    L = abi.lib()
    assert L.sdrhip_strerror(0) == b"ok" and b"device" in L.sdrhip_strerror(abi.E_NODEVICE)
    if nodes.device_count() == 0:
        with pytest.raises(abi.SdrHipError) as e:
            nodes.Context(0)
        assert e.value.code == abi.E_NODEVICE and "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("case", ["g3_iqbb127d8", "g8_neg_o16_d1", "g8_o21_d3", "g8_o33_d5", "g8_o16_d4_even",
                                  "g8_o255_d8", "g8_noshift_o21_d8", "g8_ofs_d300"])
def test_product_designers_iqbb(golden, case):
    m = golden.meta(case + "_taps")
    assert np.array_equal(nodes.design_iqbb_taps(m["Ff"], m["width"], m["Fs"], m["order"]).ravel(), golden.load(case + "_taps"))
    assert np.array_equal(nodes.design_freqshift_lut_i16().ravel(), golden.load(case + "_lut"))
    assert nodes.design_freqshift_inc(m["Fc"], m["Fs"]) == m["lut_inc"]
    assert nodes.design_iqbb_decim(m["Fs"], m["sub"], m["oFs"]) == m["decim"]


@pytest.mark.parametrize("N", [127, 255, 4097])
def test_product_designers_fir(golden, N):
    assert np.array_equal(nodes.design_fir_lowpass(N, 100e3, 2.4e6), golden.load("g2_firlp_alpha%d" % N))


@pytest.mark.parametrize("N", [1024, 8192])
def test_product_designers_fftfilt(golden, orc, N):
    h = nodes.design_fftfilt_kernel(N, 50e3, 150e3, 2.4e6)
    assert np.array_equal(h, golden.load("g7_fftfilt_h%d" % N))
    K = nodes.design_fftfilt_spectrum(h)
    Ko = orc.fftfilt_design_K(h)
    assert np.abs(K - Ko).max() <= 1e-6 * np.abs(Ko).max()


def test_product_designers_fftfilt_any_block_size_and_double(golden, orc):
    """g15: the product's sinc_flt_kernel<float> at N = 1000 and sinc_flt_kernel<double> (bit-exact to the reference's),
    and the spectra behind them (any DFT length) against the oracle's."""
    h = nodes.design_fftfilt_kernel(1000, -350e3, -250e3, 2.4e6)
    assert np.array_equal(h, golden.load("g15_fftfilt_h1000"))
    K, Ko = nodes.design_fftfilt_spectrum(h), orc.fftfilt_design_K(h)
    assert K.shape == (2000, 2) and np.abs(K - Ko).max() <= 1e-6 * np.abs(Ko).max()
    for N in (1000, 1024):
        hd = nodes.design_fftfilt_kernel(N, -350e3, -250e3, 2.4e6, dtype=np.float64)
        assert hd.dtype == np.float64 and np.array_equal(hd.ravel(), golden.load("g15_fftfilt_h%d_f64" % N))
        K, Ko = nodes.design_fftfilt_spectrum(hd), orc.fftfilt_design_K_f64(hd)
        assert K.dtype == np.float64 and np.abs(K - Ko).max() <= 1e-13 * np.abs(Ko).max()


@pytest.mark.parametrize("case", ["g10_bb21d8", "g10_bb127d8_neg_ragged", "g10_bb64d5", "g10_bb16d1_noshift", "g10_bb1d3",
                                  "g10_bb127d8_loud"])
def test_product_designers_real_baseband(golden, case):
    """BaseBand<int16_t> (real input): Q16 taps of the product designer vs the reference node's kernel."""
    m = golden.meta(case + "_taps")
    assert np.array_equal(nodes.design_bb_taps(m["Ff"], m["width"], m["Fs"], m["order"]).ravel(), golden.load(case + "_taps"))
    assert nodes.design_freqshift_inc(m["Fc"], m["Fs"]) == m["lut_inc"]


def test_product_designer_fmdeemph():
    for rate, alpha in ((125e3, 10), (48e3, 4), (22050.0, 2)):
        got = nodes.design_fmdeemph_alpha(rate) if hasattr(nodes, "design_fmdeemph_alpha") else None
        if got is not None:
            assert got == int(round(1.0 / (1.0 - np.exp(-1.0 / (rate * 75e-6)))))


def test_no_oracle_in_product_path():
    """The product (libsdr_amd/, include/) must never reach into oracle/."""
    root = abi.ROOT
    for base in ("libsdr_amd", "include"):
        for dp, _, fs in os.walk(os.path.join(root, base)):
            for f in fs:
                if f.endswith((".py", ".hip", ".hpp", ".hh", ".h", ".cc", "Makefile")):
                    txt = open(os.path.join(dp, f), errors="ignore").read()
                    assert "pyoracle" not in txt and "liboracle" not in txt and "sdr_oracle" not in txt, f
    needed = subprocess.run(["ldd", abi.SO_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in needed


@pytest.mark.gpu
def test_roctx_ranges_around_process_calls():
    """SDRHIP_ROCTX=1 brackets every *_process call with roctxRangePush / Pop (SURVEY §5 tracing): the smoke chain must run
    unchanged with the ranges on (libroctx is opened with dlopen; without a profiler attached the calls are no-ops)."""
    import subprocess, sys
    env = dict(os.environ, SDRHIP_ROCTX="1")
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=abi.ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "smoke ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
