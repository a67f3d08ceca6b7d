"""C++ side of the real-input tuner bank: sdr::gpu::RealTunerBank<int16_t> (include/sdr/gpu/nodes.hh), built the way
tests/test_cpp_tuner_modes.py builds its program — the host half (construction, the tunes kept as doubles, config() rules, type
checks, the no-device path) under ASan/UBSan on the CPU; on the GPU a source of real int16 buffers -> bank with a demodulator
per channel -> one Recorder per channel, against rows the CPU oracle's BaseBand<int16_t> (+ FMDemod / AMDemod / USBDemod) made
of the same buffers and this module wrote to files for it."""
import os
import subprocess

import numpy as np
import pytest
from cpp_build import SAN, build


# as tests/cpp/test_tuner_real.cc states them
FS, BS, ORDER, D = 2.0e6, 4096, 127, 20
TUNES = [(101.5e3, 101.5e3, 12.5e3, "fm"), (455000.25, 455000.25, 9e3, "am"), (14.07e3, 15.57e3, 3e3, "usb")]
CUTS = [BS, BS, BS, 1000]


def test_real_tuner_bank_host_half_under_sanitizers():
    """A Sink<int16_t>; tunes kept as doubles; silent return on an incomplete Config, ConfigError on a complex or byte input
    type and on a mode the bank has no demodulator for; with a complete Config either a plan or a ConfigError (no device, no CPU
    fallback) — never a crash; clean destructors."""
    exe = build("test_tuner_real.cc", SAN, out="test_tuner_real_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.gpu
def test_real_tuner_bank_in_a_graph(tmp_path, orc):
    """FM, AM and USB channels of one real-input bank over three whole buffers and a short one equal, bit for bit and buffer by
    buffer, the oracle's node of each channel; Config per source."""
    import libsdr_amd as sa
    n = sum(CUTS)
    t = np.arange(n, dtype=np.float64)
    x = sum(a * np.cos(2 * np.pi * f / FS * t + p) for f, a, p in ((101.5e3, 7000, 0.3), (455e3, 6000, 1.0), (15.1e3, 5000, 0.0), (803e3, 4000, 2.0)))
    x = np.clip(np.rint(x) + np.random.default_rng(20261018).integers(-2000, 2000, n), -32768, 32767).astype(np.int16)
    x.tofile(tmp_path / "input.i16")
    lut = sa.design_freqshift_lut_i16()
    for c, (Fc, Ff, width, mode) in enumerate(TUNES):
        bb = orc.BaseBandI16(sa.design_bb_taps(Ff, width, FS, ORDER), lut, sa.design_freqshift_inc(Fc, FS), Fc < 0, D)
        fm, rows, off = orc.FMDemodI16(), [], 0
        for m in CUTS:
            y = bb.process(x[off:off + m]); off += m
            rows.append(fm.process(y) if mode == "fm" else orc.am_i16(y) if mode == "am" else orc.usb_i16(y))
        assert [len(r) for r in rows] == [204, 205, 205, 50]
        np.concatenate(rows).astype(np.int16).tofile(tmp_path / ("row%d.i16" % c))
    exe = build("test_tuner_real.cc")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr
