"""C++ side of the tuner bank with a demodulator per channel: sdr::gpu::TunerBank<int16_t> in its PerChannel form
(include/sdr/gpu/nodes.hh), built the way tests/test_cpp_tuner.py builds its program — the host half (modes recorded before
config(), mode(c), ConfigError) under ASan/UBSan on the CPU; on the GPU IQSigGen -> bank -> one Recorder per channel against
three single-demodulator banks, and setMode() between buffers."""
import os
import subprocess

import pytest
from cpp_build import SAN, build


def test_tuner_modes_host_half_under_sanitizers():
    """Modes recorded before config() and read back with mode(c); ConfigError for a mode the bank has no demodulator for, in
    both kinds of bank, with nothing changed; with a complete Config a plan or a ConfigError — never a crash."""
    exe = build("test_tuner_modes.cc", SAN, out="test_tuner_modes_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.gpu
def test_tuner_modes_in_graphs():
    """FM, AM and USB channels of one bank equal the rows of three single-demodulator banks on the same source over 4
    buffers; setMode(1, FM) after buffer 2 changes source 1 alone, which goes on from a fresh FMDemod."""
    exe = build("test_tuner_modes.cc")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr
