"""C++ side of the tuner bank: sdr::gpu::TunerBank<int16_t> (include/sdr/gpu/nodes.hh) built the way tests/test_cpp_symbols.py
builds its program — the host half (truncated tunes, config() rules) under ASan/UBSan on the CPU; on the GPU one source ->
bank -> one Recorder per channel against the g4_iqbb127d8_fm fixture and against gpu::IQBaseBand + gpu::FMDemod pairs."""
import os
import subprocess

import pytest
from cpp_build import ROOT, SAN, build

GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_tuner_bank_host_half_under_sanitizers():
    """Tunes truncated as the reference's int32 members, silent return on an incomplete Config, ConfigError on a wrong type,
    and with a complete Config either a plan or a ConfigError (no device, no CPU fallback) — never a crash; clean destructors."""
    exe = build("test_tuner.cc", SAN, out="test_tuner_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "--host-only", GOLDEN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.gpu
def test_tuner_bank_in_graphs():
    """Channel 0 reproduces g4_iqbb127d8_fm; every channel equals its gpu::IQBaseBand + gpu::FMDemod pair on the same source,
    fractional tunes and a per-channel retune between buffers included; Config per source; the drop rule with a held
    buffer; addChannel after config()."""
    exe = build("test_tuner.cc")
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr
