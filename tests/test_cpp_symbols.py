"""C++ side of the symbol path: sdr::gpu::FSKDetector, ASKDetector<int16_t> and BitStream (include/sdr/gpu/nodes.hh) built the
way tests/test_cpp.py builds its programs — the host half (designer against the g18 LUTs, config() rules) under
ASan/UBSan on the CPU, sdr_ax25's graph detector -> bits -> Recorder on the GPU."""
import os
import subprocess

import pytest
from cpp_build import ROOT, SAN, build

GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_symbol_nodes_host_half_under_sanitizers():
    """Designer LUTs bit for bit, silent return on an incomplete Config, ConfigError on a wrong type, and with a complete
    Config either a plan or a ConfigError (no device, no CPU fallback) — never a crash; clean destructors."""
    exe = build("test_symbols.cc", SAN, out="test_symbols_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "--host-only", GOLDEN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.gpu
def test_symbol_nodes_in_graphs():
    """sdr_ax25's graph reproduces the g18 AX.25 bits in both modes, with the symbols handed over on the device and through
    the host buffer; BitStream sends nothing for a bit-less buffer; ASK both ways; a Config change restarts both nodes."""
    exe = build("test_symbols.cc")
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr
