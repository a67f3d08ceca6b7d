"""The C++ message assembly of the POCSAG decoder bank (include/sdr/gpu/pocsag_message.hh) on the CPU: tests/cpp/
test_pocsag_assemble.cc, a stand-alone program with its own main and no HIP, built with ASan/UBSan, fed the golden cases' event
streams; what it releases at every END has to be what the reference delivered there — address, function, bits, payload, both
scores and both readings."""
import os
import subprocess

import pocsag_cases
from cpp_build import ROOT, SAN, build

# (its own base flags: -Wextra, no -O2, and no libsdrhip.so — the program has no HIP in it)
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror=return-type", "-I" + os.path.join(ROOT, "include")]


def test_message_assembly_under_sanitizers(tmp_path):
    exe = build("test_pocsag_assemble.cc", SAN, link=False, out="test_pocsag_assemble_san", cxx=CXX)
    n_cases, n_msgs = pocsag_cases.write_cases(tmp_path / "cases.txt")
    assert n_cases >= 18 and n_msgs > 20
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%d cases, %d messages" % (n_cases, n_msgs) in r.stdout, r.stdout[-500:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
