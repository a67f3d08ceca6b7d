"""The C++ host side of the AX.25 deframer (include/sdr/gpu/ax25_message.hh) on the CPU: tests/cpp/test_ax25_message.cc, a
stand-alone program with its own main and no HIP, built with ASan/UBSan and run directly. It parses every frame the reference
delivered in the g24 fixtures into the reference's to / from / via / payload, prints it as the reference's AX25Dump did, and holds
frames of 0, 6, 13, 14 and 20 bytes and an address field that never ends to `malformed` — each frame in a heap block of exactly
its size, so a read behind it is the sanitizer's to find."""
import json
import os
import subprocess

from cpp_build import ROOT, SAN, build

# (its own base flags: -Wextra, no -O2, and no libsdrhip.so — the program has no HIP in it)
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror=return-type", "-I" + os.path.join(ROOT, "include")]
GOLDEN = os.path.join(ROOT, "tests", "golden")


def write_frames(path):
    """manifest_ax25.json, flattened for the C++ program: one line per delivered frame. -> the number of frames"""
    man = json.load(open(os.path.join(GOLDEN, "manifest_ax25.json")))
    n = 0
    with open(path, "w") as f:
        for case in man["cases"]:
            for call in case["frames"]:
                for w in call:
                    via = "".join(" %s %d" % (c or "-", s) for c, s in w["via"])
                    f.write("%s %s %d %s %d %d%s %s %s\n" % (w["raw"], w["to"][0] or "-", w["to"][1], w["from"][0] or "-", w["from"][1], len(w["via"]), via,
                                                             w["payload"] or "-", w["text"]))
                    n += 1
    return n


def test_message_parsing_under_sanitizers(tmp_path):
    exe = build("test_ax25_message.cc", SAN, link=False, out="test_ax25_message_san", cxx=CXX)
    n = write_frames(tmp_path / "frames.txt")
    assert n == 30
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path / "frames.txt")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%d frames" % n in r.stdout, r.stdout[-500:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
