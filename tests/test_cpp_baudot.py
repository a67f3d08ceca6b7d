"""C++ side of the Baudot decoder: sdr::gpu::Baudot and sdr::gpu::BaudotBank (include/sdr/gpu/baudot.hh), built the way
tests/test_cpp_pocsag.py builds its program. The host half — ConfigError on a wrong type, and what a second config() does to
the node — needs no device and runs under ASan/UBSan on the CPU; on the GPU tests/cpp/test_baudot.cc runs every fixture case
through source -> gpu::Baudot -> sink, call by call, and all fixture rows as the channels of one bank through process() (host
rows) and processDev() (device rows)."""
import json
import os
import subprocess

import pytest

from cpp_build import ROOT, SAN, build

GOLDEN = os.path.join(ROOT, "tests", "golden")


def write_cases(path):
    """manifest_baudot.json, flattened for the C++ program: per case a line `name stop offset n calls`, then per call the split
    and what the call sent (hex, - for no send). -> the number of cases"""
    man = json.load(open(os.path.join(GOLDEN, "manifest_baudot.json")))
    with open(path, "w") as f:
        for c in man["cases"]:
            f.write("%s %d %d %d %d\n" % (c["name"], c["stop"], c["offset"], c["n"], len(c["splits"])))
            f.write(" ".join("%d %s" % (n, s if s is not None else "-") for n, s in zip(c["splits"], c["sends"])) + "\n")
    return len(man["cases"])


def test_baudot_config_rules_under_sanitizers():
    """ConfigError with the reference's message on a wrong type, before any device is looked at; a first config() makes a
    fresh node, a second one resets it with keep_mode, a larger buffer makes a new node in the old one's table; the Config
    forwarded declares bufferSize / 14 + 1 characters."""
    exe = build("test_baudot.cc", SAN, out="test_baudot_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.gpu
def test_baudot_graph_and_bank_deliver_the_fixtures(tmp_path):
    exe = build("test_baudot.cc")
    n_cases = write_cases(tmp_path / "cases.txt")
    r = subprocess.run([exe, str(tmp_path / "cases.txt"), os.path.join(GOLDEN, "g23_baudot_bits.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "graph: %d cases" % n_cases in r.stdout and "process, processDev: %d channels" % n_cases in r.stdout
