"""C++ side of the AX.25 deframer: sdr::gpu::AX25, AX25Dump and AX25Bank (include/sdr/gpu/ax25.hh), built the way
tests/test_cpp_baudot.py builds its program. The host half — ConfigError on a wrong type, what a second config() does to the node,
the dump's text — needs no device; on the GPU tests/cpp/test_ax25.cc runs every fixture case through source -> gpu::AX25 ->
handleAX25Message, call by call, and all fixture rows as the channels of one bank through process() (host rows) and processDev()
(device rows)."""
import json
import os
import subprocess

import pytest

from cpp_build import ROOT, build

GOLDEN = os.path.join(ROOT, "tests", "golden")


def write_cases(path):
    """manifest_ax25.json, flattened for the C++ program: per case a line `name offset n calls`, then per call the split, the
    number of frames and every frame's raw bytes and text (hex). -> the number of cases"""
    man = json.load(open(os.path.join(GOLDEN, "manifest_ax25.json")))
    with open(path, "w") as f:
        for c in man["cases"]:
            f.write("%s %d %d %d\n" % (c["name"], c["offset"], c["n"], len(c["splits"])))
            f.write(" ".join("%d %d%s" % (n, len(fr), "".join(" %s %s" % (w["raw"], w["text"]) for w in fr)) for n, fr in zip(c["splits"], c["frames"])) + "\n")
    return len(man["cases"])


def test_ax25_config_rules_without_a_device():
    """ConfigError with the reference's message on a source that is not uint8_t, before any device is looked at; a first config()
    makes a device node, a later one resets it, a larger buffer makes a new one; AX25Dump prints the reference's line."""
    exe = build("test_ax25.cc")
    r = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_ax25_graph_and_bank_deliver_the_fixtures(tmp_path):
    exe = build("test_ax25.cc")
    n_cases = write_cases(tmp_path / "cases.txt")
    r = subprocess.run([exe, str(tmp_path / "cases.txt"), os.path.join(GOLDEN, "g24_ax25_bits.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "graph: %d cases" % n_cases in r.stdout and "process, processDev: %d channels" % n_cases in r.stdout
