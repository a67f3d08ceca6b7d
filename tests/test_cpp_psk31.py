"""C++ side of the PSK31 nodes (include/sdr/gpu/psk31.hh), built the way tests/test_cpp_agc.py builds its program.
tests/cpp/test_psk31.cc runs sdr::Varicode on the host against the reference's fixture (no GPU needed), and on the GPU every
g21_psk31_* stream through a graph Source -> gpu::BPSK31 -> Sink buffer by buffer against the reference's bits and counts, the
config rules, and the streams' first buffers as rows of gpu::BPSK31Bank through host pointers and as strided device rows."""
import os
import subprocess

import pytest

import psk31_restatement as R
from cpp_build import build


def test_varicode_on_the_host():
    exe = build("test_psk31.cc")
    m = R.manifest()["g21_varicode"]
    r = subprocess.run([exe, "varicode", os.path.join(R.GOLDEN, m["bits"]), str(m["count"]), os.path.join(R.GOLDEN, m["text"]), str(m["chars"])],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "varicode: %d bits, %d characters" % (m["count"], m["chars"]) in r.stdout


@pytest.mark.gpu
def test_psk31_nodes_and_bank_follow_the_fixtures(tmp_path):
    exe = build("test_psk31.cc")
    man = R.manifest()
    names = R.fixture_names()
    with open(tmp_path / "cases.txt", "w") as f:
        for name in names:
            m = man[name]
            words = [name, m["dtype"], repr(float(m["Fs"])), repr(m["dF"]), m["count"], sum(m["counts"]), len(m["lens"])] + m["lens"] + m["counts"]
            f.write(" ".join(str(w) for w in words) + "\n")
    r = subprocess.run([exe, "nodes", str(tmp_path / "cases.txt"), R.GOLDEN, os.path.join(R.GOLDEN, man["table"])], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "nodes: %d streams" % len(names) in r.stdout
    for dtype, Fs in (("cs16", 8000), ("cf32", 8000), ("cf32", 2000)):
        rows = len([n for n in names if man[n]["dtype"] == dtype and man[n]["Fs"] == Fs])
        assert "bank %s at %d Hz: %d rows" % (dtype, Fs, rows) in r.stdout
