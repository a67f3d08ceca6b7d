"""C++ side of the channelizer (include/sdr/gpu/channelizer.hh), built the way tests/test_cpp_resample.py builds its program.
tests/cpp/test_channelizer.cc checks the constructor's rules on the host (no GPU needed), and on the GPU runs a cs16 stream
through a graph Source -> gpu::Channelizer<int16_t> -> one Sink per selected row, buffer by buffer, against the values this side
wrote from the numpy restatement (<= 1e-5 of the largest), then the same stream as device rows through processDev."""
import subprocess

import numpy as np
import pytest

import channelizer_restatement as R
from cpp_build import build


def test_the_constructor_refuses_what_create_refuses():
    exe = build("test_channelizer.cc")
    r = subprocess.run([exe, "rules"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rules: 13 constructions refused" in r.stdout


@pytest.mark.gpu
def test_channelizer_in_a_graph_follows_the_restatement(tmp_path):
    exe = build("test_channelizer.cc")
    M, D, n_taps = 12, 6, 30
    sel = [11, 0, 5, 6]
    lens = [600, 1, 5, 7, 0, 595, 298]
    n = sum(lens)
    assert n % D == 0
    rng = np.random.default_rng(12)
    x = rng.integers(-20000, 20000, (n, 2)).astype(np.int16)
    x[5], x[6] = (32767, -32768), (-32768, 32767)
    t = np.arange(n_taps) - (n_taps - 1) / 2
    taps = np.sinc(t / M) / M * np.hanning(n_taps + 2)[1:-1]
    want = R.folded(R.pairs(x), R.round32(taps), M, D)[sel]
    with open(tmp_path / "case.txt", "w") as f:
        f.write(" ".join(str(v) for v in [M, D, n_taps, n, len(sel)] + sel + [len(lens)] + lens) + "\n")
    taps.astype(np.float64).tofile(tmp_path / "taps.bin")
    x.tofile(tmp_path / "x.bin")
    R.as_rows(want).astype(np.float64).tofile(tmp_path / "want.bin")
    r = subprocess.run([exe, "graph"] + [str(tmp_path / v) for v in ("case.txt", "taps.bin", "x.bin", "want.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "graph: %d rows x %d outputs" % (len(sel), n // D) in r.stdout and "processDev: %d rows" % len(sel) in r.stdout
