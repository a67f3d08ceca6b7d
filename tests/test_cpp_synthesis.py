"""C++ side of the synthesis bank (include/sdr/gpu/synthesis.hh), built the way tests/test_cpp_channelizer.py builds its
program. tests/cpp/test_synthesis.cc checks the constructor's rules on the host (no GPU needed), and on the GPU runs host rows
through gpu::Synthesis::process round by round into a Sink, against the values this side wrote from the numpy restatement
(<= 1e-5 of the largest), then the same rows as strided device rows through processDev."""
import subprocess

import numpy as np
import pytest

import synthesis_restatement as R
from cpp_build import build


def test_the_constructor_refuses_what_create_refuses():
    exe = build("test_synthesis.cc")
    r = subprocess.run([exe, "rules"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rules: 14 constructions refused" in r.stdout


@pytest.mark.gpu
def test_synthesis_rounds_follow_the_restatement(tmp_path):
    exe = build("test_synthesis.cc")
    M, D, n_taps = 12, 5, 30
    sel = [11, 0, 5, 6]
    lens = [40, 1, 5, 0, 7, 37]
    n = sum(lens)
    rng = np.random.default_rng(12)
    x = (0.5 * rng.standard_normal((len(sel), n, 2))).astype(np.float32)
    t = np.arange(n_taps) - (n_taps - 1) / 2
    taps = np.sinc(t / M) * np.hanning(n_taps + 2)[1:-1] * D / M
    want = R.folded(R.rows_of(x), R.round32(taps), M, D, sel)
    with open(tmp_path / "case.txt", "w") as f:
        f.write(" ".join(str(v) for v in [M, D, n_taps, n, len(sel)] + sel + [len(lens)] + lens) + "\n")
    taps.astype(np.float64).tofile(tmp_path / "taps.bin")
    x.tofile(tmp_path / "x.bin")
    R.as_pairs(want).astype(np.float64).tofile(tmp_path / "want.bin")
    r = subprocess.run([exe, "run"] + [str(tmp_path / v) for v in ("case.txt", "taps.bin", "x.bin", "want.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "run: %d rows x %d columns" % (len(sel), n) in r.stdout and "processDev: %d rows" % len(sel) in r.stdout
