"""C++ side of the interpolating resampler (include/sdr/gpu/resample.hh), built the way tests/test_cpp_psk31.py builds its
program. tests/cpp/test_resample.cc checks the constructor's frac rule on the host (no GPU needed), and on the GPU runs every
g22_inpol_* stream through a graph Source -> gpu::InpolSubSampler -> Sink buffer by buffer against the reference's outputs,
counts and mu, the config rules, and the streams of a type as the rows of gpu::InpolSubSamplerBank (a frac per row) through host
pointers and as strided device rows."""
import os
import subprocess

import pytest

import resample_restatement as R
from cpp_build import build


def test_the_constructor_refuses_a_frac_outside_its_range():
    exe = build("test_resample.cc")
    r = subprocess.run([exe, "rules"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rules: 4 fractions refused" in r.stdout


@pytest.mark.gpu
def test_resample_nodes_and_bank_follow_the_fixtures(tmp_path):
    exe = build("test_resample.cc")
    man = R.manifest()
    names = R.fixture_names()
    with open(tmp_path / "cases.txt", "w") as f:
        for name in names:
            m = man[name]
            words = [name, m["dtype"], m["frac_bits"], m["count"], m["outputs"], len(m["lens"])] + m["lens"] + m["counts"] + m["mu_bits"]
            f.write(" ".join(str(w) for w in words) + "\n")
    r = subprocess.run([exe, "nodes", str(tmp_path / "cases.txt"), R.GOLDEN, os.path.join(R.GOLDEN, man["table"])], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "nodes: %d streams" % len(names) in r.stdout
    for dtype in R.DTYPES:
        assert "bank %s: 4 rows" % dtype in r.stdout
