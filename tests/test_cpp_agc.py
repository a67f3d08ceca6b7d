"""C++ side of the AGC on the GPU: sdr::gpu::AGC<int16_t>, gpu::AGC<float> and gpu::AGCBank (include/sdr/gpu/agc.hh), built the
way tests/test_cpp_pocsag.py builds its program. tests/cpp/test_agc.cc runs every g20_agc_* stream through a graph
Source -> gpu::AGC -> Sink buffer by buffer, the recorded enable() / setGain() calls included, against the reference's output,
gain and level bits, and the streams' heads as device rows through AGCBank::processDev. setTau, which no fixture holds, runs
between two buffers against the restatement with its decay changed (the reference's setTau touches nothing else)."""
import subprocess

import numpy as np
import pytest

import agc_restatement as R
from cpp_build import build


def write_cases(path):
    man = R.manifest()
    with open(path, "w") as f:
        for name in sorted(man):
            m = man[name]
            words = [name, m["dtype"], repr(m["Fs"]), repr(m["tau"]), repr(m["target"]), m["count"], len(m["lens"])] + m["lens"] + [len(m["ops"])]
            for op in m["ops"]:
                words += [op["at"], 0 if op["what"] == "enable" else 1, op["value_bits"]]
            for g, s, _ in m["state_bits"]:
                words += [g, s]
            f.write(" ".join(str(w) for w in words) + "\n")
    return len(man)


def write_tau_cases(path, tmp):
    """setTau(tau2) between buffers of n1 and n2 samples of the two `target` streams; expected by the restatement."""
    man, tau2, n1, n2 = R.manifest(), 0.0005, 700, 1300
    with open(path, "w") as f:
        for t in ("i16", "f32"):
            name = "g20_agc_%s_target" % t
            m, x, _ = R.load(name, man)
            node = R.Bank(x.dtype, R.design_lambda(m["tau"], m["Fs"]), m["target"])
            y1 = node.process(x[:n1])[0]
            g1, s1 = int(node.gain.view(np.uint32)[0]), int(node.sd.view(np.uint32)[0])
            node.lam[0] = R.design_lambda(tau2, m["Fs"])
            y2 = node.process(x[n1:n1 + n2])[0]
            y = np.concatenate([y1, y2])
            assert not np.isnan(y.astype(np.float64)).any() and not np.array_equal(y[n1:], R.load(name, man)[2][n1:n1 + n2])
            expected = str(tmp / (name + "_tau.bin"))
            y.tofile(expected)
            words = [name, t, repr(m["Fs"]), repr(m["tau"]), repr(m["target"]), repr(tau2), n1, n2, g1, s1,
                     int(node.gain.view(np.uint32)[0]), int(node.sd.view(np.uint32)[0]), expected]
            f.write(" ".join(str(w) for w in words) + "\n")


@pytest.mark.gpu
def test_agc_nodes_and_bank_follow_the_fixtures(tmp_path):
    exe = build("test_agc.cc")
    n = write_cases(tmp_path / "cases.txt")
    write_tau_cases(tmp_path / "tau.txt", tmp_path)
    r = subprocess.run([exe, str(tmp_path / "cases.txt"), R.GOLDEN, str(tmp_path / "tau.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "nodes: %d streams" % n in r.stdout and r.stdout.count("setTau g20_agc_") == 2
    assert "processDev i16: %d rows" % (n // 2) in r.stdout and "processDev f32: %d rows" % (n // 2) in r.stdout
