"""C++ side of the channel power monitor (include/sdr/gpu/chanpower.hh), built the way tests/test_cpp_channelizer.py builds its
program. tests/cpp/test_chanpower.cc checks the constructor's and the setters' rules on the host (no GPU needed), and on the GPU
runs a cs16 stream through a graph Source -> gpu::ChannelPower<int16_t> in two buffers against the values this side wrote from
the numpy restatement (sums and levels <= 1e-5 of the largest, occupied() exactly), then reset() and the same buffers again, then
the state alone through processDev."""
import subprocess

import numpy as np
import pytest

import chanpower_restatement as P
from cpp_build import build


def test_the_constructor_refuses_what_create_refuses():
    exe = build("test_chanpower.cc")
    r = subprocess.run([exe, "rules"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rules: 20 refused" in r.stdout


def _case():
    """two carriers over noise; the second buffer has only one of them left"""
    M, D, n_taps, alpha = 12, 6, 30, 0.5
    lens = [600, 594]
    rng = np.random.default_rng(12)
    n = sum(lens)
    t = np.arange(n)
    x = 100.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x += 6000.0 * np.exp(2j * np.pi * 3 * t / M) + (t < lens[0]) * 6000.0 * np.exp(2j * np.pi * (8 * t / M + 0.3))
    x = np.stack([np.round(x.real), np.round(x.imag)], axis=1).astype(np.int16)
    tt = np.arange(n_taps) - (n_taps - 1) / 2
    taps = np.sinc(tt / M) / M * np.hanning(n_taps + 2)[1:-1]
    return M, D, n_taps, alpha, lens, x, taps


def test_the_case_keeps_its_margins():
    M, D, n_taps, alpha, lens, x, taps = _case()
    mon = P.Monitor(taps, M, D, alpha)
    mon.process(x[:lens[0]])
    carrier = mon.level[3]
    open_thr, close_thr = 0.8 * carrier, 0.6 * carrier
    mon.reset()
    mon.set_thresholds(open_thr, close_thr)
    mon.process(x[:lens[0]])
    assert mon.occupied() == [3, 8] and np.delete(mon.level, [3, 8]).max() < 0.1 * open_thr and mon.level[8] > 1.1 * open_thr
    mon.process(x[lens[0]:])
    assert mon.occupied() == [3] and mon.level[8] < 0.9 * close_thr and mon.level[3] > 1.1 * close_thr


@pytest.mark.gpu
def test_chanpower_in_a_graph_follows_the_restatement(tmp_path):
    exe = build("test_chanpower.cc")
    M, D, n_taps, alpha, lens, x, taps = _case()
    mon = P.Monitor(taps, M, D, alpha)
    mon.process(x[:lens[0]])
    open_thr, close_thr = 0.8 * mon.level[3], 0.6 * mon.level[3]
    mon.reset()
    mon.set_thresholds(open_thr, close_thr)
    want, occ, off = [], [], 0
    for n in lens:
        want += [mon.process(x[off:off + n]).copy(), mon.level.copy()]
        occ.append(mon.occupied())
        off += n
    assert occ == [[3, 8], [3]]
    with open(tmp_path / "case.txt", "w") as f:
        f.write("%d %d %d %.17g %.17g %.17g %d %d " % (M, D, n_taps, alpha, open_thr, close_thr, lens[0], lens[1]))
        f.write(" ".join(str(v) for o in occ for v in [len(o)] + o) + "\n")
    taps.astype(np.float64).tofile(tmp_path / "taps.bin")
    x.tofile(tmp_path / "x.bin")
    np.array(want, np.float64).tofile(tmp_path / "want.bin")
    r = subprocess.run([exe, "graph"] + [str(tmp_path / v) for v in ("case.txt", "taps.bin", "x.bin", "want.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "graph: %d channels, occupied 2 then 1" % M in r.stdout and "reset: 2 buffers again" in r.stdout and "processDev: 2 buffers" in r.stdout
