"""C++ side of the real-input channelizer family (include/sdr/gpu/chanreal.hh), built the way tests/test_cpp_channelizer.py builds
its program. tests/cpp/test_chanreal.cc checks the three constructors' rules, the setters' and config()'s input-type rule on the
host (no GPU needed), and on the GPU runs a real int16 stream through a graph Source -> gpu::RealChannelizer<int16_t> -> one Sink
per selected row, buffer by buffer, against the values this side wrote from the numpy restatement (<= 1e-5 of the largest), then
the same stream as device rows through processDev; gpu::RealAudioChannelizer<int16_t> and gpu::RealChannelPower<int16_t> take the
same stream in a graph and through processDev and are held, bit for bit, to what the Python nodes (which the parity tests hold to
the restatements) give for the same buffers on the same device."""
import subprocess

import numpy as np
import pytest

import channelizer_restatement as R
import chanreal_restatement as RR
from cpp_build import build


def test_the_constructor_refuses_what_create_refuses():
    exe = build("test_chanreal.cc")
    r = subprocess.run([exe, "rules"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rules: 14 constructions refused" in r.stdout and "rules: audio: 10 constructions refused" in r.stdout
    assert "rules: power: 11 refused" in r.stdout and "rules: config: 4 input types refused" in r.stdout


@pytest.mark.gpu
def test_real_channelizer_in_a_graph_follows_the_restatement(tmp_path):
    exe = build("test_chanreal.cc")
    M, D, n_taps = 12, 5, 30
    sel = [6, 0, 5, 3]
    lens = [600, 1, 4, 7, 0, 595, 298]
    n = sum(lens)
    assert n % D == 0
    rng = np.random.default_rng(12)
    x = rng.integers(-20000, 20000, n).astype(np.int16)
    x[5], x[6] = 32767, -32768
    taps = RR.prototype(M, n_taps)
    want = RR.folded_real(x, RR.round32(taps), M, D)[sel]
    with open(tmp_path / "case.txt", "w") as f:
        f.write(" ".join(str(v) for v in [M, D, n_taps, n, len(sel)] + sel + [len(lens)] + lens) + "\n")
    taps.astype(np.float64).tofile(tmp_path / "taps.bin")
    x.tofile(tmp_path / "x.bin")
    R.as_rows(want).astype(np.float64).tofile(tmp_path / "want.bin")
    r = subprocess.run([exe, "graph"] + [str(tmp_path / v) for v in ("case.txt", "taps.bin", "x.bin", "want.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "graph: %d rows x %d outputs" % (len(sel), n // D) in r.stdout and "processDev: %d rows" % len(sel) in r.stdout


M, D, N_TAPS = 12, 5, 30
LENS = [600, 1, 4, 7, 0, 595, 298]


def _stream(tmp_path, sel):
    """the case files the program reads; -> (x, taps)"""
    n = sum(LENS)
    assert n % D == 0
    rng = np.random.default_rng(12)
    x = rng.integers(-20000, 20000, n).astype(np.int16)
    x[5], x[6] = 32767, -32768
    taps = RR.prototype(M, N_TAPS)
    with open(tmp_path / "case.txt", "w") as f:
        f.write(" ".join(str(v) for v in [M, D, N_TAPS, n, len(sel)] + sel + [len(LENS)] + LENS) + "\n")
    taps.astype(np.float64).tofile(tmp_path / "taps.bin")
    x.tofile(tmp_path / "x.bin")
    return x, taps


def _cut(x):
    off = 0
    for n in LENS:
        yield x[off:off + n]
        off += n


@pytest.mark.gpu
def test_real_audio_channelizer_in_a_graph_equals_the_python_node(tmp_path):
    import libsdr_amd as sa
    exe = build("test_chanreal.cc")
    sel = [6, 0, 5, 3]
    x, taps = _stream(tmp_path, sel)
    K = M // 2 + 1
    modes, gains = [sa.EPI_FM] * K, np.ones(K, np.float32)
    for i, k in enumerate(sel):                      # row i: (FM, AM, USB)[i % 3], 0.75 + 0.5 i, as the program sets them
        modes[k], gains[k] = (sa.EPI_FM, sa.EPI_AM, sa.EPI_USB)[i % 3], np.float32(0.75) + np.float32(0.5) * np.float32(i)
    ctx = sa.Context(0)
    node = sa.AudioChannelizer(ctx, np.int16, M, D, taps, modes=modes, gains=gains, channels=sel, max_in=len(x), real=True)
    want = np.concatenate([node.process(part) for part in _cut(x)], axis=1)
    node.reset()
    one = node.process(x)
    node.close()
    ctx.close()
    assert want.shape == one.shape == (len(sel), len(x) // D) and want.any()
    want.tofile(tmp_path / "want.bin")
    one.tofile(tmp_path / "one.bin")
    r = subprocess.run([exe, "audio"] + [str(tmp_path / v) for v in ("case.txt", "taps.bin", "x.bin", "want.bin", "one.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "audio: %d rows x %d outputs" % (len(sel), len(x) // D) in r.stdout and "audio processDev: %d rows" % len(sel) in r.stdout


@pytest.mark.gpu
def test_real_channel_power_in_a_graph_equals_the_python_node(tmp_path):
    import libsdr_amd as sa
    exe = build("test_chanreal.cc")
    x, taps = _stream(tmp_path, [0])
    K = M // 2 + 1
    ctx = sa.Context(0)
    free = sa.ChannelPower(ctx, np.int16, M, D, taps, alpha=0.375, max_in=len(x), real=True)
    one = free.process(x)
    thr = float(np.median(free.levels()[0]))         # the first call's level is its mean: some channels open, some do not
    free.close()
    node = sa.ChannelPower(ctx, np.int16, M, D, taps, alpha=0.375, max_in=len(x), real=True)
    node.set_thresholds(thr, 0.5 * thr)
    for part in _cut(x):
        if len(part):
            sums = node.process(part)
    level, flags = node.levels()
    node.close()
    ctx.close()
    assert 0 < flags.sum() < K
    np.concatenate([[thr], sums, level, flags.astype(np.float64), one]).astype(np.float64).tofile(tmp_path / "want.bin")
    r = subprocess.run([exe, "power"] + [str(tmp_path / v) for v in ("case.txt", "taps.bin", "x.bin", "want.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "power: %d channels" % K in r.stdout and "power processDev: %d sums" % K in r.stdout
