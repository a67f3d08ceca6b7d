"""C++ side of the audio channelizer (include/sdr/gpu/chanaudio.hh), built the way tests/test_cpp_channelizer.py builds its
program. tests/cpp/test_chanaudio.cc checks the constructor's rules on the host (no GPU needed), and on the GPU runs a cs16 stream
through a graph Source -> gpu::AudioChannelizer<int16_t> -> one Sink per selected row, in two buffers, mixed FM / AM / USB rows,
bit for bit against the int16 rows this side's wrapper made of the same buffers (which tests/test_gpu_parity_chanaudio.py holds
to the reference), then the same buffers as device rows through processDev."""
import subprocess

import numpy as np
import pytest

from cpp_build import build


def test_the_constructor_refuses_what_create_refuses():
    exe = build("test_chanaudio.cc")
    r = subprocess.run([exe, "rules"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rules: 15 constructions refused" in r.stdout


@pytest.mark.gpu
def test_audio_channelizer_in_a_graph_equals_the_python_side(tmp_path):
    import libsdr_amd as sa
    exe = build("test_chanaudio.cc")
    M, D, n_taps = 12, 5, 30
    sel, modes = [11, 0, 5, 6], [sa.EPI_AM, sa.EPI_FM, sa.EPI_USB, sa.EPI_FM]
    lens = [603, 897]
    n = sum(lens)
    assert n % D == 0
    rng = np.random.default_rng(12)
    x = rng.integers(-20000, 20000, (n, 2)).astype(np.int16)
    t = np.arange(n_taps) - (n_taps - 1) / 2
    taps = np.sinc(t / M) / M * np.hanning(n_taps + 2)[1:-1]
    all_modes, all_gains = [sa.EPI_FM] * M, np.ones(M, np.float32)
    for i, k in enumerate(sel):
        all_modes[k], all_gains[k] = modes[i], 0.5 + i
    ctx = sa.Context(0)
    node = sa.AudioChannelizer(ctx, np.int16, M, D, taps, modes=all_modes, gains=all_gains, channels=sel, max_in=max(lens))
    want = np.concatenate([node.process(x[:lens[0]]), node.process(x[lens[0]:])], axis=1)
    node.close()
    ctx.close()
    assert want.shape == (len(sel), n // D) and want.dtype == np.int16 and all(want[i].any() for i in range(len(sel)))
    with open(tmp_path / "case.txt", "w") as f:
        f.write(" ".join(str(v) for v in [M, D, n_taps, n, len(sel)] + [v for p in zip(sel, modes) for v in p] + [len(lens)] + lens) + "\n")
    taps.astype(np.float64).tofile(tmp_path / "taps.bin")
    x.tofile(tmp_path / "x.bin")
    want.tofile(tmp_path / "want.bin")
    r = subprocess.run([exe, "graph"] + [str(tmp_path / v) for v in ("case.txt", "taps.bin", "x.bin", "want.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "graph: %d rows x %d outputs" % (len(sel), n // D) in r.stdout and "processDev: %d rows" % len(sel) in r.stdout
