"""The channelizer's numpy restatement (tests/channelizer_restatement.py) checked against itself, without a GPU: the fast form
equals the definition, the streaming replay does not depend on the call lengths, the output-count rule holds, and a designed
prototype puts a tone at a channel's centre into that channel's row and nowhere else."""
import numpy as np
import pytest

import channelizer_restatement as R

CASES = [(8, 8, 24), (8, 4, 21), (12, 6, 30), (12, 4, 12), (16, 16, 5), (6, 2, 40), (10, 10, 64), (8, 3, 24)]


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _taps(n, seed):
    return R.round32(np.random.default_rng(seed).standard_normal(n) / np.sqrt(n))


@pytest.mark.parametrize("M,D,n_taps", CASES, ids=["%d-%d-%d" % c for c in CASES])
def test_folded_equals_direct(M, D, n_taps):
    x, h = _signal(7 * M + 3, 100 + M + D), _taps(n_taps, n_taps)
    want = R.direct(x, h, M, D, range(M))
    got = R.folded(x, h, M, D)
    assert got.shape == want.shape == (M, len(x) // D)
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err <= 1e-12, err


@pytest.mark.parametrize("M,D,n_taps", [(8, 8, 24), (8, 3, 21), (12, 6, 30), (16, 16, 5)], ids=str)
def test_a_split_stream_equals_the_unsplit_one_exactly(M, D, n_taps):
    rng = np.random.default_rng(M * 100 + D)
    lens = [0, 1, D - 1, D, D + 1] + [int(v) for v in rng.integers(0, 4 * M, 9)] + [0, 1]
    x, h = _signal(sum(lens), 7), _taps(n_taps, 8)
    whole = R.Stream(h, M, D).process(x)
    s, parts, off = R.Stream(h, M, D), [], 0
    for n in lens:
        assert s.out_count(n) == (off + n) // D - off // D
        y = s.process(x[off:off + n])
        assert y.shape == (M, (off + n) // D - off // D)
        parts.append(y)
        off += n
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    assert s.state()[0] == len(x)
    tail = s.state()[1]
    assert tail.shape == (n_taps - 1, 2) and np.array_equal(tail[:, 0] + 1j * tail[:, 1], x[len(x) - (n_taps - 1):])
    # a subset, in any order, is those rows; the definition gives them too
    sel = [M - 1, 0, 3]
    assert np.array_equal(R.Stream(h, M, D, channels=sel).process(x), whole[sel])
    d = R.Stream(h, M, D, channels=sel, form=R.direct).process(x)
    assert np.abs(d - whole[sel]).max() <= 1e-12 * np.abs(whole).max()


def test_the_output_count_rule():
    for D in (1, 2, 3, 8):
        for N in range(0, 20):
            for n in range(0, 20):
                assert R.out_count(N, n, D) == len([t for t in range(N, N + n) if (t + 1) % D == 0])
    s = R.Stream([1.0], 4, 3)
    assert [s.process(np.zeros(n, np.complex128)).shape[1] for n in (0, 1, 1, 1, 2, 5, 0)] == [0, 0, 0, 1, 0, 2, 0]


def test_a_designed_prototype_puts_a_tone_into_its_channel():
    """sdrhip_design_fir_lowpass with upper_freq = fs / (2 M): a tone at channel 5's centre comes out of row 5 with the
    prototype's gain at 0 and is down in every other row by the prototype's own response at that row's offset, which lies in
    its stop band (from the adjacent channel's centre, fs / M, onwards)"""
    import libsdr_amd as sa
    M, D, fs, amp = 16, 8, 16000.0, 1000.0
    n_taps = 12 * M
    h = R.round32(sa.design_fir_lowpass(n_taps, fs / (2 * M), fs))
    n = n_taps + 40 * D
    t = np.arange(n)
    x = amp * np.exp(2j * np.pi * 5 * t / M)
    y = R.folded(x, h, M, D)
    settled = y[:, (np.arange(y.shape[1]) + 1) * D - 1 >= n_taps - 1]
    assert settled.shape[1] >= 30
    H = lambda f: abs(np.sum(h * np.exp(-2j * np.pi * f * np.arange(n_taps) / fs)))
    grid = np.abs(np.fft.fft(h, 64 * n_taps))
    f = np.fft.fftfreq(64 * n_taps, 1 / fs)
    stop = grid[np.abs(f) >= fs / M - 1e-9].max()
    assert stop < 0.05 * H(0.0), (stop, H(0.0))          # (the prototype has a stop band worth the name)
    level = np.abs(settled)
    assert np.allclose(level[5], amp * H(0.0), rtol=1e-9)
    for k in range(M):
        if k != 5:
            off = ((5 - k + M // 2) % M - M // 2) * fs / M
            assert np.allclose(level[k], amp * H(off), rtol=1e-6, atol=1e-9 * amp), k
            assert level[k].max() <= amp * stop * (1 + 1e-9), (k, level[k].max(), amp * stop)
