"""The channel power monitor's numpy restatement (tests/chanpower_restatement.py) checked against itself, without a GPU: the
sums of the fast form equal the definition's, a tone at a channel's centre gives that channel A^2 (sum h)^2 per output and the
other channels no more than the prototype's stop band, and the level recursion and the hysteresis follow a hand-written sequence
of means with the expected levels and flags written out."""
import numpy as np

import channelizer_restatement as R
import chanpower_restatement as P

INF, NAN = float("inf"), float("nan")


def _taps(M, n_taps):
    t = np.arange(n_taps) - (n_taps - 1) / 2
    return np.sinc(t / M) / M * np.hanning(n_taps + 2)[1:-1]


def test_sums_of_the_folded_form_against_the_direct_form():
    M, D, n_taps = 12, 5, 30
    rng = np.random.default_rng(5)
    x = rng.standard_normal(9 * M + 4) + 1j * rng.standard_normal(9 * M + 4)
    taps = _taps(M, n_taps)
    a, b = P.Monitor(taps, M, D, 0.5), P.Monitor(taps, M, D, 0.5, form=R.direct)
    off = 0
    for n in (0, 1, D - 1, D + 1, 40, len(x) - 40 - 2 * D - 1):
        J = a.out_count(n)
        assert J == (off + n) // D - off // D
        sa_, sb = a.process(x[off:off + n]), b.process(x[off:off + n])
        off += n
        assert sa_.shape == sb.shape == (M,) and sa_.dtype == np.float64
        if J == 0:
            assert not sa_.any() and not sb.any()
        else:
            assert np.abs(sa_ - sb).max() <= 1e-12 * sb.max()
    assert off == len(x) and a.calls == b.calls == 4                    # (the calls of 0 and 1 samples complete no output)
    assert np.abs(a.level - b.level).max() <= 1e-12 * b.level.max()
    # the sums are those of the plain restated channelizer's rows
    y = R.folded(x, R.round32(taps), M, D)
    whole = P.Monitor(taps, M, D, 1.0).process(x)
    assert np.array_equal(whole, (y.real ** 2 + y.imag ** 2).sum(axis=1))


def test_a_tone_at_a_channels_centre():
    """x[t] = A exp(2 pi i k0 t / M): once n_taps samples are in, y_k0[m] = A sum(h) exactly, so |y_k0|^2 = A^2 (sum h)^2; every
    other channel sees the prototype's response at a multiple of fs / M, which lies in its stop band"""
    M, D, k0, A = 16, 8, 5, 1000.0
    n_taps = 12 * M
    taps = _taps(M, n_taps)
    h = R.round32(taps)
    mon = P.Monitor(taps, M, D, 1.0)
    t = np.arange(n_taps + 1 + 41 * D)
    x = A * np.exp(2j * np.pi * k0 * t / M)
    last = len(x) - D
    head = n_taps + 1 - (n_taps + 1) % D + D                            # a whole number of blocks with n_taps samples in
    mon.process(x[:head])
    J = mon.out_count(last - head)
    s = mon.process(x[head:last])
    assert J >= 30
    want = A * A * h.sum() ** 2
    assert abs(s[k0] / J - want) <= 1e-9 * want, (s[k0] / J, want)
    assert abs(mon.level[k0] - want) <= 1e-9 * want                     # (alpha = 1: the level is the mean)
    grid = np.abs(np.fft.fft(h, 64 * n_taps))
    f = np.fft.fftfreq(64 * n_taps)
    stop = grid[np.abs(f) >= 1.0 / M - 1e-12].max()
    assert stop < 0.05 * abs(h.sum()), (stop, h.sum())                  # (the prototype has a stop band worth the name)
    others = np.delete(s, k0) / J
    assert others.max() <= (A * stop) ** 2 * (1 + 1e-9), (others.max(), (A * stop) ** 2)
    mon.set_thresholds(0.5 * want, 0.25 * want)
    mon.process(x[last:])                                               # (any call with J > 0 looks at the flags again)
    assert mon.occupied() == [k0]


class _Means(P.Monitor):
    """the state step alone: one channel per column, fed means directly (J = 1, so sum = mean)"""

    def __init__(self, M, alpha):
        self.M, self.alpha = M, alpha
        self.open_thr, self.close_thr = np.full(M, np.inf), np.zeros(M)
        self.level, self.open, self.calls = np.zeros(M), np.zeros(M, bool), 0


def test_the_level_recursion_and_the_hysteresis_on_a_written_sequence():
    # alpha = 0.5, open_thr = 8, close_thr = 4; every value below is exact in binary
    # channel 0: opens on equality, stays open at level == close_thr, closes just below
    # channel 1: never reaches the threshold; channel 2: a NaN mean in the third call
    m = _Means(3, 0.5)
    assert m.occupied() == [] and m.calls == 0
    m.update([100.0, 100.0, 100.0], 1)                                  # thresholds at their defaults: +inf and 0
    assert m.level.tolist() == [100.0, 100.0, 100.0] and m.occupied() == [] and m.calls == 1
    m = _Means(3, 0.5)
    m.set_thresholds(8.0, 4.0)                                          # (scalars go to every channel)
    assert m.open_thr.tolist() == [8.0] * 3 and m.close_thr.tolist() == [4.0] * 3
    steps = [
        # means                  levels behind the call        flags behind the call
        ([8.0, 7.5, 2.0],        [8.0, 7.5, 2.0],              [True, False, False]),     # the first call: level = mean; 8 >= 8 opens
        ([0.0, 8.0, 2.0],        [4.0, 7.75, 2.0],             [True, False, False]),     # 4 < 4 is false: stays open; 7.75 < 8
        ([3.5, 8.0, NAN],        [3.75, 7.875, NAN],           [False, False, False]),    # 3.75 < 4 closes
        ([12.25, 8.0, 100.0],    [8.0, 7.9375, NAN],           [True, False, False]),     # opens again on equality; NaN stays
        ([8.0, 8.0625, 100.0],   [8.0, 8.0, NAN],              [True, True, False]),
    ]
    for k, (means, levels, flags) in enumerate(steps):
        if k == 2:
            m.update([55.0, 55.0, 55.0], 0)                             # a call with J = 0 touches nothing
            assert m.calls == 2
        m.update(means, 1)
        assert np.array_equal(m.level, np.array(levels), equal_nan=True), (k, m.level)
        assert m.open.tolist() == flags and m.occupied() == [i for i, f in enumerate(flags) if f], (k, m.open)
    assert m.calls == 5
    # an OPEN channel whose level turns NaN stays open: both comparisons are false
    m.update([NAN, 0.0, 0.0], 1)
    assert np.isnan(m.level[0]) and m.open.tolist() == [True, True, False]
    m.update([0.0, 0.0, 0.0], 1)
    assert np.isnan(m.level[0]) and m.level[1] == 2.0 and m.open.tolist() == [True, False, False]
    # sums are divided by J
    j = _Means(1, 1.0)
    j.update([12.0], 3)
    assert j.level.tolist() == [4.0]
    # the rules of the thresholds and of alpha
    for bad in ((1.0, 2.0), (-1.0, -1.0), (NAN, 0.0), (1.0, NAN), (1.0, -0.5)):
        try:
            m.set_thresholds(*bad)
        except AssertionError:
            continue
        raise AssertionError("accepted %r" % (bad,))
    m.set_thresholds(INF, 0.0)
    m.set_thresholds(INF, INF)
    for bad in (0.0, -0.5, 1.5, NAN):
        try:
            m.set_alpha(bad)
        except AssertionError:
            continue
        raise AssertionError("accepted alpha %r" % bad)


def test_reset_keeps_taps_alpha_and_thresholds():
    M, D = 8, 4
    taps = _taps(M, 24)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    mon = P.Monitor(taps, M, D, 0.25)
    mon.set_thresholds(1e-3, 1e-4)
    first = [mon.process(x[:40]).copy(), mon.process(x[40:]).copy()]
    level, flags = mon.level.copy(), mon.open.copy()
    assert flags.any() and mon.calls == 2
    mon.reset()
    assert mon.calls == 0 and not mon.level.any() and not mon.open.any() and mon.occupied() == []
    again = [mon.process(x[:40]), mon.process(x[40:])]
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    assert np.array_equal(mon.level, level) and np.array_equal(mon.open, flags)
