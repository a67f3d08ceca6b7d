"""numpy float64 restatement of the channel power monitor (include/sdrhip_chanpower.h) — TEST CODE, the node's check: it has no
reference node behind it. Built on channelizer_restatement.Stream: the sums are those of |y|^2 over a call's outputs, y the
restated channelizer's float64 values for all M channels; on top of them the level recursion, the hysteresis and the occupied
list, exactly as the header writes them:

    mean = sum / J;  level = mean if calls == 0 else level + alpha * (mean - level)
    open = !(level < close_thr) if open else level >= open_thr

Monitor replays a sequence of calls. Monitor.update(sums, J) makes the state step alone, from any sums — the GPU tests feed it
the DEVICE's sums, so that levels compare bit for bit."""
import numpy as np

import channelizer_restatement as R


def powers(y):
    """complex128 [M, J] -> the sums of |y|^2 over the J outputs, [M] float64 (zeros for J = 0)"""
    return (y.real * y.real + y.imag * y.imag).sum(axis=1)


class Monitor:
    """The node as a sequence of calls: process(x) -> sum [M] float64; level, open, calls as the header keeps them."""

    def __init__(self, taps, M, D, alpha, form=R.folded):
        self.M, self.alpha = int(M), float(alpha)
        assert 0.0 < self.alpha <= 1.0
        self.stream = R.Stream(taps, M, D, form=form)
        self.open_thr, self.close_thr = np.full(self.M, np.inf), np.zeros(self.M)
        self.reset()

    def reset(self):
        """as freshly created, with the current taps, alpha and thresholds"""
        self.stream.reset()
        self.level, self.open, self.calls = np.zeros(self.M), np.zeros(self.M, bool), 0

    def set_taps(self, taps):
        self.stream.set_taps(taps)

    def set_alpha(self, alpha):
        assert 0.0 < float(alpha) <= 1.0
        self.alpha = float(alpha)

    def set_thresholds(self, open_thr, close_thr):
        o, c = (np.array(np.broadcast_to(np.asarray(v, np.float64), (self.M,))) for v in (open_thr, close_thr))
        assert np.all(c >= 0.0) and np.all(c <= o)          # (a NaN fails the comparison it meets)
        self.open_thr, self.close_thr = o, c

    def out_count(self, n):
        return self.stream.out_count(n)

    def update(self, sums, J):
        """the state step of a call whose sums are given"""
        if J <= 0:
            return
        mean = np.asarray(sums, np.float64) / float(J)
        with np.errstate(invalid="ignore"):
            self.level = mean.copy() if self.calls == 0 else self.level + self.alpha * (mean - self.level)
            self.open = np.where(self.open, ~(self.level < self.close_thr), self.level >= self.open_thr)
        self.calls += 1

    def process(self, x):
        y = self.stream.process(x)
        sums = powers(y)
        self.update(sums, y.shape[1])
        return sums

    def occupied(self):
        return [int(k) for k in np.flatnonzero(self.open)]
