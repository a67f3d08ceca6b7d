"""numpy float64 restatement of the polyphase channelizer (include/sdrhip_channelizer.h) — TEST CODE, the node's check: it has no
reference node behind it. Two forms of the same numbers:

    direct(x, h32, M, D, channels)   the definition, for a list of channels:
        y_k[m] = sum_l h[l] x[t_m - l] exp(-2 pi i k (t_m - l) / M),  t_m = (m + 1) D - 1,  x[t] = 0 for t < 0
    folded(x, h32, M, D)             the fast form, all M channels: the branch sums u_m[r] over p in order, the circular shift by
        the absolute time, an unnormalised backward DFT (numpy's ifft times M)

and Stream, the streaming state (the count and the samples a later output still needs), so that a sequence of calls can be
replayed: every output is computed from the whole history with the same operations wherever the call boundaries fall.
Samples are complex128 arrays (pairs(x) makes them of [n, 2] rows); taps are the float32-rounded values (round32)."""
import numpy as np


def round32(taps):
    """the prototype as the node uses it: doubles rounded once to float32, as float64 values"""
    return np.asarray(taps, np.float64).astype(np.float32).astype(np.float64)


def pairs(x):
    """[n, 2] (re, im) rows of any real type -> complex128 [n]"""
    x = np.asarray(x)
    return x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)


def out_count(consumed, n, D):
    return (consumed + n) // D - consumed // D


def _window(x, t, n):
    """x[t], x[t - 1], ... x[t - n + 1] with zeros before the stream's start"""
    w = np.zeros(n, np.complex128)
    k = min(n, t + 1)
    w[:k] = x[t - k + 1:t + 1][::-1]
    return w


def direct(x, h32, M, D, channels, first=0, count=None):
    """outputs first ... first + count of the channels listed, from the whole stream x (complex128): [len(channels), count]"""
    h32, channels = np.asarray(h32, np.float64), np.asarray(channels, np.int64)
    count = len(x) // D - first if count is None else count
    y = np.zeros((len(channels), count), np.complex128)
    l = np.arange(len(h32))
    for j in range(count):
        t = (first + j + 1) * D - 1
        hx = h32 * _window(x, t, len(h32))
        ph = np.exp(-2j * np.pi * ((channels[:, None] * ((t - l) % M)[None, :]) % M) / M)   # (the phase's argument reduced exactly)
        y[:, j] = ph @ hx
    return y


def folded(x, h32, M, D, first=0, count=None):
    """the same outputs of all M channels by the fast form: [M, count]"""
    h32 = np.asarray(h32, np.float64)
    P = -(-len(h32) // M)
    hp = np.zeros(P * M)
    hp[:len(h32)] = h32
    count = len(x) // D - first if count is None else count
    y = np.zeros((M, count), np.complex128)
    r = np.arange(M)
    for j in range(count):
        t = (first + j + 1) * D - 1
        prod = (hp * _window(x, t, P * M)).reshape(P, M)
        u = np.zeros(M, np.complex128)
        for p in range(P):                       # in that order
            u = u + prod[p]
        w = np.zeros(M, np.complex128)
        w[(r - t) % M] = u
        y[:, j] = np.fft.ifft(w) * M
    return y


class Stream:
    """The node as a sequence of calls: process(x) -> [rows, n_out] complex128 of the selected channels (all M by default)."""

    def __init__(self, taps, M, D, channels=None, form=folded):
        self.M, self.D, self.h = int(M), int(D), round32(taps)
        self.selected = list(range(self.M)) if channels is None else [int(k) for k in channels]
        self.form = form
        self.reset()

    def reset(self):
        self.consumed, self.x = 0, np.zeros(0, np.complex128)   # x: the stream from t = 0 (the replay keeps all of it)

    def set_taps(self, taps):
        h = round32(taps)
        assert h.size == self.h.size
        self.h = h

    def set_channels(self, channels):
        self.selected = list(range(self.M)) if channels is None else [int(k) for k in channels]

    def out_count(self, n):
        return out_count(self.consumed, n, self.D)

    def process(self, x):
        x = np.asarray(x)
        x = pairs(x) if x.ndim == 2 else x.astype(np.complex128)
        first, count = self.consumed // self.D, self.out_count(len(x))
        self.x = np.concatenate([self.x, x])
        self.consumed += len(x)
        if self.form is folded:
            return folded(self.x, self.h, self.M, self.D, first, count)[self.selected]
        return direct(self.x, self.h, self.M, self.D, self.selected, first, count)

    def state(self):
        """(consumed, the last n_taps - 1 samples as [n_taps - 1, 2] float64, oldest first, zeros before the stream's start)"""
        n = self.h.size - 1
        tail = np.zeros(n, np.complex128)
        k = min(n, len(self.x))
        if k:
            tail[n - k:] = self.x[len(self.x) - k:]
        return self.consumed, np.stack([tail.real, tail.imag], axis=1)


def as_rows(y):
    """complex [rows, n] -> float64 [rows, n, 2]"""
    return np.stack([y.real, y.imag], axis=-1)
