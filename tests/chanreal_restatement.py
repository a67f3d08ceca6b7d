"""numpy float64 restatement of the channelizer family for a real-sampled row (include/sdrhip_chanreal.h) — TEST CODE, the
nodes' check. Two forms of the same numbers, rows k = 0 ... H with H = M / 2:

    direct_real(x, h32, M, D)   the definition: channelizer_restatement.direct on (x, 0), channels 0 ... H
    folded_real(x, h32, M, D)   the fast form in the header's order: the real branch sums u_m[r] over p in order, the circular
        shift by the absolute time, z[j] = w[2 j] + i w[2 j + 1], an unnormalised backward H-point DFT (numpy's ifft times H) and
        the untangling pass — per pair (k, kp = (H - k) mod H): er, ei, qr, qi, pr, pi, y_k = (er + pr, ei + pi),
        y_kp = (er - pr, pi - ei), the second value of k = 0 being y_H

and Stream, the streaming state, as channelizer_restatement.Stream. Samples are float64 arrays [n]; taps are the float32-rounded
values (channelizer_restatement.round32)."""
import numpy as np

import channelizer_restatement as R

round32, out_count = R.round32, R.out_count

# (M, D, n_taps) of the GPU parity test, which test_chanreal_restatement.py holds the two forms to as well: H = 2, the smallest
# plan, with D = M and a D that divides nothing; H = 4; H = 6, mixed radix; H = 13, one odd pass; n_taps < M, empty branches;
# H = 7 * 11; H = 500; H = 2048, the largest image and the smallest T, with n_taps a multiple of M and one above
SHAPES = [(4, 4, 5), (4, 3, 9), (8, 8, 24), (12, 5, 30), (26, 13, 57), (64, 64, 40), (154, 77, 500), (1000, 500, 3000),
          (4096, 4096, 8192), (4096, 2048, 4097)]


def prototype(M, n_taps):
    """a windowed sinc of cutoff fs / (2 M), as doubles (any finite prototype would do)"""
    t = np.arange(n_taps) - (n_taps - 1) / 2
    return np.sinc(t / M) / M * np.hanning(n_taps + 2)[1:-1]


def channels(M):
    return list(range(M // 2 + 1))


def tile_times(M):
    """the header's plan rule: T = min(256, E / M), E = 4096 complex elements for M <= 512 and 8192 above"""
    return min(256, (4096 if M <= 512 else 8192) // M)


def image_stride(M):
    """ld = (H + 1) | 1 complex elements"""
    return (M // 2 + 1) | 1


def direct_real(x, h32, M, D, first=0, count=None):
    """outputs first ... first + count of the channels 0 ... H from the whole stream x (real): [H + 1, count] complex128"""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and M % 2 == 0
    return R.direct(x.astype(np.complex128), h32, M, D, channels(M), first, count)


def _window(x, t, n):
    """x[t], x[t - 1], ... x[t - n + 1] with zeros before the stream's start"""
    w = np.zeros(n, np.float64)
    k = min(n, t + 1)
    w[:k] = x[t - k + 1:t + 1][::-1]
    return w


def folded_real(x, h32, M, D, first=0, count=None):
    """the same outputs by the fast form: [H + 1, count] complex128"""
    x, h32 = np.asarray(x, np.float64), np.asarray(h32, np.float64)
    assert x.ndim == 1 and M % 2 == 0
    H = M // 2
    P = -(-len(h32) // M)
    hp = np.zeros(P * M)
    hp[:len(h32)] = h32
    count = len(x) // D - first if count is None else count
    y = np.zeros((H + 1, count), np.complex128)
    r = np.arange(M)
    k = np.arange(H // 2 + 1)
    kp = (H - k) % H
    c, s = np.cos(2 * np.pi * k / M), np.sin(2 * np.pi * k / M)
    for j in range(count):
        t = (first + j + 1) * D - 1
        prod = (hp * _window(x, t, P * M)).reshape(P, M)
        u = np.zeros(M)
        for p in range(P):                       # in that order
            u = u + prod[p]
        w = np.zeros(M)
        w[(r - t) % M] = u
        Z = np.fft.ifft(w[0::2] + 1j * w[1::2]) * H
        a, b = Z[k], Z[kp]
        er, ei = 0.5 * (a.real + b.real), 0.5 * (a.imag - b.imag)
        qr, qi = 0.5 * (a.imag + b.imag), 0.5 * (b.real - a.real)
        pr, pi = c * qr - s * qi, c * qi + s * qr
        second = (er - pr) + 1j * (pi - ei)
        y[kp[1:], j] = second[1:]                # (H even: k = H / 2 is its own partner, and y_k below overwrites it)
        y[H, j] = second[0]
        y[k, j] = (er + pr) + 1j * (ei + pi)
    return y


class Stream:
    """The node as a sequence of calls: process(x) -> [rows, n_out] complex128 of the selected channels (0 ... H by default)."""

    def __init__(self, taps, M, D, channels_=None, form=folded_real):
        self.M, self.D, self.h = int(M), int(D), round32(taps)
        self.set_channels(channels_)
        self.form = form
        self.reset()

    def reset(self):
        self.consumed, self.x = 0, np.zeros(0, np.float64)   # x: the stream from t = 0 (the replay keeps all of it)

    def set_taps(self, taps):
        h = round32(taps)
        assert h.size == self.h.size
        self.h = h

    def set_channels(self, channels_):
        self.selected = channels(self.M) if channels_ is None else [int(k) for k in channels_]

    def out_count(self, n):
        return out_count(self.consumed, n, self.D)

    def process(self, x):
        x = np.asarray(x, np.float64)
        assert x.ndim == 1
        first, count = self.consumed // self.D, self.out_count(len(x))
        self.x = np.concatenate([self.x, x])
        self.consumed += len(x)
        return self.form(self.x, self.h, self.M, self.D, first, count)[self.selected]

    def state(self):
        """(consumed, the last n_taps - 1 samples as (re, 0) rows [n_taps - 1, 2] float64, oldest first)"""
        n = self.h.size - 1
        tail = np.zeros((n, 2), np.float64)
        k = min(n, len(self.x))
        if k:
            tail[n - k:, 0] = self.x[len(self.x) - k:]
        return self.consumed, tail
