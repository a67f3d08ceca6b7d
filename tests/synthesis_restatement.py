"""numpy float64 restatement of the polyphase synthesis bank (include/sdrhip_synthesis.h) — TEST CODE, the node's check: it has no
reference node behind it. Two forms of the same numbers, for channel rows c [rows, n] complex128 on the channels listed:

    direct(c, g32, M, D, channels, times)   the definition, at the output times listed:
        z[t] = sum_k sum_m c_k[m] g[t - m D] exp(+2 pi i k t / M),  g[l] = 0 outside [0, n_taps), c_k[m] = 0 for m < 0
    folded(c, g32, M, D, channels)          the fast form, every output time of the columns: v_m = the unnormalised backward DFT of
        column m (numpy's ifft times M), z[t] = sum over q ascending with q D + d < n_taps of g[q D + d] v_(m0 - q)[t mod M],
        m0 = t div D, d = t mod D; a term beyond the taps is skipped, a column before the stream's start is zeros

and Stream, the streaming state (the count and the transformed columns), so that a sequence of calls — with set_taps and
set_channels between them — can be replayed. Rows are complex128 arrays (rows_of(x) makes them of [rows, n, 2]); taps are the
float32-rounded values (round32)."""
import numpy as np


def round32(taps):
    """the prototype as the node uses it: doubles rounded once to float32, as float64 values"""
    return np.asarray(taps, np.float64).astype(np.float32).astype(np.float64)


def rows_of(x):
    """[rows, n, 2] (re, im) of any real type -> complex128 [rows, n]"""
    x = np.asarray(x)
    return x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)


def as_pairs(z):
    """complex [...] -> float64 [..., 2]"""
    return np.stack([z.real, z.imag], axis=-1)


def _channels(channels, M, rows):
    ch = np.arange(M) if channels is None else np.asarray(channels, np.int64)
    assert ch.shape == (rows,), (ch.shape, rows)
    return ch


def direct(c, g32, M, D, channels=None, times=None):
    """z[t] at the output times listed (default: all n D of them), from the whole stream c [rows, n]: [len(times)]"""
    c, g = np.asarray(c, np.complex128), np.asarray(g32, np.float64)
    ch, n = _channels(channels, M, c.shape[0]), c.shape[1]
    times = np.arange(n * D) if times is None else np.asarray(times, np.int64)
    z = np.zeros(len(times), np.complex128)
    for i, t in enumerate(times):
        t = int(t)
        lo, hi = max(0, -((len(g) - 1 - t) // D)), min(t // D, n - 1)      # 0 <= t - m D < n_taps
        if hi < lo:
            continue
        m = np.arange(lo, hi + 1)
        s = c[:, m] @ g[t - m * D]
        z[i] = np.sum(s * np.exp(2j * np.pi * ((ch * t) % M) / M))         # (the phase's argument reduced exactly)
    return z


def transform(c, M, channels=None):
    """v [n, M]: the unnormalised backward DFT of every column of the rows c [rows, n] on the channels listed"""
    c = np.asarray(c, np.complex128)
    full = np.zeros((M, c.shape[1]), np.complex128)
    full[_channels(channels, M, c.shape[0])] = c
    return (np.fft.ifft(full, axis=0) * M).T


def overlap(v, g32, M, D, first, count):
    """z[t] for t in [first D, (first + count) D) from v [cols, M], v[i] being column i (columns below 0 are zeros)"""
    g = np.asarray(g32, np.float64)
    t = np.arange(first * D, (first + count) * D)
    m0, d, tm = t // D, t % D, t % M
    z = np.zeros(len(t), np.complex128)
    for q in range(-(-len(g) // D)):                  # in that order
        l, m = q * D + d, m0 - q
        ok = (l < len(g)) & (m >= 0)
        z[ok] = z[ok] + g[l[ok]] * v[m[ok], tm[ok]]
    return z


def folded(c, g32, M, D, channels=None):
    """all n D output times of the rows c [rows, n] by the fast form"""
    return overlap(transform(c, M, channels), g32, M, D, 0, np.asarray(c).shape[1])


def chain_case():
    """The synthesis -> analysis chain of tests/test_gpu_synthesis_chain.py, shared with the CPU test of its margins: M = 16,
    D = 8, the prototype sinc(l / M) hamming / M of 128 taps (l centred; the synthesis bank's taps are D h), three rows of 96
    columns on channels [3, 7, 12] — a 0.05-cycle tone, a constant 0.5 and a 0.03-cycle tone of amplitude 0.25.
    -> dict(M, D, h, channels, amplitudes, x [3, 96, 2] float32, delay, settled)"""
    M, D, n_taps, n = 16, 8, 128, 96
    l = np.arange(n_taps) - (n_taps - 1) / 2
    h = np.sinc(l / M) * np.hamming(n_taps) / M
    m = np.arange(n)
    rows = np.stack([np.exp(2j * np.pi * 0.05 * m), np.full(n, 0.5 + 0j), 0.25 * np.exp(2j * np.pi * 0.03 * m)])
    return dict(M=M, D=D, h=h, channels=[3, 7, 12], amplitudes=[1.0, 0.5, 0.25], x=as_pairs(rows).astype(np.float32), delay=15, settled=40)


def chain_margins(case, y):
    """What the chain's conditions measure on the analysis rows y [M, 96] complex: (the largest error of a used channel behind
    column `settled` against its input delayed by `delay` columns, relative to the row's amplitude; the strongest other
    channel's mean power under the strongest channel's, in dB). Both behind column `settled`: the rows switch on at column 0,
    and that step is in every channel until both filters have run past it (over all 96 columns the second figure is -43.8 dB
    on the restatements, behind column 40 it is -65.4 dB)."""
    c, dl, st = rows_of(case["x"]), case["delay"], case["settled"]
    err = max(float(np.abs(y[k, st:] - c[i, st - dl:c.shape[1] - dl]).max()) / a
              for i, (k, a) in enumerate(zip(case["channels"], case["amplitudes"])))
    power = np.mean(np.abs(y[:, st:]) ** 2, axis=1)
    others = [k for k in range(case["M"]) if k not in case["channels"]]
    return err, float(10 * np.log10(power[others].max() / power.max()))


class Stream:
    """The node as a sequence of calls: process(x) -> [n D] complex128."""

    def __init__(self, taps, M, D, channels=None):
        self.M, self.D, self.g = int(M), int(D), round32(taps)
        self.Q = -(-len(self.g) // self.D)
        self.selected = None if channels is None else [int(k) for k in channels]
        self.reset()

    def reset(self):
        self.consumed, self.v = 0, np.zeros((0, self.M), np.complex128)   # v: every transformed column from m = 0 (the replay keeps all)

    def set_taps(self, taps):
        g = round32(taps)
        assert g.size == self.g.size
        self.g = g

    def set_channels(self, channels):
        self.selected = None if channels is None else [int(k) for k in channels]

    def out_count(self, n):
        return n * self.D

    def process(self, x):
        x = np.asarray(x)
        x = rows_of(x) if x.ndim == 3 else x.astype(np.complex128)
        first, n = self.consumed, x.shape[1]
        self.v = np.concatenate([self.v, transform(x, self.M, self.selected)])
        self.consumed += n
        return overlap(self.v, self.g, self.M, self.D, first, n)

    def state(self):
        """(consumed, the last Q - 1 transformed columns as [Q - 1, M] complex128, oldest first, zeros before the stream's start)"""
        cols = np.zeros((self.Q - 1, self.M), np.complex128)
        k = min(self.Q - 1, len(self.v))
        if k:
            cols[self.Q - 1 - k:] = self.v[len(self.v) - k:]
        return self.consumed, cols
