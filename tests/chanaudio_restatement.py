"""The audio channelizer's steps 2 and 3 (include/sdrhip_chanaudio.h) in numpy, over GIVEN float32 channelizer rows: the
conversion to complex<int16> (one float32 multiply, round to nearest even, NaN -> 0, clamp) and the reference's three int16
demodulators with the library's per-call FM convention — out[0] = q[0].re, out[j] = last - phi[j] with int16 wrap, a call's
sample 0 never touches `last`. The FM angle is a vectorised fast_atan2<int16_t, int16_t> / 2, held to the oracle's
fast_atan2_i16 in tests/test_chanaudio_restatement.py. Nothing here imports the library."""
import numpy as np

FM, AM, USB = 1, 2, 3   # SDRHIP_EPI_FM, _AM, _USB


def convert(y32, gain):
    """[..., 2] float32 rows times a float32 gain (one, or an array that broadcasts) -> [..., 2] int16 (the header's numpy line)"""
    y32 = np.asarray(y32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.asarray(gain, np.float32) * y32)
    return np.clip(np.nan_to_num(v, nan=0), -32768, 32767).astype(np.int16)


def _tdiv(num, den):
    """C's truncating integer division, den > 0"""
    return np.sign(num) * (np.abs(num) // den)


def fast_atan2(a, b):
    """The reference's fast_atan2<int16_t, int16_t>(a, b) (src/math.hh:31-40) over int arrays: pi = 16384, integer division"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    aa = np.abs(a)
    den_p, den_n = np.maximum(b + aa, 1), np.maximum(aa - b, 1)
    pos = 4096 - _tdiv(4096 * (b - aa), den_p)
    neg = 3 * 4096 - _tdiv(4096 * (b + aa), den_n)
    ang = np.where(b >= 0, pos, neg)
    ang = np.where((a == 0) & (b == 0), 0, ang)
    return np.where(a < 0, -ang, ang)


def phi(q):
    """[..., 2] int16 -> the angle FMDemod<int16_t> differences: fast_atan2(re, im) / 2, truncating"""
    q = np.asarray(q, np.int64)
    return _tdiv(fast_atan2(q[..., 0], q[..., 1]), 2)


def am(q):
    q = np.asarray(q, np.int64)
    m = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]).astype(np.uint32).astype(np.int32)   # the reference's wrapping int32 sum
    with np.errstate(invalid="ignore"):
        r = np.sqrt(m.astype(np.float64))
    return np.nan_to_num(r, nan=-2147483648.0).astype(np.int64).astype(np.int16)   # (double)m -> int: never negative for int16 inputs but (-32768, -32768)


def usb(q):
    q = np.asarray(q, np.int64)
    return _tdiv(q[..., 0] + q[..., 1], 2).astype(np.int16)


def fm_call(q, last):
    """One call of one FM row: q [n, 2] int16, last int -> (out [n] int16, the new last)"""
    n = len(q)
    out = np.zeros(n, np.int16)
    if n == 0:
        return out, last
    out[0] = q[0, 0]
    if n >= 2:
        p = phi(q)
        prev = np.concatenate([[last], p[1:-1]])
        out[1:] = (prev - p[1:]).astype(np.int16)   # int16 wrap
        last = int(p[-1])
    return out, last


class Rows:
    """The per-channel state of an audio channelizer's rows: process(y32 [rows, n, 2] float32 of ONE call) -> [rows, n] int16.
    Row i has modes[i], gains[i] and last[i]; set_mode restarts a row's last at 0."""

    def __init__(self, modes, gains=None):
        self.modes = [int(m) for m in modes]
        self.gains = [np.float32(1)] * len(self.modes) if gains is None else [np.float32(g) for g in gains]
        self.last = [0] * len(self.modes)

    def set_mode(self, row, mode):
        self.modes[row], self.last[row] = int(mode), 0

    def set_gain(self, row, gain):
        self.gains[row] = np.float32(gain)

    def reset(self):
        self.last = [0] * len(self.modes)

    def process(self, y32, rows=None):
        """rows: the state rows that y32's rows belong to (default: all, in order)"""
        rows = list(range(len(self.modes)) if rows is None else rows)
        y32 = np.asarray(y32, np.float32)
        n = y32.shape[1]
        q = convert(y32, np.array([self.gains[r] for r in rows], np.float32)[:, None, None])
        mode = np.array([self.modes[r] for r in rows])
        out = np.zeros(y32.shape[:2], np.int16)
        out[mode == AM], out[mode == USB] = am(q[mode == AM]), usb(q[mode == USB])
        fm = np.flatnonzero(mode == FM)
        if n and len(fm):                                   # fm_call over all FM rows at once
            out[fm, 0] = q[fm, 0, 0]
            if n >= 2:
                p = phi(q[fm])
                prev = np.concatenate([np.array([[self.last[rows[i]]] for i in fm], np.int64), p[:, 1:-1]], axis=1)
                out[fm, 1:] = (prev - p[:, 1:]).astype(np.int16)
                for i, v in zip(fm, p[:, -1]):
                    self.last[rows[i]] = int(v)
        return out
