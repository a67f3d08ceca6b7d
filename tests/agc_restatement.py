"""numpy restatement of the reference's AGC<int16_t> / AGC<float> (src/utils.hh:658-793), float32 operation by float32 operation,
vectorised over channels and looping over samples. tests/test_agc_restatement.py holds it against the g20_agc_* fixtures cut
from the compiled reference; the GPU tests hold the device node against it.

    lambda = float32(exp(-1 / (double(float32(tau)) * Fs)))      the member _tau is a float; exp in double, narrowed once
    per sample:  sd = fl(fl(lambda * sd) + fl(fl(1 - lambda) * |x|));  gain = target / fl(4 * sd) while enabled;  y = fl(gain * x)
    int16: out = 0 unless |y| < 2^31, else the low 16 bits of int32(trunc(y)) (x86's cvttss2si and a 16-bit truncation)
A row that is disabled with gain 0 copies its samples and keeps its state.
"""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32


def design_lambda(tau, Fs):
    return f32(math.exp(-1.0 / (float(f32(tau)) * float(Fs))))


def design_target(dtype):
    return f32(16000.0) if np.dtype(dtype) == np.int16 else f32(0.5)


class Bank:
    """`channels` AGC nodes: lam, target per channel (scalars broadcast; target 0: the type's default)."""

    def __init__(self, dtype, lam, target=0.0, enabled=True, channels=None):
        self.dtype = np.dtype(dtype)
        assert self.dtype in (np.dtype(np.int16), np.dtype(np.float32))
        n = channels if channels is not None else np.size(lam)
        self.lam = np.broadcast_to(np.asarray(lam, f32), (n,)).copy()
        t = np.broadcast_to(np.asarray(target, f32), (n,)).copy()
        t[t == 0] = design_target(self.dtype)
        self.target = t
        self.enabled = np.broadcast_to(np.asarray(enabled, bool), (n,)).copy()
        self.channels = n
        self.reset()

    def reset(self):
        self.sd, self.gain = self.target.copy(), np.ones(self.channels, f32)

    def set_channel(self, c, lam, target=0.0):
        self.lam[c] = f32(lam)
        self.target[c] = f32(target) if target else design_target(self.dtype)
        self.sd[c], self.gain[c], self.enabled[c] = self.target[c], f32(1), True

    def process(self, x):
        x = np.asarray(x, self.dtype)
        if x.ndim == 1:
            x = x[None]
        assert x.shape[0] == self.channels, x.shape
        n = x.shape[1]
        out = x.copy()
        walk = ~(~self.enabled & (self.gain == 0))
        if n == 0 or not walk.any():
            return out
        xf = x.astype(f32)
        a = np.abs(x.astype(np.int32)).astype(f32) if self.dtype == np.int16 else np.abs(xf)
        with np.errstate(all="ignore"):
            c = (f32(1) - self.lam)[:, None] * a          # fl(oml * |x|), one rounding
            SD = np.empty((self.channels, n), f32)
            sd, lam = self.sd.copy(), self.lam
            for i in range(n):
                sd = lam * sd + c[:, i]
                SD[:, i] = sd
            g = np.where(self.enabled[:, None], self.target[:, None] / (f32(4) * SD), self.gain[:, None]).astype(f32)
            y = g * xf
            if self.dtype == np.int16:
                ok = np.abs(y) < f32(2147483648.0)
                y = (np.trunc(np.where(ok, y, f32(0))).astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)
        assert y.dtype == self.dtype
        out[walk] = y[walk]
        if n:
            self.sd = np.where(walk, SD[:, -1], self.sd).astype(f32)
            self.gain = np.where(walk & self.enabled, g[:, -1], self.gain).astype(f32)
        return out


def same(got, want):
    """Bit for bit, except where BOTH sides are NaN (x86's inf * 0 is the negative quiet NaN, the GPU's the positive one)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return bool(np.array_equal(got, want))
    both = np.isnan(got) & np.isnan(want)
    return bool(np.array_equal(got.view(np.uint32)[~both], want.view(np.uint32)[~both]))


def bits_f32(u):
    return np.array([u], np.uint32).view(f32)[0]


def manifest():
    with open(os.path.join(GOLDEN, "manifest_agc.json")) as f:
        return json.load(f)


def load(name, m=None):
    """-> (meta, x, y) of one fixture stream"""
    m = (m or manifest())[name]
    dt = np.int16 if m["dtype"] == "i16" else np.float32
    x, y = (np.fromfile(os.path.join(GOLDEN, m[k]), dt) for k in ("x", "y"))
    assert x.size == m["count"] and y.size == m["count"], name
    return m, x, y


def apply_ops(node, c, m, b):
    """the fixture's setter calls in front of buffer b, on channel c of a Bank or of a wrapper with the same setters"""
    for op in m["ops"]:
        if op["at"] == b:
            v = bits_f32(op["value_bits"])
            if op["what"] == "enable":
                if isinstance(node, Bank):
                    node.enabled[c] = bool(v)
                else:
                    node.set_enabled(c, bool(v))
            elif isinstance(node, Bank):
                node.gain[c] = v
            else:
                node.set_gain(c, float(v))


def buffers(m):
    """-> [(offset, length)] of the recorded call split"""
    out, off = [], 0
    for n in m["lens"]:
        out.append((off, n))
        off += n
    return out
