"""The interpolating resampler bank restated in numpy from the contract in include/sdrhip_resample.h. The phase chain does not
depend on the samples: chain() walks it as a plain float32 loop, once per distinct (frac, mu, n), and answers which window of
the input and which table row every output of the call takes. The interpolation is then vectorised over the outputs and over the
rows that share a schedule: float32 arithmetic with every operation rounded on its own (numpy rounds each ufunc), the int16
accumulator converted back after every tap as x86 does (truncate to int32, keep the low 16 bits)."""
import functools
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32
DTYPES = ("f32", "cf32", "i16", "cs16_cf32")
CODE = {"f32": 0, "cf32": 1, "i16": 2, "cs16_cf32": 3}
IN_DT = {"f32": np.float32, "cf32": np.float32, "i16": np.int16, "cs16_cf32": np.int16}
OUT_DT = {"f32": np.float32, "cf32": np.float32, "i16": np.int16, "cs16_cf32": np.float32}
IQ = {"f32": False, "cf32": True, "i16": False, "cs16_cf32": True}
FRAC_MIN, FRAC_MAX = 0.125, 4096.0


def manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest_resample.json")))


def table():
    """The reference's interpolation table as its running program holds it: [129, 8] float32 (the BPSK31 bank's fixture)."""
    return np.fromfile(os.path.join(GOLDEN, "g21_psk31_table.bin"), f32).reshape(129, 8)


def fixture_names():
    return sorted(k for k in manifest() if k.startswith("g22_inpol_"))


def fixture(name):
    """-> (m, x [n(, 2)] of the input type, y [sum(counts)(, 2)] of the output type, lines [calls, 8(, 2)] of the output type)"""
    m = manifest()[name]
    d = m["dtype"]
    shape = (-1, 2) if IQ[d] else (-1,)
    x = np.fromfile(os.path.join(GOLDEN, m["x"]), IN_DT[d]).reshape(shape)
    y = np.fromfile(os.path.join(GOLDEN, m["y"]), OUT_DT[d]).reshape(shape)
    lines = np.fromfile(os.path.join(GOLDEN, m["lines"]), OUT_DT[d]).reshape((len(m["lens"]), 8, 2) if IQ[d] else (len(m["lens"]), 8))
    return m, x, y, lines


def out_capacity(fracs, n):
    """The bound of sdrhip_resample_out_capacity (see the header): the largest over the rows."""
    if n == 0:
        return 0
    return max(n if f32(f) == f32(1) else int(math.floor((n + 1.0) / float(f32(f)))) + 2 for f in np.atleast_1d(fracs))


def _bits(v):
    return int(np.asarray(v, f32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _chain(frac_bits, mu_bits, n):
    frac = np.array(frac_bits, np.uint32).view(f32)[()]
    mu = np.array(mu_bits, np.uint32).view(f32)[()]
    one = f32(1)
    pos, rows = [], []
    i = 0
    while i < n:
        while mu >= one and i < n:
            i += 1
            mu = f32(mu - one)
        while mu <= one:
            pos.append(i)
            rows.append(int(math.floor(float(mu) * 128.0 + 0.5)))   # roundf(mu * 128): mu >= 0, the product is exact
            mu = f32(mu + frac)
    return np.array(pos, np.int64), np.array(rows, np.int64), _bits(mu)


def chain(frac, mu, n):
    """The call's schedule: (pos, rows, mu after the call). Output o takes the 8 samples that end with the call's sample
    pos[o] - 1 (pos[o] = how many of the call's samples the line has taken) and the table row rows[o]."""
    pos, rows, mu_bits = _chain(_bits(frac), _bits(mu), int(n))
    return pos, rows, np.array(mu_bits, np.uint32).view(f32)[()]


def to_i16(v):
    """float32 -> int16 as x86 narrows it: truncate to int32 (0x80000000 out of range and for NaN), keep the low 16 bits"""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        ok = np.abs(v) < f32(2147483648.0)
        t = np.where(ok, np.trunc(np.where(ok, v, 0)), 0).astype(np.int64)
    return (t & 0xFFFF).astype(np.uint16).view(np.int16)


def interp(win, taps, i16):
    """win [..., 8(, 2)] windows, taps [..., 8] -> the sum from 0 in tap order; i16: the wrapping int16 accumulator"""
    iq = win.ndim == taps.ndim + 1
    with np.errstate(all="ignore"):
        if i16:
            acc = np.zeros(win.shape[:-1], np.int16)
            for k in range(8):
                acc = to_i16(acc.astype(f32) + win[..., k].astype(f32) * taps[..., k])
            return acc
        acc = np.zeros(win.shape[:-2] + (2,) if iq else win.shape[:-1], f32)
        for k in range(8):
            acc = acc + (win[..., k, :] * taps[..., k, None] if iq else win[..., k] * taps[..., k])
        return acc


class Bank:
    """`rows` InpolSubSampler nodes; fracs: one value or one per row; dtype: one of DTYPES; tab: the [129, 8] table."""

    def __init__(self, dtype, fracs, tab, rows=None):
        fracs = np.atleast_1d(np.asarray(fracs, f32))
        self.R = int(rows if rows is not None else fracs.size)
        self.frac = np.broadcast_to(fracs, (self.R,)).copy()
        assert np.all(np.isfinite(self.frac) & (self.frac >= FRAC_MIN) & (self.frac <= FRAC_MAX)), self.frac
        self.dtype, self.iq, self.out_dt = dtype, IQ[dtype], OUT_DT[dtype]
        self.tab = np.ascontiguousarray(tab, f32).reshape(129, 8)
        self.mu = np.zeros(self.R, f32)
        self.line = np.zeros((self.R, 8, 2) if self.iq else (self.R, 8), self.out_dt)
        self.rows_taken = [[] for _ in range(self.R)]   # the table rows of the last call's outputs

    def reset_row(self, r, frac=None):
        """A fresh node behind row r (frac: a new ratio)."""
        if frac is not None:
            assert FRAC_MIN <= f32(frac) <= FRAC_MAX
            self.frac[r] = frac
        self.mu[r], self.line[r] = 0, 0

    def reset(self):
        for r in range(self.R):
            self.reset_row(r)

    def out_capacity(self, n):
        return out_capacity(self.frac, n)

    def state(self):
        """-> (mu bit patterns [rows] uint32, line [rows, 8(, 2)] of the output type)"""
        return self.mu.view(np.uint32).copy(), self.line.copy()

    def process(self, x):
        """x: [rows, n(, 2)] of the input type -> the list of the rows' output arrays"""
        x = np.asarray(x)
        if x.ndim == (2 if self.iq else 1):
            x = x[None]
        assert x.shape[0] == self.R and x.dtype == IN_DT[self.dtype], (x.shape, x.dtype)
        n = x.shape[1]
        out = [None] * self.R
        groups = {}
        for r in range(self.R):
            if self.frac[r] == f32(1):     # the reference's short cut: the samples are forwarded, the state is left alone
                out[r] = x[r].astype(self.out_dt)
                self.rows_taken[r] = []
            else:
                groups.setdefault((_bits(self.frac[r]), _bits(self.mu[r])), []).append(r)
        for (fb, mb), rs in groups.items():
            pos, rows, mu_bits = _chain(fb, mb, n)
            ext = np.concatenate([self.line[rs], x[rs].astype(self.out_dt)], axis=1)   # [g, 8 + n(, 2)]
            win = ext[:, pos[:, None] + np.arange(8)[None, :]]                          # [g, outs, 8(, 2)]
            y = interp(win, self.tab[rows][None], self.dtype == "i16") if len(pos) else np.zeros((len(rs), 0) + ext.shape[2:], self.out_dt)
            for k, r in enumerate(rs):
                out[r] = y[k]
                self.rows_taken[r] = rows.tolist()
            if n:
                self.line[rs] = ext[:, n:n + 8]
                self.mu[rs] = np.array(mu_bits, np.uint32).view(f32)
        return out
