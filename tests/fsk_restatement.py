"""CPU restatement of the reference's FSKDetector, ASKDetector<int16_t> and BitStream (reference src/fsk.cc:19-202,
src/fsk.hh:69-118) in numpy — TEST CODE, the second oracle of the symbol path next to the g18 fixtures (oracle/ is frozen).

Every class carries `channels` independent node instances that receive the same number of samples per call, like the
product's handles. Arithmetic follows the reference operation for operation: float32 products and float32 adds in ring-SLOT
order for the detector (numpy float32 arithmetic is IEEE, unfused), float32 phase / rate with float64 corrections for the
bit PLL. The LUT is an input (a different libm must not move a symbol); `fsk_lut` restates the designer for shapes without
a fixture, using the math library's float sine and cosine through numpy.
"""
import math

import numpy as np

NORMAL, TRANSITION = 0, 1


def corr_len(Fs, baud):
    """int(Fs / baud) with baud a float member (src/fsk.cc:32,122)."""
    return int(float(Fs) / float(np.float32(baud)))


class FSKDetector:
    """mark_lut, space_lut: [L, 2] float32 (re, im)."""

    def __init__(self, mark_lut, space_lut, channels=1):
        self.m = np.ascontiguousarray(mark_lut, np.float32).reshape(-1, 2)
        self.s = np.ascontiguousarray(space_lut, np.float32).reshape(-1, 2)
        self.L, self.C = self.m.shape[0], channels
        self.reset()

    def reset(self):
        # the ring as absolute history: the last L - 1 samples (zeros: a slot never written holds 0) and the index mod L
        self.hist = np.zeros((self.C, self.L - 1), np.int16)
        self.t = 0

    def process(self, x):
        x = np.ascontiguousarray(x, np.int16).reshape(self.C, -1)
        n, L = x.shape[1], self.L
        if n == 0:
            return np.zeros((self.C, 0), np.uint8)
        H = L - 1
        ext = np.concatenate([self.hist, x], axis=1).astype(np.float32)       # sample j of the call sits at column j + H
        lidx = (self.t + np.arange(-H, n)) % L                                # its LUT slot
        P = [ext * self.m[lidx, 0], ext * self.m[lidx, 1], ext * self.s[lidx, 0], ext * self.s[lidx, 1]]   # :70-71
        i = np.arange(n)
        p = (self.t + i) % L
        base = i + H - p                                                      # column of slot 0
        acc = [np.zeros((self.C, n), np.float32) for _ in range(4)]
        for slot in range(L):                                                 # :75-79, slot order
            col = base + slot - np.where(slot > p, L, 0)
            for k in range(4):
                acc[k] = acc[k] + P[k][:, col]
        mr, mi, sr, si = acc
        f = mr * mr + mi * mi - sr * sr - si * si                             # :81-84, float32, left to right
        self.hist = np.concatenate([self.hist, x], axis=1)[:, n:n + H] if H else self.hist
        self.t = (self.t + n) % L
        return (f > 0).astype(np.uint8)


def ask_detect(x, invert=False):
    """(x > 0) ^ invert (src/fsk.hh:108)."""
    return ((np.asarray(x, np.int16) > 0) ^ bool(invert)).astype(np.uint8)


class BitStream:
    def __init__(self, Fs, baud, mode=TRANSITION, channels=1):
        self.Fs, self.baud, self.mode, self.C = float(Fs), np.float32(baud), mode, channels
        self.L = corr_len(Fs, baud)
        self.reset()

    def reset(self):
        C = self.C
        self.phase = np.zeros(C, np.float32)
        om = np.float32(float(self.baud) / self.Fs)                               # :127
        self.omega = np.full(C, om, np.float32)
        self.omin = np.float32(float(om) - 0.005 * float(om))                     # :129
        self.omax = np.float32(float(om) + 0.005 * float(om))                     # :130
        self.gain = np.float32(0.0005)                                            # :132
        self.ring = np.zeros((C, self.L), np.int32)
        self.idx = 0
        self.sym_sum = np.zeros(C, np.int32)
        self.last_bits = np.zeros(C, np.uint8)

    def capacity(self, n):
        return int(math.ceil(n * float(self.omax))) + 1

    def process(self, sym):
        """sym: [channels, n] -> list of the channels' bit arrays."""
        sym = np.ascontiguousarray(sym, np.uint8).reshape(self.C, -1)
        out = [[] for _ in range(self.C)]
        g = float(self.gain)
        one = np.float32(1)
        for i in range(sym.shape[1]):
            last = self.sym_sum.copy()                                            # :164
            v = np.where(sym[:, i] != 0, 1, -1).astype(np.int32)
            self.sym_sum = self.sym_sum - self.ring[:, self.idx] + v              # :165-167
            self.ring[:, self.idx] = v
            self.idx = (self.idx + 1) % self.L
            self.phase = self.phase + self.omega                                  # :171, float32
            emit = self.phase >= one
            if emit.any():
                while True:                                                       # :176
                    over = self.phase >= one
                    if not over.any():
                        break
                    self.phase = np.where(over, self.phase - one, self.phase)
                vote = (self.sym_sum > 0).astype(np.uint8)
                nb = ((self.last_bits << 1) | vote).astype(np.uint8)              # :178
                self.last_bits = np.where(emit, nb, self.last_bits)
                lb = self.last_bits
                bit = ((lb ^ (lb >> 1) ^ 1) & 1) if self.mode == TRANSITION else (lb & 1)   # :180-186
                for c in np.flatnonzero(emit):
                    out[c].append(int(bit[c]))
            tr = ((last < 0) & (self.sym_sum >= 0)) | ((last >= 0) & (self.sym_sum < 0))   # :190
            if tr.any():
                ph, om = self.phase.astype(np.float64), self.omega.astype(np.float64)
                up = (om + g * (0.5 - ph)).astype(np.float32)                     # :193, double, narrowed by the assignment
                dn = (om - g * (ph - 0.5)).astype(np.float32)                     # :195
                new = np.where(ph < 0.5, up, dn)
                new = np.where(self.omin < new, new, self.omin)                   # std::max(_omegaMin, _omega)
                new = np.where(new < self.omax, new, self.omax)                   # std::min(_omegaMax, .)
                self.omega = np.where(tr, new, self.omega).astype(np.float32)
        return [np.array(o, np.uint8) for o in out]


def fsk_lut(Fs, baud, freq):
    """FSKDetector::config's LUT (src/fsk.cc:39-44); the product's designer is pinned against the fixtures, this one serves
    shapes without a fixture only where both sides of a comparison take the same array."""
    L = corr_len(Fs, baud)
    lut = np.zeros((L, 2), np.float32)
    phi = 0.0
    for i in range(L):
        a = np.float32(phi)
        lut[i] = (np.cos(a, dtype=np.float32), np.sin(a, dtype=np.float32))
        phi += (2.0 * math.pi * float(np.float32(freq))) / float(Fs)
    return lut
