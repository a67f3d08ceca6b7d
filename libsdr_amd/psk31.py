"""numpy-facing wrappers over include/sdrhip_psk31.h (libsdr_amd.abi_psk31): the BPSK31 bank — the reference's
BPSK31<int16_t> / BPSK31<float> per row, all rows in one launch: complex baseband rows in, each row's 31.25 baud bit stream
out — and the host half of a PSK31 receiver: Varicode turns the bit rows into text, one shift register per row carried across
calls (as MessageAssembler does for POCSAG)."""
import ctypes as C

import numpy as np

from . import abi_psk31
from .abi import check
from .abi_psk31 import PSK31_CS16, PSK31_CF32
from . import nodes
from .nodes import _Node, _TilePlan, _designed, _out, _p, _scalar_dtype

__all__ = ["BPSK31", "BPSK31Bank", "Varicode", "design_inpol_taps", "PSK31_CS16", "PSK31_CF32"]


def design_inpol_taps():
    """The library's own interpolation table [129, 8] float32: least-squares fractional-delay filters (sdrhip_psk31.h)."""
    return _designed(abi_psk31.lib().sdrhip_design_inpol_taps, (129, 8), np.float32)


class BPSK31Bank(_TilePlan, _Node):
    """A BPSK31 node PER ROW at one sample rate Fs (sdrhip_psk31bank_create): dF[c] is row c's carrier-loop range in radians per
    sample. dtype: np.int16 (complex<int16> rows) or np.float32. table: the [129, 8] interpolation table (default:
    design_inpol_taps(); the reference's own, quirks included, for bit parity with it). process(x[channels, n, 2]) returns the
    list of the rows' bit arrays; process_dev takes device rows, e.g. a tuner bank's EPI_NONE channels."""
    _prefix, _calls = "sdrhip_psk31", "out_capacity process process_dev set_channel reset get_state plan_info kernel_names"
    _assert_channels = True

    def __init__(self, ctx, dtype, Fs, dF, table=None, max_in=65536):
        dF = np.ascontiguousarray(dF, np.float32).ravel()
        self._setup(ctx, dtype, Fs, int(dF.size), table, max_in)
        check(abi_psk31.lib().sdrhip_psk31bank_create(ctx.handle, self.dtype, self.Fs, _p(dF, True), _p(self.table, True), self.channels,
                                                      self.max_in, C.byref(self._h)))

    def _setup(self, ctx, dtype, Fs, channels, table, max_in):
        abi_psk31.lib()
        _Node.__init__(self)
        self.dtype = _scalar_dtype(dtype, PSK31_CS16, PSK31_CF32)
        self._in = (np.int16 if self.dtype == PSK31_CS16 else np.float32, 2)
        self.table = np.ascontiguousarray(design_inpol_taps() if table is None else table, np.float32).reshape(129, 8)
        self.ctx, self.Fs, self.channels, self.max_in, self._counts_dev = ctx, float(Fs), int(channels), int(max_in), 0

    def out_capacity(self, n):
        """The most bits a row writes in a call of n samples: the smallest bit-row stride."""
        return _out(C.c_size_t, self._c_out_capacity, self._h, n)

    def process_raw(self, x):
        """-> (bits [channels, capacity(n)] uint8, counts [channels] uint32)"""
        x = self._rows(x)
        n = x.shape[1]
        cap = self.out_capacity(n)
        out, counts = np.zeros((self.channels, cap), np.uint8), np.zeros(self.channels, np.uint32)
        if nodes.device_router is not None and n:   # (the counts go through a device buffer of the node's own, freed in close())
            if not self._counts_dev:
                self._counts_dev = self.ctx.malloc(4 * self.channels)
            nodes.device_router(self.ctx, x, out, lambda i, si, o, so: self.process_dev(i, n, si, o, so, self._counts_dev))
            self.ctx.d2h(counts, self._counts_dev)
            return out, counts
        check(self._c_process(self._h, _p(x), n, n, _p(out), cap, _p(counts)))
        return out, counts

    def process(self, x):
        out, counts = self.process_raw(x)
        return [out[c, :counts[c]].copy() for c in range(self.channels)]

    def process_dev(self, in_ptr, n, in_stride, bits_ptr, out_stride, counts_ptr):
        """Device pointers, strides in complex samples / bytes; one launch, nothing is synchronised."""
        check(self._c_process_dev(self._h, C.c_void_p(in_ptr), n, in_stride, C.c_void_p(bits_ptr), out_stride, C.c_void_p(counts_ptr)))

    def set_channel(self, c, dF):
        """A fresh node with range dF behind row c; the other rows stream on."""
        check(self._c_set_channel(self._h, int(c), float(dF)))

    def reset(self):
        check(self._c_reset(self._h))

    def get_state(self):
        """-> dict of P, F, mu, omega (float32 [channels]) and hist_idx, last (int32 [channels]) behind the calls enqueued so far"""
        f = [np.zeros(self.channels, np.float32) for _ in range(4)]
        i = [np.zeros(self.channels, np.intc) for _ in range(2)]
        check(self._c_get_state(self._h, *[_p(a, True) for a in f + i], self.channels))
        return dict(zip(("P", "F", "mu", "omega", "hist_idx", "last"), f + i))

    def _release(self):
        if self._counts_dev:
            self.ctx.free(self._counts_dev)
            self._counts_dev = 0
        super()._release()


class BPSK31(BPSK31Bank):
    """sdr::BPSK31<Scalar>(dF) at sample rate Fs on `channels` rows with the same dF (sdrhip_psk31_create)."""

    def __init__(self, ctx, dtype, Fs, dF=0.1, channels=1, table=None, max_in=65536):
        self._setup(ctx, dtype, Fs, channels, table, max_in)
        self.dF = float(dF)
        check(abi_psk31.lib().sdrhip_psk31_create(ctx.handle, self.dtype, self.Fs, self.dF, _p(self.table, True), self.channels, self.max_in,
                                                  C.byref(self._h)))


# The Varicode alphabet of PSK31 (G3PLX's published table: every code starts and ends with 1 and holds no 00; 00 separates
# codes), restricted to what the reference's decoder knows and with the values it knows them by: where those differ from the
# published table (its '%', '!' and some digits and brackets do) the reference's value stands, since the bank's text is held
# to the reference's. LF and EOT (1011101011) both decode as '\n'; a code outside the table is dropped.
_CODES = """
\\n 11101  \\n 1011101011  \\r 11111  SP 1  ! 1111111111  " 101011111  # 1111110101  $ 111011011  % 11011010101  & 1010111011
' 1101111111  ) 111110111  * 101101111  + 1111011111  - 1110101  . 1010111  / 1110101111  0 10110111  1 10111101  2 11101101
3 111111111  4 101110111  5 1101011011  6 101101011  7 1110101101  8 110101011  9 1110110111  : 11110101  ; 110111101
< 111101101  = 1010101  > 111010111  ? 1010101111  @ 1010111101  A 1111101  B 11101011  C 10101101  D 10110101  E 1110111
F 11011011  G 11111101  H 101010101  I 1111111  J 111111101  K 101111101  L 11010111  M 10111011  N 11011101  O 10101011
P 11010101  Q 111011101  R 10101111  S 1101111  T 1101101  U 101010111  V 110110101  W 101011101  X 101110101  Y 101111011
Z 1010101101  [ 11111011  \\ 111101111  ] 111111011  ^ 1010111111  _ 101101101  ` 1011011111  a 1011  b 1011111  c 101111
d 101101  e 11  f 111101  g 1011011  h 101011  i 1101  j 111101011  k 10111111  l 11011  m 111011  n 1111  o 111  p 111111
q 110111111  r 10101  s 10111  t 101  u 110111  v 1111011  w 1101011  x 11011111  y 1011101  z 111010101  { 1010110111
| 110111011  } 1010110101  ~ 1011010111
"""
_NAMED = {"\\n": "\n", "\\r": "\r", "SP": " "}


def _table():
    words = _CODES.split()
    return {int(code, 2): _NAMED.get(ch, ch) for ch, code in zip(words[0::2], words[1::2])}


VARICODE = _table()   # code value -> character


class Varicode:
    """The host half of `channels` PSK31 receivers: sdr::Varicode per row. feed(rows) takes each row's bits of one call and
    returns the rows' decoded text; a code cut by the end of a call is finished by the next."""

    def __init__(self, channels=1):
        self.channels = int(channels)
        self._value = [0] * self.channels

    def feed_row(self, c, bits):
        v, out = self._value[c], []
        for b in np.asarray(bits, np.uint8).ravel().tolist():
            v = ((v << 1) | (b & 1)) & 0xFFFF   # (the reference's register is a uint16_t)
            if v & 3 == 0:
                ch = VARICODE.get(v >> 2)
                if ch is not None:
                    out.append(ch)
                v = 0
        self._value[c] = v
        return "".join(out)

    def feed(self, rows):
        assert len(rows) == self.channels, (len(rows), self.channels)
        return [self.feed_row(c, rows[c]) for c in range(self.channels)]

    def reset(self):
        self._value = [0] * self.channels
