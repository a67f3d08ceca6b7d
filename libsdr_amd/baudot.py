"""numpy-facing wrappers over include/sdrhip_baudot.h (libsdr_amd.abi_baudot): the Baudot decoder bank — the Python mirror of
sdr::gpu::Baudot and sdr::gpu::BaudotBank (include/sdr/gpu/baudot.hh). The reference's Baudot node per row, all rows in one
launch: the half-bit rows of a BitStreamBank or a ReceiverBank in (an RTTY channel: 90.90 half-bits per second), text out."""
import ctypes as C

import numpy as np

from . import abi_baudot, nodes
from .abi import E_SIZE, SdrHipError, check
from .abi_baudot import STOP1, STOP15, STOP2, LETTERS, FIGURES
from .nodes import _Node, _p, _text

__all__ = ["Baudot", "BaudotBank", "STOP1", "STOP15", "STOP2", "LETTERS", "FIGURES"]


class BaudotBank(_Node):
    """A Baudot node PER ROW (sdrhip_baudotbank_create): stops[c] is row c's stop-bit setting (STOP1, STOP15, STOP2), enabled[c]
    whether the row decodes. process(bits, counts) takes host rows; process_dev takes the device rows and counts
    sdrhip_bits_process_dev or ReceiverBank.process_dev left, with no host copy in between."""
    _prefix = "sdrhip_baudot"
    _calls = ("out_capacity process process_dev set_channel set_enabled get_channels reset reset_channel channel_state "
              "set_channel_state kernel_names")
    _in, _assert_channels = (np.uint8, 0), True

    def __init__(self, ctx, stops, max_bits, enabled=None):
        stops = np.ascontiguousarray(stops, np.intc).ravel()
        self._setup(ctx, int(stops.size), max_bits)
        en = None if enabled is None else np.ascontiguousarray(np.asarray(enabled, bool), np.intc).ravel()
        assert en is None or en.size == self.channels, (en.size, self.channels)
        check(abi_baudot.lib().sdrhip_baudotbank_create(ctx.handle, _p(stops, True), None if en is None else _p(en, True), self.channels,
                                                       self.max_bits, C.byref(self._h)))

    def _setup(self, ctx, channels, max_bits):
        abi_baudot.lib()
        _Node.__init__(self)
        self.ctx, self.channels, self.max_bits, self._side = ctx, int(channels), int(max_bits), 0
        self._last = None

    def out_capacity(self, n_bits=None):
        """The characters a row of n_bits half-bits (default max_bits: the smallest text-row stride) can leave."""
        return int(self._c_out_capacity(self.max_bits if n_bits is None else n_bits))

    def process_dev(self, bits_ptr, bits_stride, counts_ptr, text_ptr, text_stride, out_counts_ptr, status_ptr=0):
        """Device pointers; text / out_counts / status as sdrhip_baudot_process_dev leaves them. Nothing is synchronised."""
        check(self._c_process_dev(self._h, C.c_void_p(bits_ptr), bits_stride, C.c_void_p(counts_ptr), C.c_void_p(text_ptr), text_stride,
                                  C.c_void_p(out_counts_ptr), C.c_void_p(status_ptr) if status_ptr else None))

    def process(self, bits, counts):
        """bits [channels, stride] uint8, counts [channels] -> (text [channels, capacity] uint8, out_counts [channels] uint32).
        A count above max_bits raises SdrHipError(E_SIZE). With nodes.device_router set the rows go through it and
        process_dev; the counts, the output counts and the status word then pass through a device buffer of the node's own."""
        bits = self._rows(np.ascontiguousarray(bits, np.uint8).reshape(self.channels, -1))
        counts = np.ascontiguousarray(counts, np.uint32)
        assert counts.shape == (self.channels,)
        cap = self.out_capacity()
        text, outc = np.zeros((self.channels, cap), np.uint8), np.zeros(self.channels, np.uint32)
        if nodes.device_router is not None and bits.shape[1]:
            Cn = self.channels
            if not self._side:
                self._side = self.ctx.malloc(8 * Cn + 4)
            side = self._side
            self.ctx.h2d(side, counts)
            nodes.device_router(self.ctx, bits, text, lambda i, si, o, so: self.process_dev(i, si, side, o, so, side + 4 * Cn, side + 8 * Cn))
            back = np.zeros(Cn + 1, np.uint32)
            self.ctx.d2h(back, side + 4 * Cn)
            outc[:] = back[:Cn]
            self._last = (text, outc)
            if back[Cn]:
                raise SdrHipError(E_SIZE, "a row's count exceeds max_bits %d: clamped" % self.max_bits)
            return text, outc
        self._last = (text, outc)
        check(self._c_process(self._h, _p(bits), bits.shape[1], _p(counts), _p(text), cap, _p(outc)))
        return text, outc

    def text(self, c):
        """What row c left in the last process() call, as bytes."""
        assert self._last is not None, "no process() call yet"
        text, outc = self._last
        return text[c, :int(outc[c])].tobytes()

    def set_channel(self, c, stop):
        """A freshly constructed node of setting `stop` behind row c; the other rows stream on."""
        check(self._c_set_channel(self._h, int(c), int(stop)))

    def set_enabled(self, c, enabled):
        check(self._c_set_enabled(self._h, int(c), int(bool(enabled))))

    def get_channels(self):
        """-> (stops [channels], enabled [channels] of bool)"""
        s, e = (C.c_int * self.channels)(), (C.c_int * self.channels)()
        check(self._c_get_channels(self._h, s, e, self.channels))
        return list(s), [bool(v) for v in e]

    def reset(self, keep_mode=False):
        """Every row a freshly constructed node; keep_mode: config() on the old nodes — the registers start over, the tables stay."""
        check(self._c_reset(self._h, int(bool(keep_mode))))

    def reset_channel(self, c, keep_mode=False):
        check(self._c_reset_channel(self._h, int(c), int(bool(keep_mode))))

    def channel_state(self, c):
        """-> (bitstream, bitcount, mode) of row c: the reference node's _bitstream, _bitcount, _mode"""
        b, n, m = C.c_uint16(), C.c_uint64(), C.c_int()
        check(self._c_channel_state(self._h, int(c), C.byref(b), C.byref(n), C.byref(m)))
        return b.value, n.value, m.value

    def set_channel_state(self, c, bitstream, bitcount, mode):
        check(self._c_set_channel_state(self._h, int(c), int(bitstream), int(bitcount), int(mode)))

    @property
    def kernel_names(self):
        return _text(self._c_kernel_names, self._h, size=256).split(",")

    def _release(self):
        if self._side:
            self.ctx.free(self._side)
            self._side = 0
        super()._release()


class Baudot(BaudotBank):
    """sdr::Baudot(stop) on `channels` rows with the same setting, every row enabled (sdrhip_baudot_create)."""

    def __init__(self, ctx, channels, max_bits, stop=STOP15):
        self._setup(ctx, channels, max_bits)
        self.stop = int(stop)
        check(abi_baudot.lib().sdrhip_baudot_create(ctx.handle, self.stop, self.channels, self.max_bits, C.byref(self._h)))
