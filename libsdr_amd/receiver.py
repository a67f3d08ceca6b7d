"""numpy-facing wrappers over include/sdrhip_rx.h (libsdr_amd.abi_rx): the per-channel FMDeemph and the receiver bank — the
Python mirror of sdr::gpu::ReceiverBank<int16_t> (include/sdr/gpu/receiver.hh), used by the tests and tools/bench_receiver.py.
The component wrappers are libsdr_amd.nodes'."""
import ctypes as C

import numpy as np

from . import abi_rx, nodes
from .abi import check
from .nodes import _Handle, _out, _p

__all__ = ["FMDeemphBankI16", "ReceiverBank"]


class FMDeemphBankI16(nodes.FMDeemphI16):
    """FMDeemph<int16_t> PER CHANNEL at one alpha (sdrhip_deemphbank_i16_create): enabled[c] false is the reference node after
    enable(false), a pass-through whose average rests. process, process_dev, kernel_names and reset are the parent's."""

    def __init__(self, ctx, alpha, enabled, max_in=65536):
        nodes._Node.__init__(self)
        L = abi_rx.lib()
        self._c_set_enabled, self._c_get_enabled = L.sdrhip_deemphbank_i16_set_enabled, L.sdrhip_deemphbank_i16_get_enabled
        en = np.ascontiguousarray(np.asarray(enabled, bool), np.intc).ravel()
        self.ctx, self.channels = ctx, int(en.size)
        check(L.sdrhip_deemphbank_i16_create(ctx.handle, alpha, _p(en, True), self.channels, max_in, C.byref(self._h)))

    def set_enabled(self, c, enabled):
        """enable(bool) of row c, behind the calls already enqueued; the other rows stream on."""
        check(self._c_set_enabled(self._h, int(c), int(bool(enabled))))

    def enabled(self):
        e = (C.c_int * self.channels)()
        check(self._c_get_enabled(self._h, e, self.channels))
        return [bool(v) for v in e]


class ReceiverBank(_Handle):
    """One antenna buffer to every channel's bits on the device (sdrhip_rxbank_create): tuner bank -> de-emphasis -> detector ->
    bit stream. The components are wrappers the caller made and keeps: their setters and resets are the way to change the
    running receiver between two calls. The bank holds references to them and closes before them. The bit stream's sample
    rate has to be the tuner's output rate."""

    def __init__(self, ctx, tuner, detector, bits, deemph=None):
        L = abi_rx.lib()
        self._h = C.c_void_p()
        self._c_sizes, self._c_process, self._c_process_dev, self._c_destroy = (
            L.sdrhip_rxbank_sizes, L.sdrhip_rxbank_process, L.sdrhip_rxbank_process_dev, L.sdrhip_rxbank_destroy)
        self.ctx, self.tuner, self.deemph, self.detector, self.bits = ctx, tuner, deemph, detector, bits
        self.channels = tuner.channels
        check(L.sdrhip_rxbank_create(ctx.handle, tuner._h, deemph._h if deemph is not None else None, detector._h, bits._h,
                                     C.byref(self._h)))

    def _release(self):
        self._c_destroy(self._h)

    def sizes(self, n_in):
        """-> (n_audio, bits_cap) of the next call of n_in samples; the state does not move."""
        na, cap = C.c_size_t(0), C.c_size_t(0)
        check(self._c_sizes(self._h, n_in, C.byref(na), C.byref(cap)))
        return na.value, cap.value

    def process_dev(self, in_ptr, n_in, bits_ptr, bits_stride, counts_ptr, audio_ptr=0, audio_stride=0):
        """Device pointers in, -> n_audio; bits / counts / audio as sdrhip_rxbank_process_dev leaves them."""
        return _out(C.c_size_t, self._c_process_dev, self._h, C.c_void_p(in_ptr), n_in, C.c_void_p(bits_ptr), bits_stride,
                    C.c_void_p(counts_ptr), C.c_void_p(audio_ptr) if audio_ptr else None, audio_stride)

    def process_raw(self, x, audio=True):
        """-> (bits [C, bits_cap] uint8, counts [C] uint32, audio [C, n_audio] int16 or None)"""
        x = self.tuner._rows(x)[0]
        n_in = x.shape[0]
        na, cap = self.sizes(n_in)
        bits, counts = np.zeros((self.channels, cap), np.uint8), np.zeros(self.channels, np.uint32)
        aud = np.zeros((self.channels, na), np.int16) if audio else None
        got = _out(C.c_size_t, self._c_process, self._h, _p(x), n_in, _p(bits), cap, _p(counts), _p(aud) if audio else None, na)
        assert got == na, (got, na)
        return bits, counts, aud

    def process(self, x):
        """x: ONE antenna row as the tuner takes it -> (the list of the channels' bit arrays, audio [C, n_audio])"""
        bits, counts, aud = self.process_raw(x)
        return [bits[c, :counts[c]].copy() for c in range(self.channels)], aud
