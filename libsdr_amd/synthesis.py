"""numpy-facing wrapper over include/sdrhip_synthesis.h (libsdr_amd.abi_synthesis): the polyphase synthesis bank — complex float
channel rows, as Channelizer.process_dev leaves them and the AGC, resampler and BPSK31 banks take and return them, onto ONE
wideband complex row interpolated by D. The channelizer's mirror: a synthesis row fed to a Channelizer of the same M comes back on
the same channel index."""
import ctypes as C

import numpy as np

from . import abi_synthesis, nodes
from .abi import check
from .channelizer import _Grid
from .nodes import _Counted, _out, _p, _rows

__all__ = ["Synthesis"]


class Synthesis(_Grid):
    """z[t] = sum_k sum_m c_k[m] g[t - m D] exp(+2 pi i k t / M) (sdrhip_synthesis.h has the contract). taps: the prototype
    low-pass as doubles (rounded once to float32), at most 64 D of them; channels: the channel each input row belongs to, any
    order, no duplicates (None: all M in order) — channels not listed carry zero. process(x) takes [rows, n, 2] float32 and
    returns the wideband row [n D, 2] float32; process_dev takes device pointers. Of _Grid it has the setters, plan_info's form
    and kernel_names; its create call has no input type and its input is rows, not one row."""
    _prefix = "sdrhip_synthesis"
    _calls = "out_count process process_dev set_channels set_taps reset get_state plan_info kernel_names"
    _in, _assert_channels, _out_dtype = (np.float32, 2), True, np.float32
    _abi = abi_synthesis

    def __init__(self, ctx, M, D, taps, channels=None, max_in=65536):
        self._abi.lib()
        _Counted.__init__(self)
        taps = np.ascontiguousarray(taps, np.float64).ravel()
        self.ctx, self.M, self.D, self.n_taps, self.max_in = ctx, int(M), int(D), int(taps.size), int(max_in)
        self.Q = -(-self.n_taps // max(self.D, 1))
        self.n_channels = self.M
        self.selected, self.channels = list(range(self.M)), self.M
        check(self._abi.lib().sdrhip_synthesis_create(ctx.handle, self.M, self.D, _p(taps, True), self.n_taps, self.max_in, C.byref(self._h)))
        if channels is not None:
            self.set_channels(channels)

    def _rows(self, x):
        return _rows(x, *self._in, self.channels)

    def process(self, x):
        """x: [rows, n, 2] float32, row i on channel selected[i] -> [n D, 2] float32"""
        x = self._rows(x)
        n = x.shape[1]
        no = self.out_count(n)
        out = np.zeros((1, no, 2), np.float32)
        if nodes.device_router is not None and n:
            nodes.device_router(self.ctx, x, out, lambda i, si, o, so: self._dev_checked(i, n, si, o, so, no))
        else:
            assert _out(C.c_size_t, self._c_process, self._h, _p(x), n, n, _p(out)) == no
        return out[0]

    def _dev_checked(self, i, n, si, o, so, no):
        assert self.process_dev(i, n, si, o) == no

    def process_dev(self, in_ptr, n, in_stride, out_ptr):
        """Device pointers, in_stride in complex elements (0: n); two launches, nothing is synchronised -> the outputs written."""
        return _out(C.c_size_t, self._c_process_dev, self._h, C.c_void_p(in_ptr), n, in_stride, C.c_void_p(out_ptr))

    def set_channels(self, channels):
        """Row i of the later calls belongs to channels[i] (None: all M in order); the stream itself goes on."""
        if channels is None:
            check(self._c_set_channels(self._h, None, 0))
            self.selected = list(range(self.M))
        else:
            idx = np.ascontiguousarray(channels, np.intc).ravel()
            check(self._c_set_channels(self._h, _p(idx, True), int(idx.size)))
            self.selected = [int(k) for k in idx]
        self.channels = len(self.selected)

    def get_state(self):
        """-> {consumed: columns taken since create or reset, cols: the last Q - 1 transformed columns [Q - 1, M, 2] float32,
        oldest first} behind the calls enqueued so far"""
        consumed, cols = C.c_uint64(0), np.zeros((self.Q - 1, self.M, 2), np.float32)
        check(self._c_get_state(self._h, C.byref(consumed), _p(cols, True), (self.Q - 1) * self.M))
        return {"consumed": consumed.value, "cols": cols}

    def plan_info(self):
        """{tile_times, branch_taps, lds_bytes, rows} of a call's launches (sdrhip_synthesis_plan_info)"""
        return self._plan_info("tile_times", "branch_taps", "lds_bytes", "rows")
