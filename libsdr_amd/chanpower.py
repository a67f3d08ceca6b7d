"""numpy-facing wrapper over include/sdrhip_chanpower.h (libsdr_amd.abi_chanpower): the channel power monitor — the polyphase
channelizer's arithmetic on ONE antenna row with no rows out: per call M sums of |y_k|^2, per channel a smoothed level and an
open / closed flag with hysteresis. occupied() is the ascending channel list Channelizer.set_channels and
AudioChannelizer.set_channels take."""
import ctypes as C

import numpy as np

from . import abi_chanpower, nodes
from .abi import check
from .channelizer import _Grid
from .nodes import _out, _p

__all__ = ["ChannelPower"]


class ChannelPower(_Grid):
    """sum[k] = sum over a call's outputs of |y_k[m]|^2 in double, y the plain channelizer's values; level[k] follows the calls'
    means with the factor alpha, open[k] follows level[k] between the thresholds (sdrhip_chanpower.h has the contract). dtype,
    M, D, taps: as Channelizer takes them. process(x) returns the call's sums [M] float64; process_dev takes device pointers,
    sum_ptr None or 0 where only the state is wanted."""
    _prefix = "sdrhip_chanpower"
    _calls = ("out_count process process_dev set_thresholds set_alpha set_taps reset get_levels get_occupied get_state plan_info "
              "kernel_names")
    _abi = abi_chanpower
    _create_real = "sdrhip_chanreal_power_create"

    def __init__(self, ctx, dtype, M, D, taps, alpha=0.25, max_in=65536, real=False):
        """real=True: a row [n] of real samples; sums, levels, flags and thresholds have M / 2 + 1 entries (sdrhip_chanreal.h)"""
        super().__init__(ctx, dtype, M, D, taps, max_in, _more=(float(alpha),), real=real)
        self.alpha = float(alpha)

    def process(self, x):
        """One row [n, 2] -> the call's sums [M] float64 (zeros where the call completes no block of D samples)."""
        x = self._rows(x)
        n = x.shape[1]
        no = self.out_count(n)
        out = np.zeros((1, self.n_channels), np.float64)   # (one row of doubles, one per channel: what the router guards)
        if nodes.device_router is not None and n:
            nodes.device_router(self.ctx, x, out, lambda i, si, o, so: self._dev_checked(i, n, o, no))
        else:
            assert _out(C.c_size_t, self._c_process, self._h, *self._host_in(x, n), _p(out, True)) == no
        return out[0]

    def _dev_checked(self, i, n, o, no):
        assert self.process_dev(i, n, o) == no

    def process_dev(self, in_ptr, n, sum_ptr=None):
        """Device pointers; two launches, nothing is synchronised -> the outputs per channel the call took in."""
        return _out(C.c_size_t, self._c_process_dev, self._h, C.c_void_p(in_ptr), n, C.c_void_p(sum_ptr) if sum_ptr else None)

    def set_thresholds(self, open, close):
        """open, close: [M] each, or scalars for every channel; 0 <= close <= open. The flags move with the next call."""
        o, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (self.n_channels,))) for v in (open, close))
        check(self._c_set_thresholds(self._h, _p(o, True), _p(c, True)))

    def set_alpha(self, alpha):
        check(self._c_set_alpha(self._h, float(alpha)))
        self.alpha = float(alpha)

    def levels(self):
        """-> (level [M] float64, open [M] bool) behind the calls enqueued so far"""
        level, flags = np.zeros(self.n_channels, np.float64), np.zeros(self.n_channels, np.uint8)
        check(self._c_get_levels(self._h, _p(level, True), _p(flags, True), self.n_channels))
        return level, flags.astype(bool)

    def occupied(self):
        """-> the open channels, ascending: what set_channels of the two channelizers takes (where it is not empty)"""
        idx, count = np.zeros(self.n_channels, np.intc), C.c_int(0)
        check(self._c_get_occupied(self._h, _p(idx, True), self.n_channels, C.byref(count)))
        return [int(k) for k in idx[:count.value]]

    def get_state(self):
        """-> {consumed, tail (as Channelizer.get_state), calls: the calls that completed an output since create or reset}"""
        calls = C.c_uint64(0)
        consumed, tail = self._tail_state(C.byref(calls))
        return {"consumed": consumed, "tail": tail, "calls": calls.value}

    def plan_info(self):
        """{tile_times, branch_taps, lds_bytes, grid, partial_bytes} of a launch (sdrhip_chanpower_plan_info)"""
        return self._plan_info("tile_times", "branch_taps", "lds_bytes", "grid", "partial_bytes")
