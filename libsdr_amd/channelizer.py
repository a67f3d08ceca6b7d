"""numpy-facing wrapper over include/sdrhip_channelizer.h (libsdr_amd.abi_channelizer): the polyphase channelizer — ONE antenna
row to M uniform channels, each 1 / M of the band wide and decimated by D, in one pass; complex float rows out, one per selected
channel, as the resampler, BPSK31 and AGC banks take them through process_dev."""
import ctypes as C

import numpy as np

from . import abi_channelizer, abi_chanreal
from .abi import check
from .abi_channelizer import CHAN_CS16, CHAN_CF32
from .nodes import _Counted, _out, _p, _scalar_dtype, _text

__all__ = ["Channelizer", "CHAN_CS16", "CHAN_CF32"]


class _Grid(_Counted):
    """What the nodes on the channelizer's grid share (Channelizer, AudioChannelizer, libsdr_amd.chanpower.ChannelPower): the
    create call's head (ctx, dtype, M, D, taps, n_taps, max_in, then the node's own arguments, then the handle), ONE input row
    [n, 2] of the scalar type, set_taps and kernel_names. A class names `_prefix`, `_calls` and `_abi`, its side header's binding
    module. real=True (sdrhip_chanreal.h, as TunerBankI16(real=True)): the row is [n] real samples, the handle comes from
    `_create_real`, and the node has the K = M / 2 + 1 channels 0 ... M / 2 — `n_channels` either way."""

    def __init__(self, ctx, dtype, M, D, taps, max_in, _more=(), real=False):
        """_more: what the node's create takes between max_in and the handle"""
        self._abi.lib()
        super().__init__()
        self.dtype = _scalar_dtype(dtype, CHAN_CS16, CHAN_CF32)   # (CHANREAL_S16, CHANREAL_F32 have the same values)
        self.real = bool(real)
        self._in = (np.int16 if self.dtype == CHAN_CS16 else np.float32, 0 if self.real else 2)
        taps = np.ascontiguousarray(taps, np.float64).ravel()
        self.ctx, self.M, self.D, self.n_taps, self.max_in = ctx, int(M), int(D), int(taps.size), int(max_in)
        self.n_channels = self.M // 2 + 1 if self.real else self.M
        self._created()
        create = getattr(abi_chanreal.lib(), self._create_real) if self.real else getattr(self._abi.lib(), self._prefix + "_create")
        check(create(ctx.handle, self.dtype, self.M, self.D, _p(taps, True), self.n_taps, self.max_in, *_more, C.byref(self._h)))

    def _created(self):
        """attributes a class sets before its create call"""

    # process(x) — x: ONE row [n, 2] ([n] of a real node); the router sees it as x[None]; the node's calls take no input stride
    def _rows(self, x):
        x = np.ascontiguousarray(x, self._in[0])
        if self.real:
            assert x.ndim == 1, x.shape
        else:
            assert x.ndim == 2 and x.shape[1] == 2, x.shape
        return x[None]

    def _host_in(self, x, n_in):
        return _p(x[0]), n_in

    def set_taps(self, taps):
        """A new prototype of the same length; the node's state is kept."""
        taps = np.ascontiguousarray(taps, np.float64).ravel()
        assert taps.size == self.n_taps, (taps.size, self.n_taps)
        check(self._c_set_taps(self._h, _p(taps, True)))

    def _tail_state(self, *more):
        """get_state's head: (consumed, tail [n_taps - 1, 2] float32) — `more`: the call's further arguments"""
        consumed, tail = C.c_uint64(0), np.zeros((self.n_taps - 1, 2), np.float32)
        check(self._c_get_state(self._h, C.byref(consumed), _p(tail, True), self.n_taps - 1, *more))
        return consumed.value, tail

    def _plan_info(self, *names):
        v = [C.c_int(0) for _ in names]
        check(self._c_plan_info(self._h, *[C.byref(c) for c in v]))
        return dict(zip(names, [c.value for c in v]))

    @property
    def kernel_names(self):
        return _text(self._c_kernel_names, self._h, size=256).split(",")


class Channelizer(_Grid):
    """y_k[m] = sum_l h[l] x[t_m - l] exp(-2 pi i k (t_m - l) / M), t_m = (m + 1) D - 1 (sdrhip_channelizer.h has the contract).
    dtype: np.int16 or np.float32, the scalar of the complex input row [n, 2]; taps: the prototype low-pass as doubles (rounded
    once to float32); channels: the channels to write, any order, no duplicates (None: all M in order). process(x) returns
    [rows, n_out, 2] float32, row i holding channel selected[i]; process_dev takes device pointers. real=True: the row is [n]
    of int16 or float32 and the channels are 0 ... M / 2 (sdrhip_chanreal.h)."""
    _prefix = "sdrhip_channelizer"
    _calls = "out_count process process_dev set_channels set_taps reset get_state plan_info kernel_names"
    _out_dtype = np.float32
    _abi = abi_channelizer   # the side header's binding module (libsdr_amd.chanaudio has another)
    _create_real = "sdrhip_chanreal_channelizer_create"

    def __init__(self, ctx, dtype, M, D, taps, channels=None, max_in=65536, _more=(), real=False):
        """_more: what a subclass's create takes between max_in and the handle"""
        super().__init__(ctx, dtype, M, D, taps, max_in, _more, real)
        if channels is not None:
            self.set_channels(channels)

    def _created(self):
        self.selected, self.channels = list(range(self.n_channels)), self.n_channels

    def _dev_checked(self, i, n_in, si, o, so, no):
        assert self.process_dev(i, n_in, o, so) == no

    def process_dev(self, in_ptr, n, out_ptr, out_stride):
        """Device pointers, out_stride in complex elements; one launch, nothing is synchronised -> the outputs per row."""
        return _out(C.c_size_t, self._c_process_dev, self._h, C.c_void_p(in_ptr), n, C.c_void_p(out_ptr), out_stride)

    def set_channels(self, channels):
        """Row i of the later calls holds channels[i] (None: all M in order); the stream itself goes on."""
        if channels is None:
            check(self._c_set_channels(self._h, None, 0))
            self.selected = list(range(self.n_channels))
        else:
            idx = np.ascontiguousarray(channels, np.intc).ravel()
            check(self._c_set_channels(self._h, _p(idx, True), int(idx.size)))
            self.selected = [int(k) for k in idx]
        self.channels = len(self.selected)

    def get_state(self):
        """-> {consumed: samples taken since create or reset, tail: the last n_taps - 1 samples [n_taps - 1, 2] float32, oldest
        first} behind the calls enqueued so far"""
        consumed, tail = self._tail_state()
        return {"consumed": consumed, "tail": tail}

    def plan_info(self):
        """{tile_times, branch_taps, lds_bytes, rows} of a launch (sdrhip_channelizer_plan_info)"""
        return self._plan_info("tile_times", "branch_taps", "lds_bytes", "rows")
