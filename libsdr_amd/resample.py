"""numpy-facing wrappers over include/sdrhip_resample.h (libsdr_amd.abi_resample): the interpolating resampler bank — the
reference's InpolSubSampler<iScalar, oScalar> per row, all rows in one launch: rows at one sample rate in, each row at its own
rate (input rate / frac) out."""
import ctypes as C

import numpy as np

from . import abi_resample
from .abi import check
from .abi_resample import RESAMPLE_F32, RESAMPLE_CF32, RESAMPLE_I16, RESAMPLE_CS16_CF32
from . import nodes
from .nodes import _Node, _TilePlan, _out, _p, _scalar_dtype
from .psk31 import design_inpol_taps

__all__ = ["InpolSubSampler", "InpolSubSamplerBank", "RESAMPLE_F32", "RESAMPLE_CF32", "RESAMPLE_I16", "RESAMPLE_CS16_CF32"]


class InpolSubSamplerBank(_TilePlan, _Node):
    """An InpolSubSampler PER ROW (sdrhip_resamplebank_create): frac[c] is row c's ratio of input to output rate, in
    [0.125, 4096]; a row with frac 1 passes its samples through. dtype: np.float32 or np.int16, the scalar of the input rows;
    iq: complex rows [channels, n, 2]. float -> float, complex float -> complex float, int16 -> int16 (the reference's wrapping
    int16 accumulator), complex int16 -> complex float. table: the [129, 8] interpolation table (default: design_inpol_taps();
    the reference's own, quirks included, for bit parity with it). process(x) returns the list of the rows' output arrays;
    process_dev takes device rows, e.g. a tuner bank's channels."""
    _prefix, _calls = "sdrhip_resample", "out_capacity process process_dev set_channel reset get_state plan_info kernel_names"
    _assert_channels = True

    def __init__(self, ctx, dtype, frac, iq=False, table=None, max_in=65536):
        frac = np.ascontiguousarray(frac, np.float32).ravel()
        self._setup(ctx, dtype, iq, int(frac.size), table, max_in)
        check(abi_resample.lib().sdrhip_resamplebank_create(ctx.handle, self.dtype, _p(frac, True), _p(self.table, True), self.channels,
                                                            self.max_in, C.byref(self._h)))

    def _setup(self, ctx, dtype, iq, channels, table, max_in):
        abi_resample.lib()
        _Node.__init__(self)
        if isinstance(dtype, int):
            assert dtype in (RESAMPLE_F32, RESAMPLE_CF32, RESAMPLE_I16, RESAMPLE_CS16_CF32), dtype
            self.dtype = dtype
        else:
            self.dtype = _scalar_dtype(dtype, RESAMPLE_CS16_CF32 if iq else RESAMPLE_I16, RESAMPLE_CF32 if iq else RESAMPLE_F32)
        self.iq = self.dtype in (RESAMPLE_CF32, RESAMPLE_CS16_CF32)
        self._in = (np.int16 if self.dtype in (RESAMPLE_I16, RESAMPLE_CS16_CF32) else np.float32, 2 if self.iq else 0)
        self.out_dtype = np.int16 if self.dtype == RESAMPLE_I16 else np.float32
        self.table = np.ascontiguousarray(design_inpol_taps() if table is None else table, np.float32).reshape(129, 8)
        self.ctx, self.channels, self.max_in, self._counts_dev = ctx, int(channels), int(max_in), 0

    def out_capacity(self, n):
        """The most outputs a row writes in a call of n samples: the smallest output-row stride."""
        return _out(C.c_size_t, self._c_out_capacity, self._h, n)

    def process_raw(self, x):
        """-> (out [channels, capacity(n)(, 2)] of the output type, counts [channels] uint32)"""
        x = self._rows(x)
        n = x.shape[1]
        cap = self.out_capacity(n)
        out = np.zeros((self.channels, cap, 2) if self.iq else (self.channels, cap), self.out_dtype)
        counts = np.zeros(self.channels, np.uint32)
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

    def process_dev(self, in_ptr, n, in_stride, out_ptr, out_stride, counts_ptr):
        """Device pointers, strides in input / output elements; one launch, nothing is synchronised."""
        check(self._c_process_dev(self._h, C.c_void_p(in_ptr), n, in_stride, C.c_void_p(out_ptr), out_stride, C.c_void_p(counts_ptr)))

    def set_channel(self, c, frac):
        """A fresh node with this frac behind row c; the other rows stream on."""
        check(self._c_set_channel(self._h, int(c), float(frac)))

    def reset(self):
        check(self._c_reset(self._h))

    def get_state(self):
        """-> dict of frac, mu (float32 [channels]) and line ([channels, 8(, 2)] of the output type, oldest first) behind the
        calls enqueued so far"""
        frac, mu = np.zeros(self.channels, np.float32), np.zeros(self.channels, np.float32)
        line = np.zeros((self.channels, 8, 2) if self.iq else (self.channels, 8), self.out_dtype)
        i16 = self.dtype == RESAMPLE_I16
        check(self._c_get_state(self._h, _p(frac, True), _p(mu, True), None if i16 else _p(line, True), _p(line, True) if i16 else None,
                                self.channels))
        return {"frac": frac, "mu": mu, "line": line}

    def _release(self):
        if self._counts_dev:
            self.ctx.free(self._counts_dev)
            self._counts_dev = 0
        super()._release()


class InpolSubSampler(InpolSubSamplerBank):
    """sdr::InpolSubSampler<iScalar, oScalar>(frac) on `channels` rows with the same frac (sdrhip_resample_create)."""

    def __init__(self, ctx, dtype, frac, iq=False, channels=1, table=None, max_in=65536):
        self._setup(ctx, dtype, iq, channels, table, max_in)
        self.frac = float(np.float32(frac))
        check(abi_resample.lib().sdrhip_resample_create(ctx.handle, self.dtype, self.frac, _p(self.table, True), self.channels, self.max_in,
                                                        C.byref(self._h)))
