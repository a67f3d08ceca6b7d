"""numpy-facing wrappers over include/sdrhip_agc.h (libsdr_amd.abi_agc): the AGC bank — the Python mirror of sdr::gpu::AGC and
sdr::gpu::AGCBank (include/sdr/gpu/agc.hh). AGC<int16_t> / AGC<float> of the reference per row, all rows in one launch; both
classes belong to the equal-length family of nodes.py, so process(x) meets nodes.device_router like every other node's."""
import ctypes as C

import numpy as np

from . import abi_agc
from .abi import check
from .abi_agc import AGC_I16, AGC_F32
from .nodes import _EqualLength, _TilePlan, _out, _p, _scalar_dtype

__all__ = ["AGC", "AGCBank", "design_agc_lambda", "design_agc_target", "AGC_I16", "AGC_F32"]


def design_agc_lambda(tau, Fs):
    """The per-sample decay of AGC(tau) at sample rate Fs, as the reference's config() computes it (a float)."""
    return _out(C.c_float, abi_agc.lib().sdrhip_design_agc_lambda, tau, Fs)


def design_agc_target(dtype):
    """The target of AGC(tau, 0): 16000 for int16 rows, 0.5 for float rows."""
    return _out(C.c_float, abi_agc.lib().sdrhip_design_agc_target, _dtype(dtype))


def _dtype(dtype):
    return _scalar_dtype(dtype, AGC_I16, AGC_F32)


class AGCBank(_TilePlan, _EqualLength):
    """An AGC node PER ROW (sdrhip_agcbank_create): lam[c] (design_agc_lambda), target[c] (0: the type's default) and
    enabled[c]. dtype: np.int16 or np.float32. The setters replace or adjust the node behind one row between two calls."""
    _prefix, _calls = "sdrhip_agc", "process process_dev set_channel set_lambda set_enabled set_gain get_state plan_info kernel_names reset"
    _assert_channels = True

    def __init__(self, ctx, dtype, lam, target=None, enabled=None, max_in=65536):
        abi_agc.lib()
        super().__init__()
        self.dtype = _dtype(dtype)
        self._in = (np.int16 if self.dtype == AGC_I16 else np.float32, 0)
        lam = np.ascontiguousarray(lam, np.float32).ravel()
        self.ctx, self.channels, self.max_in = ctx, int(lam.size), int(max_in)
        target = self._targets(target, self.channels)
        en = np.ascontiguousarray(np.ones(self.channels, bool) if enabled is None else np.asarray(enabled, bool), np.intc).ravel()
        assert target.size == self.channels and en.size == self.channels, (target.size, en.size, self.channels)
        check(abi_agc.lib().sdrhip_agcbank_create(ctx.handle, self.dtype, _p(lam, True), _p(target, True), _p(en, True), self.channels,
                                                  self.max_in, C.byref(self._h)))

    def _targets(self, target, n):
        t = np.zeros(n, np.float32) if target is None else np.ascontiguousarray(np.broadcast_to(np.asarray(target, np.float32), (n,)))
        t = t.copy()
        if np.any(t == 0):
            t[t == 0] = design_agc_target(self.dtype)
        return t

    def process(self, x):
        x = self._rows(x)
        return self._run(x, np.zeros_like(x))

    def set_channel(self, c, lam, target=0.0):
        """A fresh node behind row c: sd = target, gain = 1, enabled; the other rows stream on."""
        check(self._c_set_channel(self._h, int(c), float(lam), float(self._targets(target, 1)[0])))

    def set_lambda(self, c, lam):
        """setTau of row c's node: the decay only, the state goes on."""
        check(self._c_set_lambda(self._h, int(c), float(lam)))

    def set_enabled(self, c, enabled):
        check(self._c_set_enabled(self._h, int(c), int(bool(enabled))))

    def set_gain(self, c, gain):
        check(self._c_set_gain(self._h, int(c), float(gain)))

    def get_state(self):
        """-> (gain [channels] float32, sd [channels] float32, enabled [channels] bool) behind the calls enqueued so far.
        sd of an AM or USB row is that row's signal level."""
        g, s, e = np.zeros(self.channels, np.float32), np.zeros(self.channels, np.float32), np.zeros(self.channels, np.intc)
        check(self._c_get_state(self._h, _p(g, True), _p(s, True), _p(e, True), self.channels))
        return g, s, e.astype(bool)


class AGC(AGCBank):
    """sdr::AGC<Scalar>(tau, target) at sample rate Fs on `channels` rows with equal parameters (sdrhip_agc_create)."""

    def __init__(self, ctx, dtype, Fs, tau=0.1, target=0.0, channels=1, max_in=65536):
        abi_agc.lib()
        _EqualLength.__init__(self)
        self.dtype = _dtype(dtype)
        self._in = (np.int16 if self.dtype == AGC_I16 else np.float32, 0)
        self.ctx, self.channels, self.max_in, self.Fs, self.tau = ctx, int(channels), int(max_in), float(Fs), float(tau)
        self.lam = design_agc_lambda(tau, Fs)
        self.target = float(self._targets(target, 1)[0])
        check(abi_agc.lib().sdrhip_agc_create(ctx.handle, self.dtype, self.lam, self.target, self.channels, self.max_in, C.byref(self._h)))

    def set_tau(self, tau, c=None):
        """setTau on row c (default: every row)."""
        self.tau, self.lam = float(tau), design_agc_lambda(tau, self.Fs)
        for k in (range(self.channels) if c is None else [c]):
            self.set_lambda(k, self.lam)
