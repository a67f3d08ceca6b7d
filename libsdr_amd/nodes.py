"""Thin numpy-facing wrappers over the C ABI (libsdr_amd.abi) — the Python mirror of the C++ nodes in
include/sdr/gpu/*.hh, used by tests/ and bench.py.

Every class maps 1:1 to a handle type of include/sdrhip.h; `process(x)` takes/returns numpy arrays in
the channel-major layout [channels, n, 2] (complex as (re, im)), `process_dev(ptr, ...)` takes raw
device pointers (e.g. torch tensors' data_ptr()). No CPU fallback exists: constructing a Context
without a HIP device raises SdrHipError(E_NODEVICE).

The helper layer, each thing written once: _p (array -> pointer), _out (scalar out-parameter getters), _text (string
getters), _rows (input layout), _scalar_dtype (a bank's int16-or-float code), _roundtrip (host arrays through fresh device
buffers), _Handle (close / __del__ of a handle owner), _Node (entry points bound at construction), the two process families
_Counted and _EqualLength, and _TilePlan (plan_info / kernel_names of the tiled per-row banks).
To add a node: derive from the family its calls belong to, name its `_prefix` and `_calls`, declare its input layout
(`_in`, `_assert_channels`) and its output (`_out_dtype`, or the array it hands to `_run`), then write the constructor around
the create call and whatever else is particular to it. A mistyped entry point fails construction, on any machine
(tests/test_nodes_calls.py drives every wrapper against a fake library).
"""
import ctypes as C

import numpy as np

from . import abi
from .abi import (EPI_NONE, EPI_FM, EPI_AM, EPI_USB, FIR_CS16_EXACT, FIR_CF32, T_CS16, T_CF32, T_CF64,
                  FFTCONV_OLA, FFTCONV_OLS, check)


def _p(a, typed=False):
    """Pointer to a's data: void *, or (typed) a pointer to a's element type, for the ABI's typed parameters."""
    return a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)) if typed else C.c_void_p)


def _out(ctype, fn, *args):
    """fn(*args, &v), checked -> v: the calls whose last parameter is one scalar out-parameter."""
    v = ctype()
    check(fn(*args, C.byref(v)))
    return v.value


def _text(fn, *args, size=0):
    """A string getter: fn(*args, buffer, size) with a buffer of `size` bytes, or (size 0) fn(*args, &const char *)."""
    if not size:
        return _out(C.c_char_p, fn, *args).decode()
    b = C.create_string_buffer(size)
    check(fn(*args, b, size))
    return b.value.decode()


def _split_kernels(text):
    """A *_last_kernels answer -> the list of names: split at the commas outside angle brackets (template arguments)."""
    out, depth, cur = [], 0, ""
    for ch in text:
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return [k for k in out + [cur] if k]


def _rows(x, dtype, comps, channels=None):
    """x as contiguous rows [channels, n, comps] of dtype (comps 0: real rows [channels, n]); one row may come without the
    channel axis. channels: the row count x must have, for the classes that assert it."""
    x = np.ascontiguousarray(x, dtype)
    nd = 3 if comps else 2
    if x.ndim == nd - 1:
        x = x[None]
    assert x.ndim == nd and (not comps or x.shape[2] == comps), x.shape
    assert channels is None or x.shape[0] == channels, x.shape
    return x


def _scalar_dtype(dtype, i16_code, f32_code):
    """The ABI's code of a bank's scalar type: np.int16 or np.float32 (or a dtype alike), or one of the two codes itself."""
    if isinstance(dtype, int):
        assert dtype in (i16_code, f32_code), dtype
        return dtype
    dt = np.dtype(dtype)
    assert dt in (np.dtype(np.int16), np.dtype(np.float32)), dt
    return i16_code if dt == np.int16 else f32_code


def _roundtrip(ctx, x, out, call, staged_out=False):
    """x into a fresh device buffer, call(in_ptr, out_ptr), the other buffer read back into out; both are freed whatever
    happens. staged_out: out's present content goes up first (a call may leave elements alone) and the stream is synchronized
    before the read."""
    din, dout = ctx.malloc(max(x.nbytes, 16)), ctx.malloc(max(out.nbytes, 16))
    try:
        ctx.h2d(din, x)
        if staged_out:
            ctx.h2d(dout, out)
        call(din, dout)
        if staged_out:
            ctx.synchronize()
        ctx.d2h(out, dout)
    finally:
        ctx.free(din)
        ctx.free(dout)
    return out


# ---- designers (host only; identical code to include/sdr/gpu/design.hh) -----------------------

def _designed(fn, shape, dtype, *args):
    """A designer that fills an array: fn(*args, out)."""
    t = np.zeros(shape, dtype)
    check(fn(*args, _p(t, True)))
    return t


def design_iqbb_taps(Ff, width, Fs, order):
    return _designed(abi.lib().sdrhip_design_iqbb_taps, (order, 2), np.int32, Ff, width, Fs, order)


def design_bb_taps(Ff, width, Fs, order):
    """Q16 taps of the real-input BaseBand<int16_t> (reference src/baseband.hh:464-491)."""
    return _designed(abi.lib().sdrhip_design_bb_taps, (order, 2), np.int32, Ff, width, Fs, order)


def design_iqbb_decim(Fs, sub, oFs=0.0):
    return _out(C.c_int, abi.lib().sdrhip_design_iqbb_decim, Fs, sub, oFs)


def design_freqshift_lut_i16():
    return _designed(abi.lib().sdrhip_design_freqshift_lut_i16, (128, 2), np.int32)


def design_freqshift_lut_i8():
    return _designed(abi.lib().sdrhip_design_freqshift_lut_i8, (128, 2), np.int32)


def design_freqshift_inc(F, Fs):
    return _out(C.c_uint32, abi.lib().sdrhip_design_freqshift_inc, F, Fs)


def design_fir_lowpass(order, Fu, Fs):
    return _designed(abi.lib().sdrhip_design_fir_lowpass, order, np.float64, order, Fu, Fs)


def design_fmdeemph_alpha(Fs):
    return _out(C.c_int, abi.lib().sdrhip_design_fmdeemph_alpha, Fs)


def design_fftfilt_kernel(N, fmin, fmax, Fs, dtype=np.float32):
    """sinc_flt_kernel<float> (default) or <double> (dtype=np.float64): N x (re, im)."""
    f64 = np.dtype(dtype) == np.float64
    fn = abi.lib().sdrhip_design_fftfilt_kernel_f64 if f64 else abi.lib().sdrhip_design_fftfilt_kernel
    return _designed(fn, (N, 2), dtype, N, fmin, fmax, Fs)


def design_fftfilt_spectrum(h):
    """FilterSource::_updateFilter: K = DFT_2N([h, 0]) / ||K||; the dtype follows h (float32 unless h is float64)."""
    f64 = np.asarray(h).dtype == np.float64
    h = np.ascontiguousarray(h, np.float64 if f64 else np.float32).reshape(-1, 2)
    fn = abi.lib().sdrhip_design_fftfilt_spectrum_f64 if f64 else abi.lib().sdrhip_design_fftfilt_spectrum
    return _designed(fn, (2 * h.shape[0], 2), h.dtype, h.shape[0], _p(h, True))


def design_fsk_lut(Fs, baud, freq):
    """One tone's LUT of FSKDetector::config (reference src/fsk.cc:32-44): [int(Fs / baud), 2] float32."""
    L = C.c_int(0)
    check(abi.lib().sdrhip_design_fsk_lut(Fs, baud, freq, C.byref(L), None, 0))
    t = np.zeros((L.value, 2), np.float32)
    check(abi.lib().sdrhip_design_fsk_lut(Fs, baud, freq, C.byref(L), _p(t, True), L.value))
    return t


# ---- context ------------------------------------------------------------------------------------

def device_count():
    return _out(C.c_int, abi.lib().sdrhip_device_count)


class _Handle:
    """Owner of one library handle `_h`: close() releases it once (`_release`), __del__ closes and keeps quiet."""

    def close(self):
        if self._h:
            self._release()
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    _borrowed = False

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        check(abi.lib().sdrhip_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.device = device

    @classmethod
    def borrowed(cls, handle, device):
        """A context some other object owns (sdrhip_comm_ctx: rank r's context lives as long as the comm)."""
        self = cls.__new__(cls)
        self._h, self.device, self._borrowed = C.c_void_p(handle.value if isinstance(handle, C.c_void_p) else handle), device, True
        return self

    @property
    def handle(self):
        return self._h

    def synchronize(self):
        check(abi.lib().sdrhip_ctx_synchronize(self._h))

    def device_name(self):
        return _text(abi.lib().sdrhip_ctx_device_name, self._h, size=256)

    def malloc(self, nbytes):
        return _out(C.c_void_p, abi.lib().sdrhip_malloc, self._h, nbytes)

    def free(self, p):
        check(abi.lib().sdrhip_free(self._h, C.c_void_p(p)))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        check(abi.lib().sdrhip_memcpy_h2d(self._h, C.c_void_p(dptr), _p(arr), arr.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        check(abi.lib().sdrhip_memcpy_d2h(self._h, _p(arr), C.c_void_p(dptr), arr.nbytes))

    def memset(self, dptr, value, nbytes):
        check(abi.lib().sdrhip_memset(self._h, C.c_void_p(dptr), value, nbytes))

    def _release(self):
        for hook in close_hooks:   # (buffers a device_router holds on this context)
            hook(self)
        if not self._borrowed:
            abi.lib().sdrhip_ctx_destroy(self._h)


class Timer(_Handle):
    """HIP events on the context's stream."""

    def __init__(self, ctx):
        self._h = C.c_void_p()
        check(abi.lib().sdrhip_timer_create(ctx.handle, C.byref(self._h)))

    def start(self):
        check(abi.lib().sdrhip_timer_start(self._h))

    def stop(self):
        check(abi.lib().sdrhip_timer_stop(self._h))

    def elapsed_ms(self):
        return _out(C.c_float, abi.lib().sdrhip_timer_elapsed_ms, self._h)

    def _release(self):
        abi.lib().sdrhip_timer_destroy(self._h)


# Seam for callers that bring their own device buffers to process(): when `device_router` is set, process(x) hands
# (ctx, x, out, call) to it instead of using the library's host-pointer entry point; the router stages x / out in device
# memory of its choosing and runs `call(in_ptr, in_stride, out_ptr, out_stride)` (the node's *_process_dev entry point,
# strides in row elements). None: the host-pointer path. `close_hooks` run before a context is destroyed.
# (tests/redzone.py installs a red-zoned arena here: guard bands around every row, checked after every call.)
device_router = None
close_hooks = []


class _Node(_Handle):
    """A node handle. The entry points `_prefix`_<name>, for "destroy" and every name in `_calls`, are bound at construction
    as self._c_<name>: a mistyped one fails there, and a call costs one attribute lookup. `_in` = (dtype, components) is
    the layout of process()'s input rows (components 0: real samples), `_assert_channels` whether their count is checked
    against self.channels — drifted, kept: the basebands, the detectors and the bit streams do, the other nodes never did."""
    _prefix, _calls = None, ""
    _in, _assert_channels = (np.int16, 2), False

    def __init__(self):
        self._h = C.c_void_p()
        self._bind(self._prefix, self._calls + " destroy")

    def _bind(self, prefix, calls):
        L = abi.lib()
        for name in calls.split():
            setattr(self, "_c_" + name, getattr(L, "%s_%s" % (prefix, name)))

    def _release(self):
        self._c_destroy(self._h)

    def _rows(self, x):
        return _rows(x, *self._in, self.channels if self._assert_channels else None)


class _Counted(_Node):
    """The family whose calls report an output count: out_count(n_in), process(x) -> [channels, n_out(, 2)] of `_out_dtype`
    (complex pairs unless an epilogue demodulates), process_dev(...) -> n_out. The router is met only when there is both
    input and output."""
    epilogue, _out_dtype = EPI_NONE, np.int16

    def out_count(self, n_in):
        return _out(C.c_size_t, self._c_out_count, self._h, n_in)

    def _zeros(self, no):
        return np.zeros((self.channels, no, 2) if self.epilogue == EPI_NONE else (self.channels, no), self._out_dtype)

    def _host_in(self, x, n_in):
        return _p(x), n_in, n_in

    def process(self, x):
        x = self._rows(x)
        n_in = x.shape[1]
        no = self.out_count(n_in)
        out = self._zeros(no)
        if device_router is not None and n_in and no:
            return device_router(self.ctx, x, out, lambda i, si, o, so: self._dev_checked(i, n_in, si, o, so, no))
        assert _out(C.c_size_t, self._c_process, self._h, *self._host_in(x, n_in), _p(out), no) == no
        return out

    def _dev_checked(self, i, n_in, si, o, so, no):
        assert self.process_dev(i, n_in, si, o, so) == no

    def process_dev(self, in_ptr, n_in, in_stride, out_ptr, out_stride):
        got = C.c_size_t(0)
        check(self._c_process_dev(self._h, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride, C.byref(got)))
        return got.value

    def reset(self):
        check(self._c_reset(self._h))


class _EqualLength(_Node):
    """The family whose calls write as many samples as they read: process_dev(...) returns nothing, and a class's process(x)
    shapes x and the zeroed output and hands both to _run. The router is met whenever there is input."""

    def _run(self, x, out, rows=None, routed=True):
        """rows: out as the C ABI's rows [rows_out, n, ...], where that is not out's own shape."""
        n = x.shape[1]
        if routed and device_router is not None and n:
            return device_router(self.ctx, x, out if rows is None else rows, lambda i, si, o, so: self.process_dev(i, n, si, o, so))
        check(self._c_process(self._h, _p(x), n, n, _p(out), n))
        return out

    def process_dev(self, in_ptr, n, in_stride, out_ptr, out_stride):
        check(self._c_process_dev(self._h, C.c_void_p(in_ptr), n, in_stride, C.c_void_p(out_ptr), out_stride))

    def reset(self):
        check(self._c_reset(self._h))


class _TilePlan:
    """Beside a family: the banks that walk `channels_per_group` rows in tiles of `tile_samples` — `_calls` names plan_info and
    kernel_names."""

    def plan_info(self, n=0):
        """{tile_samples, channels_per_group} of a call of n samples (0: max_in)."""
        t, g = C.c_int(0), C.c_int(0)
        check(self._c_plan_info(self._h, n or self.max_in, C.byref(t), C.byref(g)))
        return {"tile_samples": t.value, "channels_per_group": g.value}

    @property
    def kernel_names(self):
        return _text(self._c_kernel_names, self._h, size=256).split(",")


class IQBaseBandI16(_Counted):
    """K1 — IQBaseBand<int16_t> (+ fused FM/AM/USB). Mirrors sdr::gpu::IQBaseBand<int16_t>."""
    _prefix = "sdrhip_iqbb_i16"
    _calls = ("path kernel_names plan_info out_count process process_dev process_dev_multi reset adopt_state set_taps set_shift "
              "set_input_format")
    _create = "sdrhip_iqbb_i16_create"   # (BaseBandI16 and IQBaseBandI8 differ in this, `_in` and `_out_dtype`, nothing else)
    _assert_channels = True

    def __init__(self, ctx, taps, lut, lut_inc, negative, decim, channels=1, max_in=65536, epilogue=EPI_NONE):
        super().__init__()
        taps = np.ascontiguousarray(taps, np.int32).reshape(-1, 2)
        lut = np.ascontiguousarray(lut, np.int32).reshape(128, 2)
        self.ctx, self.channels, self.decim, self.epilogue, self.max_in = ctx, channels, decim, epilogue, max_in
        check(getattr(abi.lib(), self._create)(ctx.handle, _p(taps, True), taps.shape[0], _p(lut, True), lut_inc, int(bool(negative)),
                                               decim, channels, max_in, epilogue, C.byref(self._h)))

    @property
    def path(self):
        """0 = VALU dot2 kernel, 1 = int8-MFMA 32x32x32 (decim 8), 3 = int8-MFMA, any decim, 4 = real input (BaseBand) on the matrix cores."""
        return _out(C.c_int, self._c_path, self._h)

    @property
    def kernel_names(self):
        """Kernels a call launches, dominant first (what to look for in a rocprofv3 kernel trace)."""
        return _text(self._c_kernel_names, self._h, size=256).split(",")

    @property
    def plan_info(self):
        """{path, S, S0, NH, NW, kind, OP, HH, multi_left, L0, NL} of the plan (sdrhip.h: sdrhip_iqbb_i16_plan_info)."""
        v = (C.c_int * 11)()
        check(self._c_plan_info(self._h, v, 11))
        return dict(zip(("path", "S", "S0", "NH", "NW", "kind", "OP", "HH", "multi_left", "L0", "NL"), list(v)))

    def process_dev_multi(self, in_ptr, n_buffers, n_per_buffer, in_stride, out_ptr, out_stride):
        """n_buffers consecutive buffers per channel in ONE launch, buffer boundaries kept (sdrhip.h); returns the output
        counts per buffer (their outputs follow one another in each channel's row)."""
        counts = (C.c_size_t * max(1, n_buffers))()
        total = _out(C.c_size_t, self._c_process_dev_multi, self._h, C.c_void_p(in_ptr), n_buffers, n_per_buffer, in_stride,
                     C.c_void_p(out_ptr), out_stride, counts)
        assert sum(counts[:n_buffers]) == total
        return list(counts[:n_buffers])

    def process_multi(self, x, n_buffers):
        """Host arrays through process_dev_multi: x = [channels, n_buffers * n_per_buffer(, 2)]; returns (rows, counts) — the
        concatenated outputs of the buffers per channel and the output count of each buffer."""
        x = self._rows(x)
        assert x.shape[1] % n_buffers == 0
        n_in, nb = x.shape[1], x.shape[1] // n_buffers
        no = self.out_count(n_in)
        out = self._zeros(no)
        counts = []
        run = lambda i, si, o, so: counts.extend(self.process_dev_multi(i, n_buffers, nb, si, o, so))
        if device_router is not None:
            device_router(self.ctx, x, out, run)
        else:
            _roundtrip(self.ctx, x, out, lambda i, o: run(i, n_in, o, no), staged_out=True)
        return out, counts

    def reset(self, keep_history=False, keep_fm=False):
        check(self._c_reset(self._h, int(bool(keep_history)) | (2 if keep_fm else 0)))

    def adopt_state(self, other, what):
        """Streaming state of `other` carried into this FRESH plan (abi.KEEP_RING | KEEP_FM | KEEP_COUNTERS): what the
        reference node keeps when a setter changes the geometry a device plan is made for."""
        check(self._c_adopt_state(self._h, other._h, int(what)))

    def set_taps(self, taps):
        """setFilterFrequency / setFilterWidth of the reference node: the kernel only."""
        taps = np.ascontiguousarray(taps, np.int32).reshape(-1, 2)
        check(self._c_set_taps(self._h, _p(taps, True)))

    def set_shift(self, lut_inc, negative):
        """setCenterFrequency of the reference node: increment, sign, LUT phase restarts."""
        check(self._c_set_shift(self._h, lut_inc, int(bool(negative))))

    def set_input_format(self, fmt):
        """abi.IN_CS16 (default) or abi.IN_CU8 (complex<uint8> buffers, AutoCast<cs16> fused into the load)."""
        check(self._c_set_input_format(self._h, fmt))
        self._in = (np.uint8, 2) if fmt == abi.IN_CU8 else type(self)._in


class TunerBankI16(_Counted):
    """Tuner bank — C IQBaseBand<int16_t> channels (+ fused FM/AM/USB) over ONE shared input row, each with its own taps
    and frequency shift. modes (a sequence of EPI_FM | EPI_AM | EPI_USB, one per channel) makes a bank with a demodulator per
    channel (sdrhip_tunermodes_i16_create) instead of the one `epilogue`. Mirrors sdr::gpu::TunerBank<int16_t>.
    real=True: the channels are BaseBand<int16_t> nodes over ONE row of real int16 samples (sdrhip_tunerbb_i16_create /
    sdrhip_tunermodes_bb_i16_create; taps Q16 from design_bb_taps); mirrors sdr::gpu::RealTunerBank<int16_t>."""
    _prefix = "sdrhip_tuner_i16"
    _calls = "kernel_names plan_info out_count process process_dev set_taps set_shift set_input_format reset"
    _CREATE = {(False, False): "sdrhip_tuner_i16_create", (False, True): "sdrhip_tunermodes_i16_create",   # (real, modes given)
               (True, False): "sdrhip_tunerbb_i16_create", (True, True): "sdrhip_tunermodes_bb_i16_create"}

    def __init__(self, ctx, taps, lut, lut_inc, negative, decim, max_in=65536, epilogue=EPI_NONE, modes=None, real=False):
        super().__init__()
        self._bind("sdrhip_tunermodes_i16", "set_mode get_modes")
        self.real = bool(real)
        taps = np.ascontiguousarray(taps, np.int32)
        assert taps.ndim == 3 and taps.shape[2] == 2, taps.shape
        lut = np.ascontiguousarray(lut, np.int32).reshape(128, 2)
        inc = np.ascontiguousarray(lut_inc, np.uint32).reshape(-1)
        neg = np.ascontiguousarray(np.asarray(negative, bool), np.int32).reshape(-1)
        channels, order = taps.shape[0], taps.shape[1]
        assert inc.size == channels and neg.size == channels
        self.ctx, self.channels, self.order, self.decim, self.epilogue, self.max_in = ctx, channels, order, decim, epilogue, max_in
        if modes is not None:
            m = np.ascontiguousarray(modes, np.intc).reshape(-1)
            assert m.size == channels
            self.epilogue = EPI_FM   # (int16 rows; the bank's geometry is FM's)
            tail = (_p(m, True), decim, channels, max_in)
        else:
            tail = (decim, channels, max_in, epilogue)
        create = getattr(abi.lib(), self._CREATE[self.real, modes is not None])
        check(create(ctx.handle, _p(taps, True), order, _p(lut, True), _p(inc, True), _p(neg, True), *tail, C.byref(self._h)))

    @property
    def kernel_names(self):
        """The kernel the last call ran (before the first call: the one a call of max_in samples will run)."""
        return _text(self._c_kernel_names, self._h, size=256).split(",")

    def plan_info(self, n_in):
        """{hot, S, CG, OG, tiles, ctiles, ctw, grid_y, PLB, lds} of a call of n_in samples from the bank's current state
        (sdrhip.h: sdrhip_tuner_i16_plan_info)."""
        v = (C.c_int * 10)()
        check(self._c_plan_info(self._h, n_in, v, 10))
        return dict(zip(("hot", "S", "CG", "OG", "tiles", "ctiles", "ctw", "grid_y", "PLB", "lds"), list(v)))

    # process(x) — x: ONE row [n, 2] (int16, or uint8 after set_input_format(IN_CU8)) — a real bank: [n] int16; returns
    # [C, n_out(, 2)]. The router sees the row as x[None]; the bank's calls take no input stride.
    def _rows(self, x):
        x = np.ascontiguousarray(x, self._in[0])
        if self.real:
            assert x.ndim == 1, x.shape
        else:
            assert x.ndim == 2 and x.shape[1] == 2, x.shape
        return x[None]

    def _host_in(self, x, n_in):
        return _p(x[0]), n_in

    def _dev_checked(self, i, n_in, si, o, so, no):
        assert self.process_dev(i, n_in, o, so) == no

    def process_dev(self, in_ptr, n_in, out_ptr, out_stride):
        got = C.c_size_t(0)
        check(self._c_process_dev(self._h, C.c_void_p(in_ptr), n_in, C.c_void_p(out_ptr), out_stride, C.byref(got)))
        return got.value

    def set_taps(self, c, taps):
        """setFilterFrequency / setFilterWidth of channel c: that channel's kernel only."""
        taps = np.ascontiguousarray(taps, np.int32).reshape(-1, 2)
        assert taps.shape[0] == self.order
        check(self._c_set_taps(self._h, int(c), _p(taps, True)))

    def set_shift(self, c, lut_inc, negative):
        """setCenterFrequency of channel c: increment, sign, that channel's LUT phase restarts."""
        check(self._c_set_shift(self._h, int(c), lut_inc, int(bool(negative))))

    def set_mode(self, c, mode):
        """A new demodulator node (EPI_FM | EPI_AM | EPI_USB) behind channel c's baseband, which goes on as it is; banks made
        with modes= only."""
        check(self._c_set_mode(self._h, int(c), int(mode)))

    def modes(self):
        """The channels' demodulators; banks made with modes= only."""
        m = (C.c_int * self.channels)()
        check(self._c_get_modes(self._h, m, self.channels))
        return list(m)

    def set_input_format(self, fmt):
        check(self._c_set_input_format(self._h, fmt))
        self._in = (np.uint8 if fmt == abi.IN_CU8 else np.int16, 2)

    def reset(self, keep_history=False, keep_fm=False):
        check(self._c_reset(self._h, int(bool(keep_history)) | (2 if keep_fm else 0)))


class BaseBandI16(IQBaseBandI16):
    """BaseBand<int16_t>, the real-input node (reference src/baseband.hh:305-529): int16 samples in, cs16 (or the
    demodulated int16) out. Shares the handle type and every call except create with IQBaseBandI16."""
    _create, _in = "sdrhip_bb_i16_create", (np.int16, 0)


class IQBaseBandI8(IQBaseBandI16):
    """IQBaseBand<int8_t> (the documentation example's baseband, reference src/sdr.hh:225-240): complex<int8> in,
    complex<int8> out — or, with EPI_FM, FMDemod<int8_t,int16_t>'s int16. Same handle type as IQBaseBandI16."""
    _create, _in = "sdrhip_iqbb_i8_create", (np.int8, 2)
    _out_dtype = property(lambda self: np.int8 if self.epilogue == EPI_NONE else np.int16)


class FIR(_Counted):
    """K2/K3 — FIRFilter<complex<int16>> exact / FIRFilter<complex<float>> (+ folded SubSample, + demod)."""
    _prefix, _calls = "sdrhip_fir", "kernel_names last_kernels out_count process process_dev reset set_taps"

    def __init__(self, ctx, kind, alpha, decim=1, channels=1, max_in=65536, epilogue=EPI_NONE):
        super().__init__()
        alpha = np.ascontiguousarray(alpha, np.float64)
        self.ctx, self.kind, self.channels, self.decim, self.epilogue = ctx, kind, channels, decim, epilogue
        self.order = alpha.shape[0]
        self._out_dtype = np.int16 if kind == FIR_CS16_EXACT else np.float32
        self._in = (self._out_dtype, 2)
        check(abi.lib().sdrhip_fir_create(ctx.handle, kind, _p(alpha, True), alpha.shape[0], decim, channels, max_in, epilogue,
                                          C.byref(self._h)))

    def kernel_names(self, n_in=0):
        """The kernel a call of n_in samples per channel runs (0: max_in) — what to look for in a rocprofv3 kernel trace."""
        return _text(self._c_kernel_names, self._h, n_in, size=256).split(",")

    def last_kernels(self):
        """The kernels the most recent process / process_dev call launched, in launch order ([] before the first call and
        after a call of 0 samples)."""
        return _split_kernels(_text(self._c_last_kernels, self._h, size=4096))

    def set_taps(self, alpha):
        """New coefficients, same order: the ring (the stream) goes on (FIRFilter::setUpperFreq, src/firfilter.hh:165-170)."""
        alpha = np.ascontiguousarray(alpha, np.float64)
        assert alpha.shape == (self.order,)
        check(self._c_set_taps(self._h, _p(alpha, True)))


class Demod(_EqualLength):
    """K4/K5 — stand-alone FMDemod<int16_t> / AMDemod / USBDemod."""
    _prefix, _calls = "sdrhip_demod", "process process_dev reset"

    def __init__(self, ctx, kind, dtype=T_CS16, channels=1, max_in=65536, inplace_fm0=True):
        super().__init__()
        self.ctx, self.kind, self.dtype, self.channels = ctx, kind, dtype, channels
        self._in = (np.int16 if dtype == T_CS16 else np.int8 if dtype == abi.T_CS8 else np.float32, 2)
        check(abi.lib().sdrhip_demod_create(ctx.handle, kind, dtype, channels, max_in, int(inplace_fm0), C.byref(self._h)))

    def process(self, x, out=None):
        x = self._rows(x)
        if out is not None:   # (drifted, kept: a caller's out never meets the router)
            return self._run(x, out, routed=False)
        return self._run(x, np.zeros((self.channels, x.shape[1]), np.float32 if self.dtype == T_CF32 else np.int16))


class FMDeemphI16(_EqualLength):
    """FMDeemph<int16_t>: sequential integer IIR per channel."""
    _prefix, _calls, _in = "sdrhip_deemph_i16", "process process_dev kernel_names reset", (np.int16, 0)

    def __init__(self, ctx, alpha, channels=1, max_in=65536):
        super().__init__()
        self.ctx, self.channels = ctx, channels
        check(abi.lib().sdrhip_deemph_i16_create(ctx.handle, alpha, channels, max_in, C.byref(self._h)))

    def process(self, x):
        x = self._rows(x)
        return self._run(x, np.zeros_like(x))

    def kernel_names(self, n=0):
        """The kernel a call of n samples per channel runs (0: max_in)."""
        return _text(self._c_kernel_names, self._h, n, size=256).split(",")


class SymbolDetector(_EqualLength):
    """FSKDetector / ASKDetector<int16_t> on `channels` rows: int16 [channels, n] in, symbols uint8 [channels, n] out."""
    _prefix, _calls = "sdrhip_detector", "process process_dev kernel_names reset"
    _in, _assert_channels = (np.int16, 0), True

    def __init__(self, ctx, kind, mark_lut=None, space_lut=None, invert=False, channels=1, max_in=65536):
        super().__init__()
        self.ctx, self.kind, self.channels = ctx, kind, channels
        if kind == abi.DET_FSK:
            m, s = _lut_pairs(mark_lut), _lut_pairs(space_lut)
            assert m.shape == s.shape, (m.shape, s.shape)
            check(abi.lib().sdrhip_detector_create(ctx.handle, kind, _p(m, True), _p(s, True), m.shape[0], 0, channels, max_in,
                                                   C.byref(self._h)))
        else:
            check(abi.lib().sdrhip_detector_create(ctx.handle, kind, None, None, 0, int(bool(invert)), channels, max_in, C.byref(self._h)))

    def process(self, x):
        x = self._rows(x)
        return self._run(x, np.zeros(x.shape, np.uint8))

    @property
    def kernel_names(self):
        return _text(self._c_kernel_names, self._h, size=256).split(",")


class FSKDetector(SymbolDetector):
    """sdr::FSKDetector(baud, Fmark, Fspace) at sample rate Fs; pass mark_lut / space_lut to pin the LUTs (fixtures)."""

    def __init__(self, ctx, Fs, baud, Fmark, Fspace, channels=1, max_in=65536, mark_lut=None, space_lut=None):
        if mark_lut is None:
            mark_lut, space_lut = design_fsk_lut(Fs, baud, Fmark), design_fsk_lut(Fs, baud, Fspace)
        super().__init__(ctx, abi.DET_FSK, mark_lut, space_lut, channels=channels, max_in=max_in)


class ASKDetector(SymbolDetector):
    """sdr::ASKDetector<int16_t>(invert)."""

    def __init__(self, ctx, invert=False, channels=1, max_in=65536):
        super().__init__(ctx, abi.DET_ASK, invert=invert, channels=channels, max_in=max_in)


class BitStream(_Node):
    """sdr::BitStream(baud, mode) at sample rate Fs on `channels` rows: symbols uint8 [channels, n] in; process() returns the
    list of the channels' bit arrays (their lengths depend on the data)."""
    _prefix, _calls = "sdrhip_bits", "corr_len out_capacity kernel_names process process_dev reset"
    _in, _assert_channels = (np.uint8, 0), True

    def __init__(self, ctx, Fs, baud, mode=abi.BITS_TRANSITION, channels=1, max_in=65536):
        super().__init__()
        self.ctx, self.channels, self._counts_dev = ctx, channels, 0
        check(abi.lib().sdrhip_bits_create(ctx.handle, Fs, baud, mode, channels, max_in, C.byref(self._h)))

    @property
    def corr_len(self):
        return _out(C.c_int, self._c_corr_len, self._h)

    def out_capacity(self, n):
        return _out(C.c_size_t, self._c_out_capacity, self._h, n)

    @property
    def kernel_names(self):
        return _text(self._c_kernel_names, self._h, size=256).split(",")

    def process_raw(self, x):
        """-> (bits [channels, capacity(n)] uint8, counts [channels] uint32)"""
        x = self._rows(x)
        n = x.shape[1]
        cap = self.out_capacity(n)
        out, counts = np.zeros((self.channels, cap), np.uint8), np.zeros(self.channels, np.uint32)
        if device_router is not None and n:   # (the counts go through a device buffer of the node's own, freed in close())
            if not self._counts_dev:
                self._counts_dev = self.ctx.malloc(4 * self.channels)
            device_router(self.ctx, x, out, lambda i, si, o, so: self.process_dev(i, n, si, o, so, self._counts_dev))
            self.ctx.d2h(counts, self._counts_dev)
            return out, counts
        check(self._c_process(self._h, _p(x), n, n, _p(out), cap, _p(counts)))
        return out, counts

    def process(self, x):
        out, counts = self.process_raw(x)
        return [out[c, :counts[c]].copy() for c in range(self.channels)]

    def process_dev(self, sym_ptr, n, in_stride, bits_ptr, out_stride, counts_ptr):
        check(self._c_process_dev(self._h, C.c_void_p(sym_ptr), n, in_stride, C.c_void_p(bits_ptr), out_stride, C.c_void_p(counts_ptr)))

    def reset(self):
        check(self._c_reset(self._h))

    def _release(self):
        if self._counts_dev:
            self.ctx.free(self._counts_dev)
            self._counts_dev = 0
        super()._release()


def _lut_pairs(lut):
    return np.ascontiguousarray(lut, np.float32).reshape(-1, 2)


class SymbolDetectorBank(SymbolDetector):
    """A detector PER CHANNEL (sdrhip_detectorbank_create): `channels` is a list with one entry per row,
    ("fsk", mark_lut, space_lut) — LUTs as design_fsk_lut makes them — or ("ask", invert). One launch serves all rows;
    set_channel replaces the node behind one row between two calls. max_corr_len: the longest correlator a later
    set_channel may ask for (default: the bank's longest)."""

    def __init__(self, ctx, channels, max_in=65536, max_corr_len=0):
        _Node.__init__(self)
        self._bind("sdrhip_detectorbank", "set_channel")
        self.ctx, self.channels, self.kind = ctx, len(channels), None
        kinds, lens, inv, marks, spaces = [], [], [], [], []
        for ch in channels:
            kind, m, s, L, i = self._channel(ch)
            kinds.append(kind); lens.append(L); inv.append(i)
            if kind == abi.DET_FSK:
                marks.append(m); spaces.append(s)
        kinds, lens, inv = (_p(np.ascontiguousarray(v, np.intc), True) for v in (kinds, lens, inv))
        m, s = (_p(np.concatenate(v), True) if marks else None for v in (marks, spaces))
        check(abi.lib().sdrhip_detectorbank_create(ctx.handle, kinds, lens, inv, m, s, max_corr_len, self.channels, max_in, C.byref(self._h)))

    @staticmethod
    def _channel(ch):
        """-> (kind, mark [L, 2] | None, space | None, corr_len, invert)"""
        if ch[0] in ("fsk", abi.DET_FSK):
            m, s = _lut_pairs(ch[1]), _lut_pairs(ch[2])
            assert m.shape == s.shape, (m.shape, s.shape)
            return abi.DET_FSK, m, s, m.shape[0], 0
        assert ch[0] in ("ask", abi.DET_ASK), ch[0]
        return abi.DET_ASK, None, None, 0, int(bool(ch[1])) if len(ch) > 1 else 0

    def set_channel(self, c, channel):
        """Row c becomes a freshly configured node — ("fsk", mark_lut, space_lut) or ("ask", invert); the other rows stream on."""
        kind, m, s, L, inv = self._channel(channel)
        check(self._c_set_channel(self._h, c, kind, _p(m, True) if m is not None else None, _p(s, True) if s is not None else None, L, inv))


class BitStreamBank(BitStream):
    """A BitStream PER CHANNEL at one sample rate (sdrhip_bitsbank_create): bauds[c], modes[c]. out_capacity(n) is the
    largest channel's capacity (the row stride); channel_info(c, n) the row's own numbers. set_channel replaces the node behind
    one row between two calls. max_corr_len: the longest window a later set_channel may ask for (default: the bank's longest)."""

    def __init__(self, ctx, Fs, bauds, modes, max_in=65536, max_corr_len=0):
        _Node.__init__(self)
        self._bind("sdrhip_bitsbank", "set_channel channel_info")
        bauds, modes = np.ascontiguousarray(bauds, np.float32).ravel(), np.ascontiguousarray(modes, np.intc).ravel()
        assert bauds.size == modes.size, (bauds.size, modes.size)
        self.ctx, self.channels, self._counts_dev = ctx, int(bauds.size), 0
        check(abi.lib().sdrhip_bitsbank_create(ctx.handle, Fs, _p(bauds, True), _p(modes, True), self.channels, max_in, max_corr_len,
                                               C.byref(self._h)))

    def set_channel(self, c, baud, mode=abi.BITS_TRANSITION):
        check(self._c_set_channel(self._h, c, baud, mode))

    def channel_info(self, c, n=0):
        """-> dict(corr_len, omega_min, omega_max, capacity) of row c for a call of n symbols"""
        L, lo, hi, cap = C.c_int(0), C.c_float(0), C.c_float(0), C.c_size_t(0)
        check(self._c_channel_info(self._h, c, n, C.byref(L), C.byref(lo), C.byref(hi), C.byref(cap)))
        return {"corr_len": L.value, "omega_min": lo.value, "omega_max": hi.value, "capacity": cap.value}


class SubSample(_Counted):
    """K6 — SubSample<complex<int16>|complex<float>>."""
    _prefix, _calls = "sdrhip_subsample", "out_count process process_dev reset"

    def __init__(self, ctx, dtype, n, channels=1, max_in=65536):
        super().__init__()
        self.ctx, self.dtype, self.n, self.channels = ctx, dtype, n, channels
        self._out_dtype = np.int16 if dtype == T_CS16 else np.float32
        self._in = (self._out_dtype, 2)
        check(abi.lib().sdrhip_subsample_create(ctx.handle, dtype, n, channels, max_in, C.byref(self._h)))


class FFTConv(_EqualLength):
    """K7 — FilterSink+FilterSource (mode OLA, kernel = 2N spectrum) or overlap-save with taps (mode OLS).
    `kernels` may be a list of equally sized kernels: a filter bank behind one forward transform per block
    (FilterNode); process() then returns [bands, channels, n, 2]. dtype=np.float64: FilterNode<double>'s plan
    (sdrhip_fftconv_f64_*)."""
    _prefix, _calls = "sdrhip_fftconv", "last_kernels reset"

    def __init__(self, ctx, mode, fft_size, kernel, channels=1, max_in=65536, dtype=np.float32):
        super().__init__()
        bank = isinstance(kernel, (list, tuple))
        self.dtype = np.dtype(dtype)
        self.f64 = self.dtype == np.float64
        self._in = (self.dtype, 2)
        self._bind("sdrhip_fftconv_f64" if self.f64 else "sdrhip_fftconv", "create_bank set_kernel process process_dev")
        ks = [np.ascontiguousarray(k, self.dtype).reshape(-1, 2) for k in (kernel if bank else [kernel])]
        assert all(k.shape == ks[0].shape for k in ks)
        self.ctx, self.mode, self.fft_size, self.channels, self.bands, self._bank = ctx, mode, fft_size, channels, len(ks), bank
        allk = np.ascontiguousarray(np.stack(ks))
        check(self._c_create_bank(ctx.handle, mode, fft_size, _p(allk, True), ks[0].shape[0], len(ks), channels, max_in, C.byref(self._h)))

    def process(self, x):
        x = self._rows(x)
        out = np.zeros((self.bands,) + x.shape, self.dtype)
        self._run(x, out, rows=out.reshape((self.bands * x.shape[0],) + x.shape[1:]))   # band-major rows, as the C ABI lays them out
        return out if self._bank else out[0]

    def set_kernel(self, band, kernel):
        kernel = np.ascontiguousarray(kernel, self.dtype).reshape(-1, 2)
        check(self._c_set_kernel(self._h, band, _p(kernel, True)))

    def last_kernels(self):
        """The kernels the most recent process / process_dev call launched, in launch order ([] before the first call and
        after a call of 0 samples)."""
        return _split_kernels(_text(self._c_last_kernels, self._h, size=4096))


def _split_dtype(dtype):
    dt = np.dtype(dtype)
    assert dt in (np.float32, np.float64), dt
    return dt, (T_CF64 if dt == np.float64 else T_CF32)


class FFTSink(_Node):
    """FilterSink<Scalar> (sdrhip_fftsink_*): every N samples -> one 2N-point spectrum (zero-padded block, forward DFT,
    natural order). process(x[channels, n_in, 2]) -> [channels, n_in / N, 2N, 2]; n_in must be a multiple of N.
    (FFTSink and FFTSource never meet the device_router.)"""
    _prefix, _calls = "sdrhip_fftsink", "form process process_dev"

    def __init__(self, ctx, N, channels=1, max_blocks=64, dtype=np.float32):
        super().__init__()
        self.dtype, dt = _split_dtype(dtype)
        self.ctx, self.N, self.channels, self._in = ctx, N, channels, (self.dtype, 2)
        check(abi.lib().sdrhip_fftsink_create(ctx.handle, dt, N, channels, max_blocks, C.byref(self._h)))

    @property
    def form(self):
        return _text(self._c_form, self._h)

    def process(self, x):
        x = self._rows(x)
        n = x.shape[1]
        out = np.zeros((x.shape[0], n // self.N, 2 * self.N, 2), self.dtype)
        check(self._c_process(self._h, _p(x), n, n, _p(out), out.shape[1] * 2 * self.N))
        return out

    def process_dev(self, in_ptr, n_in, in_stride, spec_ptr, spec_stride):
        check(self._c_process_dev(self._h, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(spec_ptr), spec_stride))


class FFTSource(_Node):
    """FilterSource<Scalar> (sdrhip_fftsource_*): spectra [channels, blocks, 2N, 2] -> overlap-added output
    [channels, blocks * N, 2]; the tail is carried across calls. `spectrum`: the 2N-point kernel spectrum (natural order,
    normalised: design_fftfilt_spectrum)."""
    _prefix, _calls = "sdrhip_fftsource", "form process process_dev set_kernel reset"

    def __init__(self, ctx, N, spectrum, channels=1, max_blocks=64, dtype=np.float32):
        super().__init__()
        self.dtype, dt = _split_dtype(dtype)
        self.ctx, self.N, self.channels = ctx, N, channels
        k = np.ascontiguousarray(spectrum, self.dtype)
        check(abi.lib().sdrhip_fftsource_create(ctx.handle, dt, N, _p(k), channels, max_blocks, C.byref(self._h)))

    @property
    def form(self):
        return _text(self._c_form, self._h)

    def process(self, spec):
        spec = np.ascontiguousarray(spec, self.dtype)
        if spec.ndim == 3:
            spec = spec[None]
        c, nb = spec.shape[0], spec.shape[1]
        out = np.zeros((c, nb * self.N, 2), self.dtype)
        check(self._c_process(self._h, _p(spec), nb, nb * 2 * self.N, _p(out), nb * self.N))
        return out

    def process_dev(self, spec_ptr, n_blocks, spec_stride, out_ptr, out_stride):
        check(self._c_process_dev(self._h, C.c_void_p(spec_ptr), n_blocks, spec_stride, C.c_void_p(out_ptr), out_stride))

    def set_kernel(self, spectrum):
        k = np.ascontiguousarray(spectrum, self.dtype)
        check(self._c_set_kernel(self._h, _p(k)))

    def reset(self):
        check(self._c_reset(self._h))


class FloatBaseBand(_Counted):
    """Build-defined float baseband (BASELINE config 2): shift -> FIR(cf32) -> /D."""
    _prefix, _calls = "sdrhip_fbb_f32", "kernel_names last_kernels out_count process process_dev reset set_taps set_shift"
    _in, _out_dtype = (np.float32, 2), np.float32

    def __init__(self, ctx, Fc, Fs, alpha, decim, channels=1, max_in=65536):
        super().__init__()
        alpha = np.ascontiguousarray(alpha, np.float64)
        self.ctx, self.channels, self.decim, self.order = ctx, channels, decim, alpha.shape[0]
        check(abi.lib().sdrhip_fbb_f32_create(ctx.handle, Fc, Fs, _p(alpha, True), alpha.shape[0], decim, channels, max_in,
                                              C.byref(self._h)))

    def kernel_names(self, n_in=0):
        """The kernel a call of n_in samples per channel runs (0: max_in)."""
        return _text(self._c_kernel_names, self._h, n_in, size=256).split(",")

    def last_kernels(self):
        """The kernels the most recent process / process_dev call launched, in launch order ([] before the first call and
        after a call of 0 samples)."""
        return _split_kernels(_text(self._c_last_kernels, self._h, size=4096))

    def set_taps(self, alpha):
        alpha = np.ascontiguousarray(alpha, np.float64)
        assert alpha.shape == (self.order,)   # (the C side reads `order` doubles)
        check(self._c_set_taps(self._h, _p(alpha, True)))

    def set_shift(self, Fc):
        check(self._c_set_shift(self._h, float(Fc)))


def _fft_c2c(fn, ctx, x, sign, dtype):
    x = np.ascontiguousarray(x, dtype)
    return _roundtrip(ctx, x, np.zeros_like(x),
                      lambda i, o: check(fn(ctx.handle, x.shape[1], sign, x.shape[0], C.c_void_p(i), C.c_void_p(o))))


def fft_c2c(ctx, x, sign):
    """Batched DFT with the library's own in-LDS FFT (test hook)."""
    return _fft_c2c(abi.lib().sdrhip_fft_c2c, ctx, x, sign, np.float32)


def fft_c2c_f64(ctx, x, sign):
    """Batched DFT on complex<double> (FFTPlan<double>): x is (batch, n, 2) float64."""
    return _fft_c2c(abi.lib().sdrhip_fft_c2c_f64, ctx, x, sign, np.float64)


def fft_exec(ctx, x, sign):
    """FFT::exec on a host buffer: x complex64 or complex128, one transform."""
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.complex64, np.complex128) and x.ndim == 1
    out = np.empty_like(x)
    check(abi.lib().sdrhip_fft_exec(ctx.handle, abi.T_CF64 if x.dtype == np.complex128 else abi.T_CF32, x.shape[0], sign,
                                    _p(x), _p(out)))
    return out


class Comm(_Handle):
    """sdrhip_comm_*: one process, one rank context per device (RCCL between distinct devices, same-device copies when
    every rank sits on one device). Mirrors what sdr::gpu::ChannelBank(devices) does on the C++ side."""

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*devices)
        self._h = C.c_void_p()
        check(abi.lib().sdrhip_comm_create(devs, len(devices), C.byref(self._h)))
        self.devices = list(devices)
        self.ctx = [Context.borrowed(_out(C.c_void_p, abi.lib().sdrhip_comm_ctx, self._h, r), d) for r, d in enumerate(devices)]

    @property
    def transport(self):
        return _text(abi.lib().sdrhip_comm_transport, self._h)

    def broadcast(self, ptrs, nbytes, root=0):
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        check(abi.lib().sdrhip_comm_broadcast(self._h, arr, nbytes, root))

    def gather(self, send_ptrs, nbytes, recv_ptr, root=0):
        sp = (C.c_void_p * len(send_ptrs))(*send_ptrs)
        nb = (C.c_size_t * len(nbytes))(*nbytes)
        check(abi.lib().sdrhip_comm_gather(self._h, sp, nb, C.c_void_p(recv_ptr), root))

    def gather_begin(self, slot, send_ptrs, nbytes, recv_ptr, root=0):
        """The gather on the comm's own streams (overlaps the ranks' next kernels); gather_wait(slot) orders the ranks' streams behind it."""
        sp = (C.c_void_p * len(send_ptrs))(*send_ptrs)
        nb = (C.c_size_t * len(nbytes))(*nbytes)
        check(abi.lib().sdrhip_comm_gather_begin(self._h, slot, sp, nb, C.c_void_p(recv_ptr), root))

    def gather_wait(self, slot):
        check(abi.lib().sdrhip_comm_gather_wait(self._h, slot))

    def synchronize(self):
        check(abi.lib().sdrhip_comm_synchronize(self._h))

    def _release(self):
        for c in self.ctx:
            c.close()
        abi.lib().sdrhip_comm_destroy(self._h)


class FFTPlan(_Node):
    """sdrhip_fft_plan_*: FFTPlan<float|double> planned once (any size), executed many times."""
    _prefix, _calls = "sdrhip_fft_plan", "form exec exec_dev"

    def __init__(self, ctx, n, dtype=np.complex64):
        super().__init__()
        self.ctx, self.n, self.dtype = ctx, int(n), np.dtype(dtype)
        assert self.dtype in (np.dtype(np.complex64), np.dtype(np.complex128))
        check(abi.lib().sdrhip_fft_plan_create(ctx.handle, abi.T_CF64 if self.dtype == np.complex128 else abi.T_CF32, self.n, C.byref(self._h)))

    @property
    def form(self):
        return _text(self._c_form, self._h)

    def exec(self, x, sign):
        """One transform on host buffers (FFTPlan::operator())."""
        x = np.ascontiguousarray(x, self.dtype)
        assert x.shape == (self.n,)
        out = np.empty_like(x)
        check(self._c_exec(self._h, sign, _p(x), _p(out)))
        return out

    def exec_batch(self, x, sign):
        """x: [batch, n] -> [batch, n] through device memory (exec_dev)."""
        x = np.ascontiguousarray(x, self.dtype)
        assert x.ndim == 2 and x.shape[1] == self.n
        return _roundtrip(self.ctx, x, np.empty_like(x),
                          lambda i, o: check(self._c_exec_dev(self._h, sign, x.shape[0], C.c_void_p(i), C.c_void_p(o))))
