"""CPU call trace of libsdr_amd.nodes: every wrapper is driven against a FAKE library that answers the names of
abi.SIGNATURES only, refuses what ctypes would refuse (argument count, each argument through its declared argtype's
from_param) and records every call in a normal form. The recorded lists are compared with the tables below, so a mistyped
entry point, a wrong argument count or type, a changed call order or a changed router decision shows here, without
libsdrhip.so and without a device.

Normal form of a call: (name, arguments...) with scalars by value, handles as "h<k>" in the order the fake made them, device
pointers by value, out-parameters as ("out", ctype), ctypes arrays as (ctype, values), string buffers as ("buf", size); a
numpy array behind a pointer is ("bytes", nbytes, crc32) in create / set_* / design calls and (dtype, shape, content) in every
other call, content being "zeros" or the crc32 of its bytes. ("router", ctx, x, out) is a call of nodes.device_router,
("hook", ctx) one of nodes.close_hooks, ("ret", tag, value) what a wrapper returned."""
import ctypes as C
import inspect
import zlib

import numpy as np
import pytest

from libsdr_amd import abi, nodes
from libsdr_amd.abi import EPI_NONE, EPI_FM, EPI_AM

KERNELS, FORM = b"k_main<1,2>,k_tail", b"radix4"
NAMES, LAST = ["k_main<1", "2>", "k_tail"], ["k_main<1,2>", "k_tail"]   # kernel_names splits at every comma, last_kernels outside <>
OUT_SZ, OUT_I, OUT_VP = ("out", "c_ulong"), ("out", "c_int"), ("out", "c_void_p")


def count(n):
    """What the fake's *_out_count / *_out_capacity answer for n, and what its counted process calls report."""
    return n // 4


def B(a):
    a = np.asarray(a)
    return ("bytes", a.nbytes, zlib.crc32(a.tobytes()))


def Z(nbytes):
    """A zeroed array of nbytes (an output of a design call)."""
    return B(np.zeros(nbytes, np.uint8))


def A(a):
    return (a.dtype.str, a.shape, zlib.crc32(a.tobytes()) if a.any() else "zeros")


def R(v):
    """Normal form of a returned value."""
    if isinstance(v, np.ndarray):
        return A(v)
    if isinstance(v, (list, tuple)):
        return type(v)(R(e) for e in v)
    if isinstance(v, dict):
        return {k: R(e) for k, e in v.items()}
    return v.item() if isinstance(v, np.generic) else v


class FakeLib:
    """signatures: the names the fake answers (default: abi.SIGNATURES; a side header's test adds its own table). answers:
    name -> function of args that fills the call's outputs in place of _fill. scalars_only: arguments other than ints and
    floats are recorded as None, not in their normal form."""

    def __init__(self, signatures=None, answers=None, scalars_only=False):
        self.calls, self.reached, self.handles, self.mallocs = [], set(), {}, 0
        self.signatures, self.answers, self.scalars_only = signatures or abi.SIGNATURES, answers or {}, scalars_only

    def __getattr__(self, name):
        if name not in self.signatures:
            raise AttributeError(name)
        self.reached.add(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        argtypes = self.signatures[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for a, t in zip(args, argtypes):
            t.from_param(a)
        config = name.endswith(("_create", "_create_bank")) or "_set_" in name or "_design_" in name
        if self.scalars_only:
            self.calls.append((name,) + tuple(a if isinstance(a, (int, float)) else None for a in args))
        else:
            self.calls.append((name,) + tuple(self._norm(a, config) for a in args))
        if name in self.answers:
            self.answers[name](args)
        else:
            self._fill(name, args)
        return abi.OK

    def _norm(self, a, config):
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, np.generic):
            return a.item()
        if getattr(a, "_arr", None) is not None:     # a pointer numpy made: data_as keeps its array
            return B(a._arr) if config else A(a._arr)
        if isinstance(a, C.c_void_p):
            return self.handles.get(a.value, a.value)
        if hasattr(a, "_obj"):                        # byref(x)
            return ("out", type(a._obj).__name__)
        assert isinstance(a, C.Array), a
        return ("buf", len(a)) if a._type_ is C.c_char else (a._type_.__name__, [self.handles.get(v, v) for v in a])

    def _fill(self, name, args):
        outs = [a._obj for a in args if hasattr(a, "_obj")]
        if name.endswith(("_create", "_create_bank")) or name == "sdrhip_comm_ctx":
            k = len(self.handles) + 1
            self.handles[0xA0000000 + 16 * k] = "h%d" % k
            outs[-1].value = 0xA0000000 + 16 * k
        elif name == "sdrhip_malloc":
            self.mallocs += 1
            outs[0].value = 0xD0000 + 0x1000 * self.mallocs
        elif name.endswith(("_out_count", "_out_capacity")):
            outs[0].value = count(args[1])
        elif name.endswith("_process_dev_multi"):
            nb, total = args[2], count(args[2] * args[3])
            for k in range(nb):
                args[7][k] = total // nb + (total % nb if k == nb - 1 else 0)
            outs[0].value = total
        elif name.endswith(("_process", "_process_dev")):
            if outs:                                  # a counted call
                outs[0].value = count(args[2])
        elif name.endswith(("_kernel_names", "_last_kernels", "_device_name")):
            args[-2].value = KERNELS
        elif name.endswith(("_form", "_transport")):
            outs[0].value = FORM
        elif name.endswith(("_plan_info", "_get_modes")):
            for k in range(args[-1]):
                args[-2][k] = k + 1
        else:
            for o in outs:                            # every other scalar out-parameter
                o.value = 7


class Run:
    """One case's fake library (default: a FakeLib of abi.SIGNATURES), recording router and — unless hook is False — close hook."""

    def __init__(self, monkeypatch, fake=None, hook=True):
        self.fake, self.mp = fake or FakeLib(), monkeypatch
        monkeypatch.setattr(abi, "_lib", self.fake)
        monkeypatch.setattr(nodes, "close_hooks", [lambda ctx: self.fake.calls.append(("hook", self.h(ctx)))] if hook else [])
        self.route(False)

    def h(self, obj):
        return self.fake.handles.get(obj._h.value, obj._h.value)

    def _router(self, ctx, x, out, call):
        self.fake.calls.append(("router", self.h(ctx), A(x), A(out)))
        call(0x1000, x.shape[1] + 3, 0x2000, out.shape[1] + 3)
        return out

    def route(self, on):
        self.mp.setattr(nodes, "device_router", self._router if on else None)

    def ret(self, tag, v):
        self.fake.calls.append(("ret", tag, R(v)))

    def three(self, tag, node, x, empty):
        """process() on the host-pointer path, through the router, and on an empty input with the router still set."""
        self.route(False)
        self.ret(tag, node.process(x))
        self.route(True)
        self.ret(tag + "/routed", node.process(x))
        self.ret(tag + "/empty", node.process(empty))
        self.route(False)

    def ctx(self):
        return nodes.Context(0)


def ramp(shape, dtype, start):
    return (np.arange(start, start + int(np.prod(shape))) % 101 + 1).astype(dtype).reshape(shape)


# 2 channels, 16 samples, order 5: every array has its own content, so a swapped argument shows
TAPS, TAPS2, BTAPS = ramp((5, 2), np.int32, 1), ramp((5, 2), np.int32, 2), ramp((2, 5, 2), np.int32, 4)
LUT = ramp((128, 2), np.int32, 3)
ALPHA, ALPHA2 = ramp((5,), np.float64, 5), ramp((5,), np.float64, 6)
X16, XU8, XI8 = ramp((2, 16, 2), np.int16, 7), ramp((2, 16, 2), np.uint8, 8), ramp((2, 16, 2), np.int8, 9)
XR16, XF32, XF64 = ramp((2, 16), np.int16, 10), ramp((2, 16, 2), np.float32, 11), ramp((2, 16, 2), np.float64, 12)
ROW16, ROWU8, ROWR = ramp((16, 2), np.int16, 13), ramp((16, 2), np.uint8, 14), ramp((16,), np.int16, 15)
SYM = ramp((2, 16), np.uint8, 16)
MARK, SPACE = ramp((4, 2), np.float32, 17), ramp((4, 2), np.float32, 18)
KERN, KERN2, KERN64 = ramp((8, 2), np.float32, 19), ramp((8, 2), np.float32, 20), ramp((8, 2), np.float64, 21)
SPECIN = ramp((2, 4, 8, 2), np.float32, 22)
XC, XCB, XC128 = ramp((16,), np.complex64, 23), ramp((2, 16), np.complex64, 24), ramp((16,), np.complex128, 25)
INC, NEG, NEG_I = np.array([11, 22], np.uint32), [True, False], np.array([1, 0], np.int32)
MODES = np.array([EPI_FM, EPI_AM], np.intc)
BAUDS, BMODES = np.array([1200.0, 300.0], np.float32), np.array([1, 0], np.intc)
# what the wrappers make of the above
X3, ROW16_1, ROWR_1, SYM_1, SPEC_1, KERNS = X16[:, :3], ROW16[None], ROWR[None], SYM[:1], SPECIN[:1], np.stack([KERN, KERN2])
FIVES = np.full((2, 16), 5, np.int16)
DB_KINDS, DB_LENS, DB_INV, DB_ASK = (np.array(v, np.intc) for v in ([abi.DET_FSK, abi.DET_ASK], [4, 0], [0, 1], [abi.DET_ASK] * 2))


def case_designers(r):
    n = nodes
    r.ret("iqbb_taps", n.design_iqbb_taps(100e3, 50e3, 2.4e6, 5))
    r.ret("bb_taps", n.design_bb_taps(100e3, 50e3, 2.4e6, 5))
    r.ret("decim", n.design_iqbb_decim(2.4e6, 8))
    r.ret("lut16", n.design_freqshift_lut_i16())
    r.ret("lut8", n.design_freqshift_lut_i8())
    r.ret("inc", n.design_freqshift_inc(100e3, 2.4e6))
    r.ret("lowpass", n.design_fir_lowpass(5, 100e3, 2.4e6))
    r.ret("alpha", n.design_fmdeemph_alpha(48e3))
    r.ret("kern", n.design_fftfilt_kernel(8, 50e3, 150e3, 2.4e6))
    r.ret("kern64", n.design_fftfilt_kernel(8, 50e3, 150e3, 2.4e6, dtype=np.float64))
    r.ret("spec", n.design_fftfilt_spectrum(KERN))
    r.ret("spec64", n.design_fftfilt_spectrum(KERN64))
    r.ret("fsk_lut", n.design_fsk_lut(48e3, 1200.0, 2200.0))
    r.ret("devices", n.device_count())


def case_context(r):
    ctx = nodes.Context(0)
    r.ret("handle", r.fake.handles[ctx.handle.value])
    ctx.synchronize()
    r.ret("name", ctx.device_name())
    p = ctx.malloc(64)
    r.ret("malloc", p)
    ctx.h2d(p, XR16)
    ctx.d2h(np.zeros_like(XR16), p)
    ctx.memset(p, 0, 64)
    ctx.free(p)
    ctx.close()
    ctx.close()
    s = nodes.Context(1, stream=0x5000)
    r.ret("device", s.device)
    s.close()
    for handle in (C.c_void_p(0xB000), 0xB100):     # a borrowed context runs the hooks and is not destroyed
        b = nodes.Context.borrowed(handle, 1)
        b.synchronize()
        b.close()
        b.close()


def case_timer(r):
    ctx = r.ctx()
    t = nodes.Timer(ctx)
    t.start()
    t.stop()
    r.ret("ms", t.elapsed_ms())
    t.__del__()
    t.__del__()
    ctx.close()


def case_iqbb_i16(r):
    ctx = r.ctx()
    node = nodes.IQBaseBandI16(ctx, TAPS, LUT, 1234, True, 4, channels=2, max_in=64)
    fm = nodes.IQBaseBandI16(ctx, TAPS2, LUT, 4321, False, 4, channels=2, max_in=64, epilogue=EPI_FM)
    r.ret("attrs", (node.channels, node.decim, node.epilogue, node.max_in, fm.epilogue))
    r.ret("path", node.path)
    r.ret("kernel_names", node.kernel_names)
    r.ret("plan_info", node.plan_info)
    r.ret("out_count", node.out_count(16))
    r.ret("process_dev", node.process_dev(0x1000, 16, 19, 0x2000, 7))
    r.ret("process_dev_multi", node.process_dev_multi(0x1000, 2, 10, 23, 0x2000, 8))
    node.reset()
    node.reset(keep_history=True, keep_fm=True)
    node.adopt_state(fm, abi.KEEP_RING | abi.KEEP_FM)
    node.set_taps(TAPS2)
    node.set_shift(99, False)
    r.three("process", node, X16, X16[:, :0])
    r.three("fm", fm, X16, X16[:, :0])
    r.route(True)
    r.ret("n=3", node.process(X16[:, :3]))          # n_in != 0, no output: the router is not met
    r.ret("multi/routed", node.process_multi(X16, 2))
    r.route(False)
    r.ret("multi", node.process_multi(X16, 2))
    node.set_input_format(abi.IN_CU8)
    r.ret("cu8", node.process(XU8))
    r.ret("cu8/multi", node.process_multi(XU8, 2))
    node.set_input_format(abi.IN_CS16)
    r.ret("cs16", node.process(X16))
    for o in (node, node, fm, ctx):
        o.close()


def case_bb_i16(r):
    ctx = r.ctx()
    node = nodes.BaseBandI16(ctx, TAPS, LUT, 1234, True, 4, channels=2, max_in=64)
    r.ret("attrs", (node.channels, node.decim, node.epilogue, node.max_in))
    r.three("process", node, XR16, XR16[:, :0])
    r.ret("multi", node.process_multi(XR16, 2))
    r.route(True)
    r.ret("multi/routed", node.process_multi(XR16, 2))
    r.route(False)
    one = nodes.BaseBandI16(ctx, TAPS, LUT, 1234, False, 4, max_in=64, epilogue=EPI_FM)
    r.ret("1-D", one.process(ROWR))
    for o in (node, node, one, ctx):
        o.close()


def case_iqbb_i8(r):
    ctx = r.ctx()
    node = nodes.IQBaseBandI8(ctx, TAPS, LUT, 1234, True, 4, channels=2, max_in=64)
    r.ret("attrs", (node.channels, node.decim, node.epilogue, node.max_in))
    r.three("process", node, XI8, XI8[:, :0])
    fm = nodes.IQBaseBandI8(ctx, TAPS, LUT, 1234, False, 4, channels=2, max_in=64, epilogue=EPI_FM)
    r.ret("fm", fm.process(XI8))
    for o in (node, node, fm, ctx):
        o.close()


def case_tuner(r):
    ctx = r.ctx()
    bank = nodes.TunerBankI16(ctx, BTAPS, LUT, [11, 22], NEG, 4, max_in=64)
    r.ret("attrs", (bank.channels, bank.order, bank.decim, bank.epilogue, bank.max_in, bank.real))
    r.ret("kernel_names", bank.kernel_names)
    r.ret("plan_info", bank.plan_info(16))
    r.ret("out_count", bank.out_count(16))
    r.ret("process_dev", bank.process_dev(0x1000, 16, 0x2000, 7))
    bank.set_taps(1, TAPS2)
    bank.set_shift(1, 99, True)
    bank.reset()
    bank.reset(keep_history=True, keep_fm=True)
    r.three("process", bank, ROW16, ROW16[:0])
    bank.set_input_format(abi.IN_CU8)
    r.ret("cu8", bank.process(ROWU8))
    bank.set_input_format(abi.IN_CS16)
    bank.close()
    bank.close()
    modes = nodes.TunerBankI16(ctx, BTAPS, LUT, [11, 22], NEG, 4, max_in=64, modes=[EPI_FM, EPI_AM])
    r.ret("modes/epilogue", modes.epilogue)
    modes.set_mode(1, abi.EPI_USB)
    r.ret("modes", modes.modes())
    r.three("modes/process", modes, ROW16, ROW16[:0])
    modes.close()
    real = nodes.TunerBankI16(ctx, BTAPS, LUT, [11, 22], NEG, 4, max_in=64, epilogue=EPI_AM, real=True)
    r.three("real/process", real, ROWR, ROWR[:0])
    real.close()
    both = nodes.TunerBankI16(ctx, BTAPS, LUT, [11, 22], NEG, 4, max_in=64, modes=[EPI_FM, EPI_AM], real=True)
    r.ret("real+modes", (both.real, both.epilogue, R(both.process(ROWR))))
    both.close()
    ctx.close()


def case_fir(r):
    ctx = r.ctx()
    node = nodes.FIR(ctx, abi.FIR_CS16_EXACT, ALPHA, decim=4, channels=2, max_in=64)
    r.ret("attrs", (node.kind, node.channels, node.decim, node.epilogue, node.order))
    r.ret("kernel_names", (node.kernel_names(), node.kernel_names(16)))
    r.ret("last_kernels", node.last_kernels())
    r.ret("out_count", node.out_count(16))
    r.ret("process_dev", node.process_dev(0x1000, 16, 19, 0x2000, 7))
    node.reset()
    node.set_taps(ALPHA2)
    r.three("process", node, X16, X16[:, :0])
    r.route(True)
    r.ret("n=3", node.process(X16[:, :3]))
    f32 = nodes.FIR(ctx, abi.FIR_CF32, ALPHA, channels=2, max_in=64, epilogue=EPI_FM)
    r.ret("cf32/routed", f32.process(XF32))
    for o in (node, node, f32, ctx):
        o.close()


def case_demod(r):
    ctx = r.ctx()
    node = nodes.Demod(ctx, EPI_FM, channels=2, max_in=64)
    r.ret("attrs", (node.kind, node.dtype, node.channels))
    node.process_dev(0x1000, 16, 19, 0x2000, 19)
    node.reset()
    r.three("process", node, X16, X16[:, :0])
    r.route(True)
    out = FIVES.copy()
    r.ret("out=", node.process(X16, out=out) is out)   # a caller's out never meets the router
    r.route(False)
    f32 = nodes.Demod(ctx, EPI_AM, abi.T_CF32, channels=2, max_in=64, inplace_fm0=False)
    r.ret("cf32", f32.process(XF32))
    i8 = nodes.Demod(ctx, EPI_FM, abi.T_CS8, channels=2, max_in=64)
    r.ret("cs8", i8.process(XI8))
    for o in (node, node, f32, i8, ctx):
        o.close()


def case_deemph(r):
    ctx = r.ctx()
    node = nodes.FMDeemphI16(ctx, 4, channels=2, max_in=64)
    r.ret("kernel_names", (node.kernel_names(), node.kernel_names(16)))
    node.process_dev(0x1000, 16, 19, 0x2000, 19)
    node.reset()
    r.three("process", node, XR16, XR16[:, :0])
    r.ret("1-D", node.process(ROWR))
    for o in (node, node, ctx):
        o.close()


def case_detector(r):
    ctx = r.ctx()
    node = nodes.SymbolDetector(ctx, abi.DET_FSK, MARK, SPACE, channels=2, max_in=64)
    r.ret("attrs", (node.kind, node.channels))
    r.ret("kernel_names", node.kernel_names)
    node.process_dev(0x1000, 16, 19, 0x2000, 19)
    node.reset()
    r.three("process", node, XR16, XR16[:, :0])
    ask = nodes.SymbolDetector(ctx, abi.DET_ASK, invert=True, max_in=64)
    r.ret("ask/1-D", ask.process(ROWR))
    fsk = nodes.FSKDetector(ctx, 48e3, 1200.0, 1200.0, 2200.0, channels=2, max_in=64)
    pinned = nodes.FSKDetector(ctx, 48e3, 1200.0, 1200.0, 2200.0, channels=2, max_in=64, mark_lut=MARK, space_lut=SPACE)
    r.ret("fsk", (fsk.kind, pinned.kind, R(pinned.process(XR16))))
    ask2 = nodes.ASKDetector(ctx, True, channels=2, max_in=64)
    r.ret("ask", (ask2.kind, R(ask2.process(XR16))))
    for o in (node, node, ask, fsk, pinned, ask2, ctx):
        o.close()


def case_bits(r):
    ctx = r.ctx()
    node = nodes.BitStream(ctx, 48e3, 1200.0, channels=2, max_in=64)
    r.ret("corr_len", node.corr_len)
    r.ret("out_capacity", node.out_capacity(16))
    r.ret("kernel_names", node.kernel_names)
    node.process_dev(0x1000, 16, 19, 0x2000, 7, 0x3000)
    node.reset()
    r.ret("process_raw", node.process_raw(SYM))
    r.three("process", node, SYM, SYM[:, :0])       # the routed call allocates the device counts, close() frees them
    normal = nodes.BitStream(ctx, 48e3, 300.0, abi.BITS_NORMAL, max_in=64)
    r.ret("1-D", normal.process(SYM[0]))
    for o in (node, node, normal, ctx):
        o.close()


def case_detectorbank(r):
    ctx = r.ctx()
    bank = nodes.SymbolDetectorBank(ctx, [("fsk", MARK, SPACE), ("ask", True)], max_in=64, max_corr_len=8)
    r.ret("attrs", (bank.channels, bank.kind))
    r.ret("kernel_names", bank.kernel_names)
    r.three("process", bank, XR16, XR16[:, :0])
    bank.set_channel(0, ("ask",))
    bank.set_channel(1, (abi.DET_FSK, MARK, SPACE))
    bank.process_dev(0x1000, 16, 19, 0x2000, 19)
    bank.reset()
    asks = nodes.SymbolDetectorBank(ctx, [(abi.DET_ASK, False), ("ask",)], max_in=64)
    for o in (bank, bank, asks, ctx):
        o.close()


def case_bitsbank(r):
    ctx = r.ctx()
    bank = nodes.BitStreamBank(ctx, 48e3, [1200.0, 300.0], [1, 0], max_in=64, max_corr_len=8)
    r.ret("attrs", (bank.channels, bank.corr_len, bank.out_capacity(16), bank.kernel_names))
    bank.set_channel(1, 600.0)
    bank.set_channel(0, 600.0, abi.BITS_NORMAL)
    r.ret("channel_info", (bank.channel_info(0), bank.channel_info(1, 16)))
    r.three("process", bank, SYM, SYM[:, :0])
    r.ret("process_raw", bank.process_raw(SYM))
    bank.process_dev(0x1000, 16, 19, 0x2000, 7, 0x3000)
    bank.reset()
    for o in (bank, bank, ctx):
        o.close()


def case_subsample(r):
    ctx = r.ctx()
    node = nodes.SubSample(ctx, abi.T_CS16, 4, channels=2, max_in=64)
    r.ret("attrs", (node.dtype, node.n, node.channels))
    r.ret("out_count", node.out_count(16))
    r.ret("process_dev", node.process_dev(0x1000, 16, 19, 0x2000, 7))
    node.reset()
    r.three("process", node, X16, X16[:, :0])
    f32 = nodes.SubSample(ctx, abi.T_CF32, 4, channels=2, max_in=64)
    r.ret("cf32", f32.process(XF32))
    for o in (node, node, f32, ctx):
        o.close()


def case_fftconv(r):
    ctx = r.ctx()
    node = nodes.FFTConv(ctx, abi.FFTCONV_OLS, 16, KERN, channels=2, max_in=64)
    r.ret("attrs", (node.mode, node.fft_size, node.channels, node.bands, node.dtype == np.float32, node.f64))
    node.set_kernel(0, KERN2)
    node.process_dev(0x1000, 16, 19, 0x2000, 19)
    r.ret("last_kernels", node.last_kernels())
    node.reset()
    r.three("process", node, XF32, XF32[:, :0])
    bank = nodes.FFTConv(ctx, abi.FFTCONV_OLA, 8, [KERN, KERN2], channels=2, max_in=64)
    r.three("bank", bank, XF32, XF32[:, :0])        # the router sees the band-major rows [bands * channels, n, 2]
    f64 = nodes.FFTConv(ctx, abi.FFTCONV_OLA, 8, KERN64, channels=2, max_in=64, dtype=np.float64)
    r.ret("f64/attrs", (f64.bands, f64.dtype == np.float64, f64.f64))
    f64.set_kernel(0, KERN64)
    f64.process_dev(0x1000, 16, 19, 0x2000, 19)
    r.three("f64", f64, XF64, XF64[:, :0])
    for o in (node, node, bank, f64, ctx):
        o.close()


def case_fftsplit(r):
    ctx = r.ctx()
    sink = nodes.FFTSink(ctx, 4, channels=2, max_blocks=8)
    r.ret("sink/attrs", (sink.N, sink.channels, sink.dtype == np.float32, sink.form))
    sink.process_dev(0x1000, 16, 19, 0x2000, 70)
    r.three("sink", sink, XF32, XF32[:, :0])        # FFTSink and FFTSource never meet the router
    sink64 = nodes.FFTSink(ctx, 4, channels=2, max_blocks=8, dtype=np.float64)
    r.ret("sink64", sink64.process(XF64))
    src = nodes.FFTSource(ctx, 4, KERN, channels=2, max_blocks=8)
    r.ret("source/attrs", (src.N, src.channels, src.dtype == np.float32, src.form))
    src.process_dev(0x1000, 4, 70, 0x2000, 19)
    src.set_kernel(KERN2)
    src.reset()
    r.three("source", src, SPECIN, SPECIN[:, :0])
    r.ret("source/3-D", src.process(SPECIN[0]))
    src64 = nodes.FFTSource(ctx, 4, KERN64, channels=2, max_blocks=8, dtype=np.float64)
    for o in (sink, sink, sink64, src, src, src64, ctx):
        o.close()


def case_fbb(r):
    ctx = r.ctx()
    node = nodes.FloatBaseBand(ctx, 100e3, 2.4e6, ALPHA, 4, channels=2, max_in=64)
    r.ret("attrs", (node.channels, node.decim, node.order))
    r.ret("kernel_names", (node.kernel_names(), node.kernel_names(16)))
    r.ret("last_kernels", node.last_kernels())
    r.ret("out_count", node.out_count(16))
    r.ret("process_dev", node.process_dev(0x1000, 16, 19, 0x2000, 7))
    node.reset()
    node.set_taps(ALPHA2)
    node.set_shift(50000)
    r.three("process", node, XF32, XF32[:, :0])
    for o in (node, node, ctx):
        o.close()


def case_fft(r):
    ctx = r.ctx()
    r.ret("c2c", nodes.fft_c2c(ctx, XF32, -1))
    r.ret("c2c_f64", nodes.fft_c2c_f64(ctx, XF64, 1))
    r.ret("exec", A(nodes.fft_exec(ctx, XC, -1))[:2])       # (np.empty: dtype and shape only)
    r.ret("exec128", A(nodes.fft_exec(ctx, XC128, 1))[:2])
    plan = nodes.FFTPlan(ctx, 16)
    r.ret("plan/attrs", (plan.n, plan.dtype == np.complex64, plan.form))
    r.ret("plan/exec", A(plan.exec(XC, -1))[:2])
    r.ret("plan/exec_batch", A(plan.exec_batch(XCB, 1))[:2])
    plan128 = nodes.FFTPlan(ctx, 16, np.complex128)
    for o in (plan, plan, plan128, ctx):
        o.close()


def case_comm(r):
    comm = nodes.Comm([0, 1])
    r.ret("attrs", (comm.devices, [(r.h(c), c.device) for c in comm.ctx], comm.transport))
    comm.broadcast([0x1000, 0x2000], 64)
    comm.gather([0x1000, 0x2000], [64, 32], 0x3000, root=1)
    comm.gather_begin(1, [0x1000, 0x2000], [64, 32], 0x3000)
    comm.gather_wait(1)
    comm.synchronize()
    comm.close()
    comm.close()


CASES = {f.__name__[5:]: f for f in (case_designers, case_context, case_timer, case_iqbb_i16, case_bb_i16, case_iqbb_i8, case_tuner,
                                     case_fir, case_demod, case_deemph, case_detector, case_bits, case_detectorbank, case_bitsbank,
                                     case_subsample, case_fftconv, case_fftsplit, case_fbb, case_fft, case_comm)}

# The call lists, written against the wrappers' code: what each case above must make the library see, in order.
EXPECT = {}

EXPECT["designers"] = [
    ("sdrhip_design_iqbb_taps", 100000.0, 50000.0, 2400000.0, 5, Z(40)),
    ("ret", "iqbb_taps", ("<i4", (5, 2), "zeros")),
    ("sdrhip_design_bb_taps", 100000.0, 50000.0, 2400000.0, 5, Z(40)),
    ("ret", "bb_taps", ("<i4", (5, 2), "zeros")),
    ("sdrhip_design_iqbb_decim", 2400000.0, 8, 0.0, OUT_I),
    ("ret", "decim", 7),
    ("sdrhip_design_freqshift_lut_i16", Z(1024)),
    ("ret", "lut16", ("<i4", (128, 2), "zeros")),
    ("sdrhip_design_freqshift_lut_i8", Z(1024)),
    ("ret", "lut8", ("<i4", (128, 2), "zeros")),
    ("sdrhip_design_freqshift_inc", 100000.0, 2400000.0, ("out", "c_uint")),
    ("ret", "inc", 7),
    ("sdrhip_design_fir_lowpass", 5, 100000.0, 2400000.0, Z(40)),
    ("ret", "lowpass", ("<f8", (5,), "zeros")),
    ("sdrhip_design_fmdeemph_alpha", 48000.0, OUT_I),
    ("ret", "alpha", 7),
    ("sdrhip_design_fftfilt_kernel", 8, 50000.0, 150000.0, 2400000.0, Z(64)),
    ("ret", "kern", ("<f4", (8, 2), "zeros")),
    ("sdrhip_design_fftfilt_kernel_f64", 8, 50000.0, 150000.0, 2400000.0, Z(128)),
    ("ret", "kern64", ("<f8", (8, 2), "zeros")),
    ("sdrhip_design_fftfilt_spectrum", 8, B(KERN), Z(128)),
    ("ret", "spec", ("<f4", (16, 2), "zeros")),
    ("sdrhip_design_fftfilt_spectrum_f64", 8, B(KERN64), Z(256)),
    ("ret", "spec64", ("<f8", (16, 2), "zeros")),
    ("sdrhip_design_fsk_lut", 48000.0, 1200.0, 2200.0, OUT_I, None, 0),
    ("sdrhip_design_fsk_lut", 48000.0, 1200.0, 2200.0, OUT_I, Z(56), 7),
    ("ret", "fsk_lut", ("<f4", (7, 2), "zeros")),
    ("sdrhip_device_count", OUT_I),
    ("ret", "devices", 7),
]

EXPECT["context"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("ret", "handle", "h1"),
    ("sdrhip_ctx_synchronize", "h1"),
    ("sdrhip_ctx_device_name", "h1", ("buf", 256), 256),
    ("ret", "name", "k_main<1,2>,k_tail"),
    ("sdrhip_malloc", "h1", 64, OUT_VP),
    ("ret", "malloc", 0xd1000),
    ("sdrhip_memcpy_h2d", "h1", 0xd1000, A(XR16), 64),
    ("sdrhip_memcpy_d2h", "h1", ("<i2", (2, 16), "zeros"), 0xd1000, 64),
    ("sdrhip_memset", "h1", 0xd1000, 0, 64),
    ("sdrhip_free", "h1", 0xd1000),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
    ("sdrhip_ctx_create", 1, 0x5000, OUT_VP),
    ("ret", "device", 1),
    ("hook", "h2"),
    ("sdrhip_ctx_destroy", "h2"),
    ("sdrhip_ctx_synchronize", 0xb000),
    ("hook", 0xb000),
    ("sdrhip_ctx_synchronize", 0xb100),
    ("hook", 0xb100),
]

EXPECT["timer"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_timer_create", "h1", OUT_VP),
    ("sdrhip_timer_start", "h2"),
    ("sdrhip_timer_stop", "h2"),
    ("sdrhip_timer_elapsed_ms", "h2", ("out", "c_float")),
    ("ret", "ms", 7.0),
    ("sdrhip_timer_destroy", "h2"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["iqbb_i16"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_iqbb_i16_create", "h1", B(TAPS), 5, B(LUT), 1234, 1, 4, 2, 64, 0, OUT_VP),
    ("sdrhip_iqbb_i16_create", "h1", B(TAPS2), 5, B(LUT), 4321, 0, 4, 2, 64, 1, OUT_VP),
    ("ret", "attrs", (2, 4, 0, 64, 1)),
    ("sdrhip_iqbb_i16_path", "h2", OUT_I),
    ("ret", "path", 7),
    ("sdrhip_iqbb_i16_kernel_names", "h2", ("buf", 256), 256),
    ("ret", "kernel_names", NAMES),
    ("sdrhip_iqbb_i16_plan_info", "h2", ("c_int", [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]), 11),
    ("ret", "plan_info", {'path': 1, 'S': 2, 'S0': 3, 'NH': 4, 'NW': 5, 'kind': 6, 'OP': 7, 'HH': 8, 'multi_left': 9, 'L0': 10, 'NL': 11}),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("ret", "out_count", 4),
    ("sdrhip_iqbb_i16_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process_dev", 4),
    ("sdrhip_iqbb_i16_process_dev_multi", "h2", 4096, 2, 10, 23, 0x2000, 8, ("c_ulong", [0, 0]), OUT_SZ),
    ("ret", "process_dev_multi", [2, 3]),
    ("sdrhip_iqbb_i16_reset", "h2", 0),
    ("sdrhip_iqbb_i16_reset", "h2", 3),
    ("sdrhip_iqbb_i16_adopt_state", "h2", "h3", 3),
    ("sdrhip_iqbb_i16_set_taps", "h2", B(TAPS2)),
    ("sdrhip_iqbb_i16_set_shift", "h2", 99, 0),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", A(X16), 16, 16, ("<i2", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "process", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(X16), ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process/routed", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 0, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", ("<i2", (2, 0, 2), "zeros"), 0, 0, ("<i2", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "process/empty", ("<i2", (2, 0, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h3", 16, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h3", A(X16), 16, 16, ("<i2", (2, 4), "zeros"), 4, OUT_SZ),
    ("ret", "fm", ("<i2", (2, 4), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h3", 16, OUT_SZ),
    ("router", "h1", A(X16), ("<i2", (2, 4), "zeros")),
    ("sdrhip_iqbb_i16_process_dev", "h3", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "fm/routed", ("<i2", (2, 4), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h3", 0, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h3", ("<i2", (2, 0, 2), "zeros"), 0, 0, ("<i2", (2, 0), "zeros"), 0, OUT_SZ),
    ("ret", "fm/empty", ("<i2", (2, 0), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 3, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", A(X3), 3, 3, ("<i2", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "n=3", ("<i2", (2, 0, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(X16), ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_process_dev_multi", "h2", 4096, 2, 8, 19, 0x2000, 7, ("c_ulong", [0, 0]), OUT_SZ),
    ("ret", "multi/routed", (("<i2", (2, 4, 2), "zeros"), [2, 2])),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_malloc", "h1", 128, OUT_VP),
    ("sdrhip_malloc", "h1", 32, OUT_VP),
    ("sdrhip_memcpy_h2d", "h1", 0xd1000, A(X16), 128),
    ("sdrhip_memcpy_h2d", "h1", 0xd2000, ("<i2", (2, 4, 2), "zeros"), 32),
    ("sdrhip_iqbb_i16_process_dev_multi", "h2", 0xd1000, 2, 8, 16, 0xd2000, 4, ("c_ulong", [0, 0]), OUT_SZ),
    ("sdrhip_ctx_synchronize", "h1"),
    ("sdrhip_memcpy_d2h", "h1", ("<i2", (2, 4, 2), "zeros"), 0xd2000, 32),
    ("sdrhip_free", "h1", 0xd1000),
    ("sdrhip_free", "h1", 0xd2000),
    ("ret", "multi", (("<i2", (2, 4, 2), "zeros"), [2, 2])),
    ("sdrhip_iqbb_i16_set_input_format", "h2", 1),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", A(XU8), 16, 16, ("<i2", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "cu8", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_malloc", "h1", 64, OUT_VP),
    ("sdrhip_malloc", "h1", 32, OUT_VP),
    ("sdrhip_memcpy_h2d", "h1", 0xd3000, A(XU8), 64),
    ("sdrhip_memcpy_h2d", "h1", 0xd4000, ("<i2", (2, 4, 2), "zeros"), 32),
    ("sdrhip_iqbb_i16_process_dev_multi", "h2", 0xd3000, 2, 8, 16, 0xd4000, 4, ("c_ulong", [0, 0]), OUT_SZ),
    ("sdrhip_ctx_synchronize", "h1"),
    ("sdrhip_memcpy_d2h", "h1", ("<i2", (2, 4, 2), "zeros"), 0xd4000, 32),
    ("sdrhip_free", "h1", 0xd3000),
    ("sdrhip_free", "h1", 0xd4000),
    ("ret", "cu8/multi", (("<i2", (2, 4, 2), "zeros"), [2, 2])),
    ("sdrhip_iqbb_i16_set_input_format", "h2", 0),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", A(X16), 16, 16, ("<i2", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "cs16", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_destroy", "h2"),
    ("sdrhip_iqbb_i16_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["bb_i16"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_bb_i16_create", "h1", B(TAPS), 5, B(LUT), 1234, 1, 4, 2, 64, 0, OUT_VP),
    ("ret", "attrs", (2, 4, 0, 64)),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", A(XR16), 16, 16, ("<i2", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "process", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(XR16), ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process/routed", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 0, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", ("<i2", (2, 0), "zeros"), 0, 0, ("<i2", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "process/empty", ("<i2", (2, 0, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_malloc", "h1", 64, OUT_VP),
    ("sdrhip_malloc", "h1", 32, OUT_VP),
    ("sdrhip_memcpy_h2d", "h1", 0xd1000, A(XR16), 64),
    ("sdrhip_memcpy_h2d", "h1", 0xd2000, ("<i2", (2, 4, 2), "zeros"), 32),
    ("sdrhip_iqbb_i16_process_dev_multi", "h2", 0xd1000, 2, 8, 16, 0xd2000, 4, ("c_ulong", [0, 0]), OUT_SZ),
    ("sdrhip_ctx_synchronize", "h1"),
    ("sdrhip_memcpy_d2h", "h1", ("<i2", (2, 4, 2), "zeros"), 0xd2000, 32),
    ("sdrhip_free", "h1", 0xd1000),
    ("sdrhip_free", "h1", 0xd2000),
    ("ret", "multi", (("<i2", (2, 4, 2), "zeros"), [2, 2])),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(XR16), ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_process_dev_multi", "h2", 4096, 2, 8, 19, 0x2000, 7, ("c_ulong", [0, 0]), OUT_SZ),
    ("ret", "multi/routed", (("<i2", (2, 4, 2), "zeros"), [2, 2])),
    ("sdrhip_bb_i16_create", "h1", B(TAPS), 5, B(LUT), 1234, 0, 4, 1, 64, 1, OUT_VP),
    ("sdrhip_iqbb_i16_out_count", "h3", 16, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h3", A(ROWR_1), 16, 16, ("<i2", (1, 4), "zeros"), 4, OUT_SZ),
    ("ret", "1-D", ("<i2", (1, 4), "zeros")),
    ("sdrhip_iqbb_i16_destroy", "h2"),
    ("sdrhip_iqbb_i16_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["iqbb_i8"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_iqbb_i8_create", "h1", B(TAPS), 5, B(LUT), 1234, 1, 4, 2, 64, 0, OUT_VP),
    ("ret", "attrs", (2, 4, 0, 64)),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", A(XI8), 16, 16, ("|i1", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "process", ("|i1", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(XI8), ("|i1", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process/routed", ("|i1", (2, 4, 2), "zeros")),
    ("sdrhip_iqbb_i16_out_count", "h2", 0, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h2", ("|i1", (2, 0, 2), "zeros"), 0, 0, ("|i1", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "process/empty", ("|i1", (2, 0, 2), "zeros")),
    ("sdrhip_iqbb_i8_create", "h1", B(TAPS), 5, B(LUT), 1234, 0, 4, 2, 64, 1, OUT_VP),
    ("sdrhip_iqbb_i16_out_count", "h3", 16, OUT_SZ),
    ("sdrhip_iqbb_i16_process", "h3", A(XI8), 16, 16, ("<i2", (2, 4), "zeros"), 4, OUT_SZ),
    ("ret", "fm", ("<i2", (2, 4), "zeros")),
    ("sdrhip_iqbb_i16_destroy", "h2"),
    ("sdrhip_iqbb_i16_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["tuner"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_tuner_i16_create", "h1", B(BTAPS), 5, B(LUT), B(INC), B(BMODES), 4, 2, 64, 0, OUT_VP),
    ("ret", "attrs", (2, 5, 4, 0, 64, False)),
    ("sdrhip_tuner_i16_kernel_names", "h2", ("buf", 256), 256),
    ("ret", "kernel_names", NAMES),
    ("sdrhip_tuner_i16_plan_info", "h2", 16, ("c_int", [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]), 10),
    ("ret", "plan_info", {'hot': 1, 'S': 2, 'CG': 3, 'OG': 4, 'tiles': 5, 'ctiles': 6, 'ctw': 7, 'grid_y': 8, 'PLB': 9, 'lds': 10}),
    ("sdrhip_tuner_i16_out_count", "h2", 16, OUT_SZ),
    ("ret", "out_count", 4),
    ("sdrhip_tuner_i16_process_dev", "h2", 4096, 16, 0x2000, 7, OUT_SZ),
    ("ret", "process_dev", 4),
    ("sdrhip_tuner_i16_set_taps", "h2", 1, B(TAPS2)),
    ("sdrhip_tuner_i16_set_shift", "h2", 1, 99, 1),
    ("sdrhip_tuner_i16_reset", "h2", 0),
    ("sdrhip_tuner_i16_reset", "h2", 3),
    ("sdrhip_tuner_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_tuner_i16_process", "h2", A(ROW16), 16, ("<i2", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "process", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_tuner_i16_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(ROW16_1), ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_tuner_i16_process_dev", "h2", 4096, 16, 0x2000, 7, OUT_SZ),
    ("ret", "process/routed", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_tuner_i16_out_count", "h2", 0, OUT_SZ),
    ("sdrhip_tuner_i16_process", "h2", ("<i2", (0, 2), "zeros"), 0, ("<i2", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "process/empty", ("<i2", (2, 0, 2), "zeros")),
    ("sdrhip_tuner_i16_set_input_format", "h2", 1),
    ("sdrhip_tuner_i16_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_tuner_i16_process", "h2", A(ROWU8), 16, ("<i2", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "cu8", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_tuner_i16_set_input_format", "h2", 0),
    ("sdrhip_tuner_i16_destroy", "h2"),
    ("sdrhip_tunermodes_i16_create", "h1", B(BTAPS), 5, B(LUT), B(INC), B(BMODES), B(MODES), 4, 2, 64, OUT_VP),
    ("ret", "modes/epilogue", 1),
    ("sdrhip_tunermodes_i16_set_mode", "h3", 1, 3),
    ("sdrhip_tunermodes_i16_get_modes", "h3", ("c_int", [0, 0]), 2),
    ("ret", "modes", [1, 2]),
    ("sdrhip_tuner_i16_out_count", "h3", 16, OUT_SZ),
    ("sdrhip_tuner_i16_process", "h3", A(ROW16), 16, ("<i2", (2, 4), "zeros"), 4, OUT_SZ),
    ("ret", "modes/process", ("<i2", (2, 4), "zeros")),
    ("sdrhip_tuner_i16_out_count", "h3", 16, OUT_SZ),
    ("router", "h1", A(ROW16_1), ("<i2", (2, 4), "zeros")),
    ("sdrhip_tuner_i16_process_dev", "h3", 4096, 16, 0x2000, 7, OUT_SZ),
    ("ret", "modes/process/routed", ("<i2", (2, 4), "zeros")),
    ("sdrhip_tuner_i16_out_count", "h3", 0, OUT_SZ),
    ("sdrhip_tuner_i16_process", "h3", ("<i2", (0, 2), "zeros"), 0, ("<i2", (2, 0), "zeros"), 0, OUT_SZ),
    ("ret", "modes/process/empty", ("<i2", (2, 0), "zeros")),
    ("sdrhip_tuner_i16_destroy", "h3"),
    ("sdrhip_tunerbb_i16_create", "h1", B(BTAPS), 5, B(LUT), B(INC), B(BMODES), 4, 2, 64, 2, OUT_VP),
    ("sdrhip_tuner_i16_out_count", "h4", 16, OUT_SZ),
    ("sdrhip_tuner_i16_process", "h4", A(ROWR), 16, ("<i2", (2, 4), "zeros"), 4, OUT_SZ),
    ("ret", "real/process", ("<i2", (2, 4), "zeros")),
    ("sdrhip_tuner_i16_out_count", "h4", 16, OUT_SZ),
    ("router", "h1", A(ROWR_1), ("<i2", (2, 4), "zeros")),
    ("sdrhip_tuner_i16_process_dev", "h4", 4096, 16, 0x2000, 7, OUT_SZ),
    ("ret", "real/process/routed", ("<i2", (2, 4), "zeros")),
    ("sdrhip_tuner_i16_out_count", "h4", 0, OUT_SZ),
    ("sdrhip_tuner_i16_process", "h4", ("<i2", (0,), "zeros"), 0, ("<i2", (2, 0), "zeros"), 0, OUT_SZ),
    ("ret", "real/process/empty", ("<i2", (2, 0), "zeros")),
    ("sdrhip_tuner_i16_destroy", "h4"),
    ("sdrhip_tunermodes_bb_i16_create", "h1", B(BTAPS), 5, B(LUT), B(INC), B(BMODES), B(MODES), 4, 2, 64, OUT_VP),
    ("sdrhip_tuner_i16_out_count", "h5", 16, OUT_SZ),
    ("sdrhip_tuner_i16_process", "h5", A(ROWR), 16, ("<i2", (2, 4), "zeros"), 4, OUT_SZ),
    ("ret", "real+modes", (True, 1, ("<i2", (2, 4), "zeros"))),
    ("sdrhip_tuner_i16_destroy", "h5"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["fir"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_fir_create", "h1", 0, B(ALPHA), 5, 4, 2, 64, 0, OUT_VP),
    ("ret", "attrs", (0, 2, 4, 0, 5)),
    ("sdrhip_fir_kernel_names", "h2", 0, ("buf", 256), 256),
    ("sdrhip_fir_kernel_names", "h2", 16, ("buf", 256), 256),
    ("ret", "kernel_names", (NAMES, NAMES)),
    ("sdrhip_fir_last_kernels", "h2", ("buf", 4096), 4096),
    ("ret", "last_kernels", LAST),
    ("sdrhip_fir_out_count", "h2", 16, OUT_SZ),
    ("ret", "out_count", 4),
    ("sdrhip_fir_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process_dev", 4),
    ("sdrhip_fir_reset", "h2"),
    ("sdrhip_fir_set_taps", "h2", B(ALPHA2)),
    ("sdrhip_fir_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_fir_process", "h2", A(X16), 16, 16, ("<i2", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "process", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_fir_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(X16), ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_fir_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process/routed", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_fir_out_count", "h2", 0, OUT_SZ),
    ("sdrhip_fir_process", "h2", ("<i2", (2, 0, 2), "zeros"), 0, 0, ("<i2", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "process/empty", ("<i2", (2, 0, 2), "zeros")),
    ("sdrhip_fir_out_count", "h2", 3, OUT_SZ),
    ("sdrhip_fir_process", "h2", A(X3), 3, 3, ("<i2", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "n=3", ("<i2", (2, 0, 2), "zeros")),
    ("sdrhip_fir_create", "h1", 1, B(ALPHA), 5, 1, 2, 64, 1, OUT_VP),
    ("sdrhip_fir_out_count", "h3", 16, OUT_SZ),
    ("router", "h1", A(XF32), ("<f4", (2, 4), "zeros")),
    ("sdrhip_fir_process_dev", "h3", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "cf32/routed", ("<f4", (2, 4), "zeros")),
    ("sdrhip_fir_destroy", "h2"),
    ("sdrhip_fir_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["demod"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_demod_create", "h1", 1, 0, 2, 64, 1, OUT_VP),
    ("ret", "attrs", (1, 0, 2)),
    ("sdrhip_demod_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("sdrhip_demod_reset", "h2"),
    ("sdrhip_demod_process", "h2", A(X16), 16, 16, ("<i2", (2, 16), "zeros"), 16),
    ("ret", "process", ("<i2", (2, 16), "zeros")),
    ("router", "h1", A(X16), ("<i2", (2, 16), "zeros")),
    ("sdrhip_demod_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("ret", "process/routed", ("<i2", (2, 16), "zeros")),
    ("sdrhip_demod_process", "h2", ("<i2", (2, 0, 2), "zeros"), 0, 0, ("<i2", (2, 0), "zeros"), 0),
    ("ret", "process/empty", ("<i2", (2, 0), "zeros")),
    ("sdrhip_demod_process", "h2", A(X16), 16, 16, A(FIVES), 16),
    ("ret", "out=", True),
    ("sdrhip_demod_create", "h1", 2, 1, 2, 64, 0, OUT_VP),
    ("sdrhip_demod_process", "h3", A(XF32), 16, 16, ("<f4", (2, 16), "zeros"), 16),
    ("ret", "cf32", ("<f4", (2, 16), "zeros")),
    ("sdrhip_demod_create", "h1", 1, 2, 2, 64, 1, OUT_VP),
    ("sdrhip_demod_process", "h4", A(XI8), 16, 16, ("<i2", (2, 16), "zeros"), 16),
    ("ret", "cs8", ("<i2", (2, 16), "zeros")),
    ("sdrhip_demod_destroy", "h2"),
    ("sdrhip_demod_destroy", "h3"),
    ("sdrhip_demod_destroy", "h4"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["deemph"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_deemph_i16_create", "h1", 4, 2, 64, OUT_VP),
    ("sdrhip_deemph_i16_kernel_names", "h2", 0, ("buf", 256), 256),
    ("sdrhip_deemph_i16_kernel_names", "h2", 16, ("buf", 256), 256),
    ("ret", "kernel_names", (NAMES, NAMES)),
    ("sdrhip_deemph_i16_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("sdrhip_deemph_i16_reset", "h2"),
    ("sdrhip_deemph_i16_process", "h2", A(XR16), 16, 16, ("<i2", (2, 16), "zeros"), 16),
    ("ret", "process", ("<i2", (2, 16), "zeros")),
    ("router", "h1", A(XR16), ("<i2", (2, 16), "zeros")),
    ("sdrhip_deemph_i16_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("ret", "process/routed", ("<i2", (2, 16), "zeros")),
    ("sdrhip_deemph_i16_process", "h2", ("<i2", (2, 0), "zeros"), 0, 0, ("<i2", (2, 0), "zeros"), 0),
    ("ret", "process/empty", ("<i2", (2, 0), "zeros")),
    ("sdrhip_deemph_i16_process", "h2", A(ROWR_1), 16, 16, ("<i2", (1, 16), "zeros"), 16),
    ("ret", "1-D", ("<i2", (1, 16), "zeros")),
    ("sdrhip_deemph_i16_destroy", "h2"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["detector"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_detector_create", "h1", 0, B(MARK), B(SPACE), 4, 0, 2, 64, OUT_VP),
    ("ret", "attrs", (0, 2)),
    ("sdrhip_detector_kernel_names", "h2", ("buf", 256), 256),
    ("ret", "kernel_names", NAMES),
    ("sdrhip_detector_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("sdrhip_detector_reset", "h2"),
    ("sdrhip_detector_process", "h2", A(XR16), 16, 16, ("|u1", (2, 16), "zeros"), 16),
    ("ret", "process", ("|u1", (2, 16), "zeros")),
    ("router", "h1", A(XR16), ("|u1", (2, 16), "zeros")),
    ("sdrhip_detector_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("ret", "process/routed", ("|u1", (2, 16), "zeros")),
    ("sdrhip_detector_process", "h2", ("<i2", (2, 0), "zeros"), 0, 0, ("|u1", (2, 0), "zeros"), 0),
    ("ret", "process/empty", ("|u1", (2, 0), "zeros")),
    ("sdrhip_detector_create", "h1", 1, None, None, 0, 1, 1, 64, OUT_VP),
    ("sdrhip_detector_process", "h3", A(ROWR_1), 16, 16, ("|u1", (1, 16), "zeros"), 16),
    ("ret", "ask/1-D", ("|u1", (1, 16), "zeros")),
    ("sdrhip_design_fsk_lut", 48000.0, 1200.0, 1200.0, OUT_I, None, 0),
    ("sdrhip_design_fsk_lut", 48000.0, 1200.0, 1200.0, OUT_I, Z(56), 7),
    ("sdrhip_design_fsk_lut", 48000.0, 1200.0, 2200.0, OUT_I, None, 0),
    ("sdrhip_design_fsk_lut", 48000.0, 1200.0, 2200.0, OUT_I, Z(56), 7),
    ("sdrhip_detector_create", "h1", 0, Z(56), Z(56), 7, 0, 2, 64, OUT_VP),
    ("sdrhip_detector_create", "h1", 0, B(MARK), B(SPACE), 4, 0, 2, 64, OUT_VP),
    ("sdrhip_detector_process", "h5", A(XR16), 16, 16, ("|u1", (2, 16), "zeros"), 16),
    ("ret", "fsk", (0, 0, ("|u1", (2, 16), "zeros"))),
    ("sdrhip_detector_create", "h1", 1, None, None, 0, 1, 2, 64, OUT_VP),
    ("sdrhip_detector_process", "h6", A(XR16), 16, 16, ("|u1", (2, 16), "zeros"), 16),
    ("ret", "ask", (1, ("|u1", (2, 16), "zeros"))),
    ("sdrhip_detector_destroy", "h2"),
    ("sdrhip_detector_destroy", "h3"),
    ("sdrhip_detector_destroy", "h4"),
    ("sdrhip_detector_destroy", "h5"),
    ("sdrhip_detector_destroy", "h6"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["bits"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_bits_create", "h1", 48000.0, 1200.0, 1, 2, 64, OUT_VP),
    ("sdrhip_bits_corr_len", "h2", OUT_I),
    ("ret", "corr_len", 7),
    ("sdrhip_bits_out_capacity", "h2", 16, OUT_SZ),
    ("ret", "out_capacity", 4),
    ("sdrhip_bits_kernel_names", "h2", ("buf", 256), 256),
    ("ret", "kernel_names", NAMES),
    ("sdrhip_bits_process_dev", "h2", 4096, 16, 19, 0x2000, 7, 0x3000),
    ("sdrhip_bits_reset", "h2"),
    ("sdrhip_bits_out_capacity", "h2", 16, OUT_SZ),
    ("sdrhip_bits_process", "h2", A(SYM), 16, 16, ("|u1", (2, 4), "zeros"), 4, ("<u4", (2,), "zeros")),
    ("ret", "process_raw", (("|u1", (2, 4), "zeros"), ("<u4", (2,), "zeros"))),
    ("sdrhip_bits_out_capacity", "h2", 16, OUT_SZ),
    ("sdrhip_bits_process", "h2", A(SYM), 16, 16, ("|u1", (2, 4), "zeros"), 4, ("<u4", (2,), "zeros")),
    ("ret", "process", [("|u1", (0,), "zeros"), ("|u1", (0,), "zeros")]),
    ("sdrhip_bits_out_capacity", "h2", 16, OUT_SZ),
    ("sdrhip_malloc", "h1", 8, OUT_VP),
    ("router", "h1", A(SYM), ("|u1", (2, 4), "zeros")),
    ("sdrhip_bits_process_dev", "h2", 4096, 16, 19, 0x2000, 7, 0xd1000),
    ("sdrhip_memcpy_d2h", "h1", ("<u4", (2,), "zeros"), 0xd1000, 8),
    ("ret", "process/routed", [("|u1", (0,), "zeros"), ("|u1", (0,), "zeros")]),
    ("sdrhip_bits_out_capacity", "h2", 0, OUT_SZ),
    ("sdrhip_bits_process", "h2", ("|u1", (2, 0), "zeros"), 0, 0, ("|u1", (2, 0), "zeros"), 0, ("<u4", (2,), "zeros")),
    ("ret", "process/empty", [("|u1", (0,), "zeros"), ("|u1", (0,), "zeros")]),
    ("sdrhip_bits_create", "h1", 48000.0, 300.0, 0, 1, 64, OUT_VP),
    ("sdrhip_bits_out_capacity", "h3", 16, OUT_SZ),
    ("sdrhip_bits_process", "h3", A(SYM_1), 16, 16, ("|u1", (1, 4), "zeros"), 4, ("<u4", (1,), "zeros")),
    ("ret", "1-D", [("|u1", (0,), "zeros")]),
    ("sdrhip_free", "h1", 0xd1000),
    ("sdrhip_bits_destroy", "h2"),
    ("sdrhip_bits_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["detectorbank"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_detectorbank_create", "h1", B(DB_INV), B(DB_LENS), B(DB_INV), B(MARK), B(SPACE), 8, 2, 64, OUT_VP),
    ("ret", "attrs", (2, None)),
    ("sdrhip_detector_kernel_names", "h2", ("buf", 256), 256),
    ("ret", "kernel_names", NAMES),
    ("sdrhip_detector_process", "h2", A(XR16), 16, 16, ("|u1", (2, 16), "zeros"), 16),
    ("ret", "process", ("|u1", (2, 16), "zeros")),
    ("router", "h1", A(XR16), ("|u1", (2, 16), "zeros")),
    ("sdrhip_detector_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("ret", "process/routed", ("|u1", (2, 16), "zeros")),
    ("sdrhip_detector_process", "h2", ("<i2", (2, 0), "zeros"), 0, 0, ("|u1", (2, 0), "zeros"), 0),
    ("ret", "process/empty", ("|u1", (2, 0), "zeros")),
    ("sdrhip_detectorbank_set_channel", "h2", 0, 1, None, None, 0, 0),
    ("sdrhip_detectorbank_set_channel", "h2", 1, 0, B(MARK), B(SPACE), 4, 0),
    ("sdrhip_detector_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("sdrhip_detector_reset", "h2"),
    ("sdrhip_detectorbank_create", "h1", B(DB_ASK), Z(8), Z(8), None, None, 0, 2, 64, OUT_VP),
    ("sdrhip_detector_destroy", "h2"),
    ("sdrhip_detector_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["bitsbank"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_bitsbank_create", "h1", 48000.0, B(BAUDS), B(BMODES), 2, 64, 8, OUT_VP),
    ("sdrhip_bits_corr_len", "h2", OUT_I),
    ("sdrhip_bits_out_capacity", "h2", 16, OUT_SZ),
    ("sdrhip_bits_kernel_names", "h2", ("buf", 256), 256),
    ("ret", "attrs", (2, 7, 4, NAMES)),
    ("sdrhip_bitsbank_set_channel", "h2", 1, 600.0, 1),
    ("sdrhip_bitsbank_set_channel", "h2", 0, 600.0, 0),
    ("sdrhip_bitsbank_channel_info", "h2", 0, 0, OUT_I, ("out", "c_float"), ("out", "c_float"), OUT_SZ),
    ("sdrhip_bitsbank_channel_info", "h2", 1, 16, OUT_I, ("out", "c_float"), ("out", "c_float"), OUT_SZ),
    ("ret", "channel_info", ({'corr_len': 7, 'omega_min': 7.0, 'omega_max': 7.0, 'capacity': 7}, {'corr_len': 7, 'omega_min': 7.0, 'omega_max': 7.0, 'capacity': 7})),
    ("sdrhip_bits_out_capacity", "h2", 16, OUT_SZ),
    ("sdrhip_bits_process", "h2", A(SYM), 16, 16, ("|u1", (2, 4), "zeros"), 4, ("<u4", (2,), "zeros")),
    ("ret", "process", [("|u1", (0,), "zeros"), ("|u1", (0,), "zeros")]),
    ("sdrhip_bits_out_capacity", "h2", 16, OUT_SZ),
    ("sdrhip_malloc", "h1", 8, OUT_VP),
    ("router", "h1", A(SYM), ("|u1", (2, 4), "zeros")),
    ("sdrhip_bits_process_dev", "h2", 4096, 16, 19, 0x2000, 7, 0xd1000),
    ("sdrhip_memcpy_d2h", "h1", ("<u4", (2,), "zeros"), 0xd1000, 8),
    ("ret", "process/routed", [("|u1", (0,), "zeros"), ("|u1", (0,), "zeros")]),
    ("sdrhip_bits_out_capacity", "h2", 0, OUT_SZ),
    ("sdrhip_bits_process", "h2", ("|u1", (2, 0), "zeros"), 0, 0, ("|u1", (2, 0), "zeros"), 0, ("<u4", (2,), "zeros")),
    ("ret", "process/empty", [("|u1", (0,), "zeros"), ("|u1", (0,), "zeros")]),
    ("sdrhip_bits_out_capacity", "h2", 16, OUT_SZ),
    ("sdrhip_bits_process", "h2", A(SYM), 16, 16, ("|u1", (2, 4), "zeros"), 4, ("<u4", (2,), "zeros")),
    ("ret", "process_raw", (("|u1", (2, 4), "zeros"), ("<u4", (2,), "zeros"))),
    ("sdrhip_bits_process_dev", "h2", 4096, 16, 19, 0x2000, 7, 0x3000),
    ("sdrhip_bits_reset", "h2"),
    ("sdrhip_free", "h1", 0xd1000),
    ("sdrhip_bits_destroy", "h2"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["subsample"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_subsample_create", "h1", 0, 4, 2, 64, OUT_VP),
    ("ret", "attrs", (0, 4, 2)),
    ("sdrhip_subsample_out_count", "h2", 16, OUT_SZ),
    ("ret", "out_count", 4),
    ("sdrhip_subsample_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process_dev", 4),
    ("sdrhip_subsample_reset", "h2"),
    ("sdrhip_subsample_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_subsample_process", "h2", A(X16), 16, 16, ("<i2", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "process", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_subsample_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(X16), ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_subsample_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process/routed", ("<i2", (2, 4, 2), "zeros")),
    ("sdrhip_subsample_out_count", "h2", 0, OUT_SZ),
    ("sdrhip_subsample_process", "h2", ("<i2", (2, 0, 2), "zeros"), 0, 0, ("<i2", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "process/empty", ("<i2", (2, 0, 2), "zeros")),
    ("sdrhip_subsample_create", "h1", 1, 4, 2, 64, OUT_VP),
    ("sdrhip_subsample_out_count", "h3", 16, OUT_SZ),
    ("sdrhip_subsample_process", "h3", A(XF32), 16, 16, ("<f4", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "cf32", ("<f4", (2, 4, 2), "zeros")),
    ("sdrhip_subsample_destroy", "h2"),
    ("sdrhip_subsample_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["fftconv"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_fftconv_create_bank", "h1", 1, 16, B(KERN), 8, 1, 2, 64, OUT_VP),
    ("ret", "attrs", (1, 16, 2, 1, True, False)),
    ("sdrhip_fftconv_set_kernel", "h2", 0, B(KERN2)),
    ("sdrhip_fftconv_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("sdrhip_fftconv_last_kernels", "h2", ("buf", 4096), 4096),
    ("ret", "last_kernels", LAST),
    ("sdrhip_fftconv_reset", "h2"),
    ("sdrhip_fftconv_process", "h2", A(XF32), 16, 16, ("<f4", (1, 2, 16, 2), "zeros"), 16),
    ("ret", "process", ("<f4", (2, 16, 2), "zeros")),
    ("router", "h1", A(XF32), ("<f4", (2, 16, 2), "zeros")),
    ("sdrhip_fftconv_process_dev", "h2", 4096, 16, 19, 0x2000, 19),
    ("ret", "process/routed", ("<f4", (2, 16, 2), "zeros")),
    ("sdrhip_fftconv_process", "h2", ("<f4", (2, 0, 2), "zeros"), 0, 0, ("<f4", (1, 2, 0, 2), "zeros"), 0),
    ("ret", "process/empty", ("<f4", (2, 0, 2), "zeros")),
    ("sdrhip_fftconv_create_bank", "h1", 0, 8, B(KERNS), 8, 2, 2, 64, OUT_VP),
    ("sdrhip_fftconv_process", "h3", A(XF32), 16, 16, ("<f4", (2, 2, 16, 2), "zeros"), 16),
    ("ret", "bank", ("<f4", (2, 2, 16, 2), "zeros")),
    ("router", "h1", A(XF32), ("<f4", (4, 16, 2), "zeros")),
    ("sdrhip_fftconv_process_dev", "h3", 4096, 16, 19, 0x2000, 19),
    ("ret", "bank/routed", ("<f4", (2, 2, 16, 2), "zeros")),
    ("sdrhip_fftconv_process", "h3", ("<f4", (2, 0, 2), "zeros"), 0, 0, ("<f4", (2, 2, 0, 2), "zeros"), 0),
    ("ret", "bank/empty", ("<f4", (2, 2, 0, 2), "zeros")),
    ("sdrhip_fftconv_f64_create_bank", "h1", 0, 8, B(KERN64), 8, 1, 2, 64, OUT_VP),
    ("ret", "f64/attrs", (1, True, True)),
    ("sdrhip_fftconv_f64_set_kernel", "h4", 0, B(KERN64)),
    ("sdrhip_fftconv_f64_process_dev", "h4", 4096, 16, 19, 0x2000, 19),
    ("sdrhip_fftconv_f64_process", "h4", A(XF64), 16, 16, ("<f8", (1, 2, 16, 2), "zeros"), 16),
    ("ret", "f64", ("<f8", (2, 16, 2), "zeros")),
    ("router", "h1", A(XF64), ("<f8", (2, 16, 2), "zeros")),
    ("sdrhip_fftconv_f64_process_dev", "h4", 4096, 16, 19, 0x2000, 19),
    ("ret", "f64/routed", ("<f8", (2, 16, 2), "zeros")),
    ("sdrhip_fftconv_f64_process", "h4", ("<f8", (2, 0, 2), "zeros"), 0, 0, ("<f8", (1, 2, 0, 2), "zeros"), 0),
    ("ret", "f64/empty", ("<f8", (2, 0, 2), "zeros")),
    ("sdrhip_fftconv_destroy", "h2"),
    ("sdrhip_fftconv_destroy", "h3"),
    ("sdrhip_fftconv_destroy", "h4"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["fftsplit"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_fftsink_create", "h1", 1, 4, 2, 8, OUT_VP),
    ("sdrhip_fftsink_form", "h2", ("out", "c_char_p")),
    ("ret", "sink/attrs", (4, 2, True, "radix4")),
    ("sdrhip_fftsink_process_dev", "h2", 4096, 16, 19, 0x2000, 70),
    ("sdrhip_fftsink_process", "h2", A(XF32), 16, 16, ("<f4", (2, 4, 8, 2), "zeros"), 32),
    ("ret", "sink", ("<f4", (2, 4, 8, 2), "zeros")),
    ("sdrhip_fftsink_process", "h2", A(XF32), 16, 16, ("<f4", (2, 4, 8, 2), "zeros"), 32),
    ("ret", "sink/routed", ("<f4", (2, 4, 8, 2), "zeros")),
    ("sdrhip_fftsink_process", "h2", ("<f4", (2, 0, 2), "zeros"), 0, 0, ("<f4", (2, 0, 8, 2), "zeros"), 0),
    ("ret", "sink/empty", ("<f4", (2, 0, 8, 2), "zeros")),
    ("sdrhip_fftsink_create", "h1", 3, 4, 2, 8, OUT_VP),
    ("sdrhip_fftsink_process", "h3", A(XF64), 16, 16, ("<f8", (2, 4, 8, 2), "zeros"), 32),
    ("ret", "sink64", ("<f8", (2, 4, 8, 2), "zeros")),
    ("sdrhip_fftsource_create", "h1", 1, 4, B(KERN), 2, 8, OUT_VP),
    ("sdrhip_fftsource_form", "h4", ("out", "c_char_p")),
    ("ret", "source/attrs", (4, 2, True, "radix4")),
    ("sdrhip_fftsource_process_dev", "h4", 4096, 4, 70, 0x2000, 19),
    ("sdrhip_fftsource_set_kernel", "h4", B(KERN2)),
    ("sdrhip_fftsource_reset", "h4"),
    ("sdrhip_fftsource_process", "h4", A(SPECIN), 4, 32, ("<f4", (2, 16, 2), "zeros"), 16),
    ("ret", "source", ("<f4", (2, 16, 2), "zeros")),
    ("sdrhip_fftsource_process", "h4", A(SPECIN), 4, 32, ("<f4", (2, 16, 2), "zeros"), 16),
    ("ret", "source/routed", ("<f4", (2, 16, 2), "zeros")),
    ("sdrhip_fftsource_process", "h4", ("<f4", (2, 0, 8, 2), "zeros"), 0, 0, ("<f4", (2, 0, 2), "zeros"), 0),
    ("ret", "source/empty", ("<f4", (2, 0, 2), "zeros")),
    ("sdrhip_fftsource_process", "h4", A(SPEC_1), 4, 32, ("<f4", (1, 16, 2), "zeros"), 16),
    ("ret", "source/3-D", ("<f4", (1, 16, 2), "zeros")),
    ("sdrhip_fftsource_create", "h1", 3, 4, B(KERN64), 2, 8, OUT_VP),
    ("sdrhip_fftsink_destroy", "h2"),
    ("sdrhip_fftsink_destroy", "h3"),
    ("sdrhip_fftsource_destroy", "h4"),
    ("sdrhip_fftsource_destroy", "h5"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["fbb"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_fbb_f32_create", "h1", 100000.0, 2400000.0, B(ALPHA), 5, 4, 2, 64, OUT_VP),
    ("ret", "attrs", (2, 4, 5)),
    ("sdrhip_fbb_f32_kernel_names", "h2", 0, ("buf", 256), 256),
    ("sdrhip_fbb_f32_kernel_names", "h2", 16, ("buf", 256), 256),
    ("ret", "kernel_names", (NAMES, NAMES)),
    ("sdrhip_fbb_f32_last_kernels", "h2", ("buf", 4096), 4096),
    ("ret", "last_kernels", LAST),
    ("sdrhip_fbb_f32_out_count", "h2", 16, OUT_SZ),
    ("ret", "out_count", 4),
    ("sdrhip_fbb_f32_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process_dev", 4),
    ("sdrhip_fbb_f32_reset", "h2"),
    ("sdrhip_fbb_f32_set_taps", "h2", B(ALPHA2)),
    ("sdrhip_fbb_f32_set_shift", "h2", 50000.0),
    ("sdrhip_fbb_f32_out_count", "h2", 16, OUT_SZ),
    ("sdrhip_fbb_f32_process", "h2", A(XF32), 16, 16, ("<f4", (2, 4, 2), "zeros"), 4, OUT_SZ),
    ("ret", "process", ("<f4", (2, 4, 2), "zeros")),
    ("sdrhip_fbb_f32_out_count", "h2", 16, OUT_SZ),
    ("router", "h1", A(XF32), ("<f4", (2, 4, 2), "zeros")),
    ("sdrhip_fbb_f32_process_dev", "h2", 4096, 16, 19, 0x2000, 7, OUT_SZ),
    ("ret", "process/routed", ("<f4", (2, 4, 2), "zeros")),
    ("sdrhip_fbb_f32_out_count", "h2", 0, OUT_SZ),
    ("sdrhip_fbb_f32_process", "h2", ("<f4", (2, 0, 2), "zeros"), 0, 0, ("<f4", (2, 0, 2), "zeros"), 0, OUT_SZ),
    ("ret", "process/empty", ("<f4", (2, 0, 2), "zeros")),
    ("sdrhip_fbb_f32_destroy", "h2"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["fft"] = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_malloc", "h1", 256, OUT_VP),
    ("sdrhip_malloc", "h1", 256, OUT_VP),
    ("sdrhip_memcpy_h2d", "h1", 0xd1000, A(XF32), 256),
    ("sdrhip_fft_c2c", "h1", 16, -1, 2, 0xd1000, 0xd2000),
    ("sdrhip_memcpy_d2h", "h1", ("<f4", (2, 16, 2), "zeros"), 0xd2000, 256),
    ("sdrhip_free", "h1", 0xd1000),
    ("sdrhip_free", "h1", 0xd2000),
    ("ret", "c2c", ("<f4", (2, 16, 2), "zeros")),
    ("sdrhip_malloc", "h1", 512, OUT_VP),
    ("sdrhip_malloc", "h1", 512, OUT_VP),
    ("sdrhip_memcpy_h2d", "h1", 0xd3000, A(XF64), 512),
    ("sdrhip_fft_c2c_f64", "h1", 16, 1, 2, 0xd3000, 0xd4000),
    ("sdrhip_memcpy_d2h", "h1", ("<f8", (2, 16, 2), "zeros"), 0xd4000, 512),
    ("sdrhip_free", "h1", 0xd3000),
    ("sdrhip_free", "h1", 0xd4000),
    ("ret", "c2c_f64", ("<f8", (2, 16, 2), "zeros")),
    ("sdrhip_fft_exec", "h1", 1, 16, -1, A(XC), ("<c8", (16,), "zeros")),
    ("ret", "exec", ("<c8", (16,))),
    ("sdrhip_fft_exec", "h1", 3, 16, 1, A(XC128), ("<c16", (16,), "zeros")),
    ("ret", "exec128", ("<c16", (16,))),
    ("sdrhip_fft_plan_create", "h1", 1, 16, OUT_VP),
    ("sdrhip_fft_plan_form", "h2", ("out", "c_char_p")),
    ("ret", "plan/attrs", (16, True, "radix4")),
    ("sdrhip_fft_plan_exec", "h2", -1, A(XC), ("<c8", (16,), "zeros")),
    ("ret", "plan/exec", ("<c8", (16,))),
    ("sdrhip_malloc", "h1", 256, OUT_VP),
    ("sdrhip_malloc", "h1", 256, OUT_VP),
    ("sdrhip_memcpy_h2d", "h1", 0xd5000, A(XCB), 256),
    ("sdrhip_fft_plan_exec_dev", "h2", 1, 2, 0xd5000, 0xd6000),
    ("sdrhip_memcpy_d2h", "h1", ("<c8", (2, 16), "zeros"), 0xd6000, 256),
    ("sdrhip_free", "h1", 0xd5000),
    ("sdrhip_free", "h1", 0xd6000),
    ("ret", "plan/exec_batch", ("<c8", (2, 16))),
    ("sdrhip_fft_plan_create", "h1", 3, 16, OUT_VP),
    ("sdrhip_fft_plan_destroy", "h2"),
    ("sdrhip_fft_plan_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]

EXPECT["comm"] = [
    ("sdrhip_comm_create", ("c_int", [0, 1]), 2, OUT_VP),
    ("sdrhip_comm_ctx", "h1", 0, OUT_VP),
    ("sdrhip_comm_ctx", "h1", 1, OUT_VP),
    ("sdrhip_comm_transport", "h1", ("out", "c_char_p")),
    ("ret", "attrs", ([0, 1], [("h2", 0), ("h3", 1)], "radix4")),
    ("sdrhip_comm_broadcast", "h1", ("c_void_p", [4096, 0x2000]), 64, 0),
    ("sdrhip_comm_gather", "h1", ("c_void_p", [4096, 0x2000]), ("c_ulong", [64, 32]), 0x3000, 1),
    ("sdrhip_comm_gather_begin", "h1", 1, ("c_void_p", [4096, 0x2000]), ("c_ulong", [64, 32]), 0x3000, 0),
    ("sdrhip_comm_gather_wait", "h1", 1),
    ("sdrhip_comm_synchronize", "h1"),
    ("hook", "h2"),
    ("hook", "h3"),
    ("sdrhip_comm_destroy", "h1"),
]


def trace(name, monkeypatch):
    r = Run(monkeypatch)
    CASES[name](r)
    return r.fake


@pytest.mark.parametrize("name", sorted(CASES))
def test_call_trace(name, monkeypatch):
    got, want = trace(name, monkeypatch).calls, EXPECT[name]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d of %s" % (k, name)
    assert len(got) == len(want), (got[len(want):], want[len(got):])


# Entry points of the header that no wrapper of nodes.py reaches (bench.py and the tools call them through abi.lib()).
NOT_WRAPPED = {"sdrhip_version", "sdrhip_strerror", "sdrhip_last_error", "sdrhip_bench_stream_read", "sdrhip_fftconv_create",
               "sdrhip_fftconv_bands", "sdrhip_comm_size", "sdrhip_host_alloc", "sdrhip_host_free", "sdrhip_host_register",
               "sdrhip_host_unregister", "sdrhip_memcpy_h2d_async", "sdrhip_memcpy_d2h_async", "sdrhip_memcpy2d_d2h_async"}


def test_every_name_the_wrappers_reach_for_is_declared(monkeypatch):
    """FakeLib answers the names of abi.SIGNATURES only, so a name outside the table fails its case; together the cases
    reach every declared entry point but the ones listed above."""
    reached = set()
    for name in CASES:
        reached |= trace(name, monkeypatch).reached
    assert set(abi.SIGNATURES) - reached == NOT_WRAPPED


def test_every_public_class_and_function_is_driven():
    src = "".join(inspect.getsource(f) for f in CASES.values())
    public = [n for n, v in vars(nodes).items() if not n.startswith("_") and getattr(v, "__module__", None) == nodes.__name__]
    assert len(public) >= 36 and not [n for n in public if "nodes.%s(" % n not in src and "n.%s(" % n not in src]


# Who meets the router in Run.three (host path, routed, empty input with the router set): counted and equal-length nodes
# once, on the non-empty input; FFTSink and FFTSource never.
ROUTER_CALLS = {"iqbb_i16": 3, "bb_i16": 2, "iqbb_i8": 1, "tuner": 3, "fir": 2, "demod": 1, "deemph": 1, "detector": 1, "bits": 1,
                "detectorbank": 1, "bitsbank": 1, "subsample": 1, "fftconv": 3, "fftsplit": 0, "fbb": 1}


@pytest.mark.parametrize("name", sorted(ROUTER_CALLS))
def test_who_meets_the_router(name, monkeypatch):
    calls = trace(name, monkeypatch).calls
    assert sum(c[0] == "router" for c in calls) == ROUTER_CALLS[name]
    for k, c in enumerate(calls):
        if c[0] == "router":        # the routed call is the node's *_process_dev(_multi), on the router's pointers
            assert "_process_dev" in calls[k + 1][0] and 0x1000 in calls[k + 1] and 0x2000 in calls[k + 1], calls[k + 1]
