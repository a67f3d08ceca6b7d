"""The contract of the C entry points (create / process / process_dev / reset), node type by node type.

One table row per node type, all at channels = 2 and max_in = 256, through the wrappers of libsdr_amd.nodes (the
strided host-pointer call goes to the C function directly: the wrappers only make packed ones). Every expected code
is what the sources say the entry point returns; where the node types disagree with each other the row records what
that node does, with a comment.
"""
import ctypes as C

import numpy as np
import pytest

import libsdr_amd as sa
from libsdr_amd import abi

pytestmark = pytest.mark.gpu

CH, MAX_IN, PAD = 2, 256, 3
FS = 2.4e6


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Row:
    """One node type. Counts are in the unit the ABI counts in (samples; FFTSource: blocks). Buffers are
    [rows, stride, comps] arrays, so a stride is the second dimension."""
    n = 200                       # the call the tests make
    too_many = MAX_IN + 1
    in_dtype, in_comps = np.int16, 2
    out_dtype, out_comps = np.int16, 2
    create_codes = (abi.E_INVALID, abi.E_SIZE)   # channels = 0, max_in = 0
    has_reset = True
    has_in_stride = True

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        raise NotImplementedError

    def in_rows(self):
        return CH

    def in_len(self, node, n):    # elements per input row
        return n

    def out_len(self, node, n):   # elements per output row, from the node's current state
        return n

    def data(self, rng, rows, length):
        if np.issubdtype(self.in_dtype, np.floating):
            return rng.standard_normal((rows, length, self.in_comps)).astype(self.in_dtype)
        return rng.integers(-2000, 2000, size=(rows, length, self.in_comps)).astype(self.in_dtype)

    def host(self, node, x, n, in_stride, out, out_stride):   # the raw host-pointer entry point -> code
        raise NotImplementedError

    def dev(self, node, i, n, in_stride, o, out_stride):      # the wrapper's process_dev (raises)
        node.process_dev(i, n, in_stride, o, out_stride)


def _got(fn, *a):
    got = C.c_size_t(0)
    return fn(*a, C.byref(got))


def _bb_parts(order=31, Fc=100e3, lut=None):
    return (sa.design_iqbb_taps(Fc, 50e3, FS, order), sa.design_freqshift_lut_i16() if lut is None else lut,
            sa.design_freqshift_inc(Fc, FS))


class IQBB(Row):
    def make(self, ctx, channels=CH, max_in=MAX_IN):
        taps, lut, inc = _bb_parts()
        return sa.IQBaseBandI16(ctx, taps, lut, inc, False, 4, channels=channels, max_in=max_in)

    def out_len(self, node, n):
        return node.out_count(n)

    def host(self, node, x, n, si, out, so):
        return _got(abi.lib().sdrhip_iqbb_i16_process, node._h, _ptr(x), n, si, _ptr(out), so)


class BB(IQBB):
    in_comps = 1

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        lut, inc = sa.design_freqshift_lut_i16(), sa.design_freqshift_inc(100e3, FS)
        return sa.BaseBandI16(ctx, sa.design_bb_taps(100e3, 50e3, FS, 31), lut, inc, False, 4, channels=channels, max_in=max_in)


class IQBB8(IQBB):
    in_dtype = out_dtype = np.int8

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        taps, lut, inc = _bb_parts(21, lut=sa.design_freqshift_lut_i8())
        return sa.IQBaseBandI8(ctx, taps, lut, inc, False, 4, channels=channels, max_in=max_in)

    def data(self, rng, rows, length):
        return rng.integers(-128, 128, size=(rows, length, 2)).astype(np.int8)


class Tuner(IQBB):
    has_in_stride = False   # one shared input row: the entry points take no in_stride

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        taps, lut, _ = _bb_parts()
        inc = [sa.design_freqshift_inc(100e3 + 50e3 * c, FS) for c in range(channels)]
        return sa.TunerBankI16(ctx, np.stack([taps] * channels) if channels else np.zeros((0, 31, 2), np.int32), lut,
                               np.asarray(inc, np.uint32), [False] * channels, 4, max_in=max_in)

    def in_rows(self):
        return 1

    def host(self, node, x, n, si, out, so):
        return _got(abi.lib().sdrhip_tuner_i16_process, node._h, _ptr(x), n, _ptr(out), so)

    def dev(self, node, i, n, in_stride, o, out_stride):
        node.process_dev(i, n, o, out_stride)


class FirExact(Row):
    kind, decim, order = sa.FIR_CS16_EXACT, 1, 15

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        return sa.FIR(ctx, self.kind, sa.design_fir_lowpass(self.order, 100e3, FS), self.decim, channels=channels, max_in=max_in)

    def out_len(self, node, n):
        return node.out_count(n)

    def host(self, node, x, n, si, out, so):
        return _got(abi.lib().sdrhip_fir_process, node._h, _ptr(x), n, si, _ptr(out), so)


class FirF32(FirExact):
    kind, decim = sa.FIR_CF32, 2
    in_dtype = out_dtype = np.float32


class FirF32Fft(FirF32):
    decim, order = 1, 65   # complex<float>, no decimation, more than 32 taps: an overlap-save plan behind the handle


class FBB(Row):
    in_dtype = out_dtype = np.float32

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        return sa.FloatBaseBand(ctx, 100e3, FS, sa.design_fir_lowpass(15, 100e3, FS), 4, channels=channels, max_in=max_in)

    def out_len(self, node, n):
        return node.out_count(n)

    def host(self, node, x, n, si, out, so):
        return _got(abi.lib().sdrhip_fbb_f32_process, node._h, _ptr(x), n, si, _ptr(out), so)


class DemodFM(Row):
    out_comps = 1

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        return sa.Demod(ctx, sa.EPI_FM, channels=channels, max_in=max_in)

    def host(self, node, x, n, si, out, so):
        return abi.lib().sdrhip_demod_process(node._h, _ptr(x), n, si, _ptr(out), so)


class Deemph(Row):
    in_comps = out_comps = 1

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        return sa.FMDeemphI16(ctx, 5, channels=channels, max_in=max_in)

    def host(self, node, x, n, si, out, so):
        return abi.lib().sdrhip_deemph_i16_process(node._h, _ptr(x), n, si, _ptr(out), so)


class Sub(Row):
    def make(self, ctx, channels=CH, max_in=MAX_IN):
        return sa.SubSample(ctx, sa.T_CS16, 3, channels=channels, max_in=max_in)

    def out_len(self, node, n):
        return node.out_count(n)

    def host(self, node, x, n, si, out, so):
        return _got(abi.lib().sdrhip_subsample_process, node._h, _ptr(x), n, si, _ptr(out), so)


class Fsk(Row):
    in_comps = out_comps = 1
    out_dtype = np.uint8

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        return sa.FSKDetector(ctx, 22050.0, 1200.0, 1200.0, 2200.0, channels=channels, max_in=max_in)

    def host(self, node, x, n, si, out, so):
        return abi.lib().sdrhip_detector_process(node._h, _ptr(x), n, si, _ptr(out), so)


class Ask(Fsk):
    def make(self, ctx, channels=CH, max_in=MAX_IN):
        return sa.ASKDetector(ctx, channels=channels, max_in=max_in)


class Bits(Row):
    in_dtype = out_dtype = np.uint8
    in_comps = out_comps = 1

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        node = sa.BitStream(ctx, 22050.0, 1200.0, channels=channels, max_in=max_in)
        node.counts = np.zeros(max(channels, 1), np.uint32)   # the last call's counts (host calls)
        node._counts_dev = ctx.malloc(4 * max(channels, 1))
        return node

    def out_len(self, node, n):
        return node.out_capacity(n)

    def data(self, rng, rows, length):   # symbols held for about a bit's 18 samples
        return np.repeat(rng.integers(0, 2, size=(rows, length // 16 + 1, 1)), 16, axis=1)[:, :length].astype(np.uint8)

    def host(self, node, x, n, si, out, so):
        return abi.lib().sdrhip_bits_process(node._h, _ptr(x), n, si, _ptr(out), so, _ptr(node.counts))

    def dev(self, node, i, n, in_stride, o, out_stride):
        node.process_dev(i, n, in_stride, o, out_stride, node._counts_dev)


class ConvOls(Row):
    in_dtype = out_dtype = np.float32

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        h = np.random.default_rng(5).standard_normal((33, 2)).astype(np.float32)
        return sa.FFTConv(ctx, sa.FFTCONV_OLS, 256, h, channels=channels, max_in=max_in)

    def host(self, node, x, n, si, out, so):
        return abi.lib().sdrhip_fftconv_process(node._h, _ptr(x), n, si, _ptr(out), so)


class ConvOla(ConvOls):
    def make(self, ctx, channels=CH, max_in=MAX_IN):
        K = sa.design_fftfilt_spectrum(sa.design_fftfilt_kernel(64, -200e3, 200e3, FS))
        return sa.FFTConv(ctx, sa.FFTCONV_OLA, 128, K, channels=channels, max_in=max_in)


class Sink(Row):
    """FilterSink counts its plan in blocks (max_blocks = max_in / N) and takes whole blocks only."""
    N = 64
    n = 192
    too_many = MAX_IN + N
    in_dtype = out_dtype = np.float32
    create_codes = (abi.E_INVALID, abi.E_INVALID)   # max_blocks = 0 is E_INVALID here, where max_in = 0 is E_SIZE elsewhere
    has_reset = False   # no state, no reset entry point

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        return sa.FFTSink(ctx, self.N, channels=channels, max_blocks=max_in // self.N)

    def out_len(self, node, n):
        return n // self.N * 2 * self.N

    def host(self, node, x, n, si, out, so):
        return abi.lib().sdrhip_fftsink_process(node._h, _ptr(x), n, si, _ptr(out), so)


class Source(Row):
    N = 64
    n = 3                 # blocks
    too_many = MAX_IN // N + 1
    in_dtype = out_dtype = np.float32
    create_codes = (abi.E_INVALID, abi.E_INVALID)   # as FilterSink

    def make(self, ctx, channels=CH, max_in=MAX_IN):
        K = sa.design_fftfilt_spectrum(sa.design_fftfilt_kernel(self.N, -200e3, 200e3, FS))
        return sa.FFTSource(ctx, self.N, K, channels=channels, max_blocks=max_in // self.N)

    def in_len(self, node, n):
        return n * 2 * self.N

    def out_len(self, node, n):
        return n * self.N

    def host(self, node, x, n, si, out, so):
        return abi.lib().sdrhip_fftsource_process(node._h, _ptr(x), n, si, _ptr(out), so)


ROWS = [IQBB, BB, IQBB8, Tuner, FirExact, FirF32, FirF32Fft, FBB, DemodFM, Deemph, Sub, Fsk, Ask, Bits, ConvOls, ConvOla, Sink, Source]


@pytest.fixture(params=ROWS, ids=lambda r: r.__name__)
def row(request):
    return request.param()


def _in(row, seed=11):
    return row.data(np.random.default_rng(seed), row.in_rows(), row.in_len(None, row.n))


def _call(row, node, x, n, in_pad=0, out_pad=0, fill=0):
    """One host-pointer call of n from x's first rows; returns (code, out) with out = [rows, out_len + out_pad, comps]."""
    length = row.in_len(node, n)
    xin = np.zeros((x.shape[0], length + in_pad, x.shape[2]), x.dtype)
    xin[:, :length] = x[:, :length]
    no = row.out_len(node, n)
    out = np.full((CH, no + out_pad, row.out_comps), fill, row.out_dtype)
    rc = row.host(node, xin, n, length + in_pad, out, no + out_pad)
    return rc, out


def _first(row, node, x):
    rc, out = _call(row, node, x, row.n)
    assert rc == abi.OK
    return (out, node.counts.copy()) if isinstance(row, Bits) else (out, None)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is None or np.array_equal(a[1], b[1]))


def test_create_refuses_no_channels_and_no_samples(ctx, row):
    for kw, code in zip(({"channels": 0}, {"max_in": 0}), row.create_codes):
        with pytest.raises(sa.SdrHipError) as e:
            row.make(ctx, **kw)
        assert e.value.code == code, (kw, str(e.value))


def test_more_than_max_in_is_a_size_error(ctx, row):
    node = row.make(ctx)
    x = row.data(np.random.default_rng(1), row.in_rows(), row.in_len(node, row.too_many))
    rc, _ = _call(row, node, x, row.too_many)
    assert rc == abi.E_SIZE


def test_empty_call_and_reset_leave_a_fresh_node(ctx, row):
    x = _in(row)
    want = _first(row, row.make(ctx), x)
    node = row.make(ctx)
    rc, out = _call(row, node, x, 0, out_pad=PAD, fill=0x5A)
    assert rc == abi.OK and (out == row.out_dtype(0x5A)).all(), "an empty call wrote to the output"
    if isinstance(row, Bits):
        assert not node.counts.any()
    got = _first(row, node, x)
    assert _same(got, want), "an empty call moved the state"
    if row.has_reset:
        _first(row, node, _in(row, seed=12))   # (more state to forget)
        node.reset()
        assert _same(_first(row, node, x), want), "reset() did not restore the fresh state"


def test_strided_host_call_equals_the_packed_one(ctx, row):
    x = _in(row)
    want = _first(row, row.make(ctx), x)
    node = row.make(ctx)
    fill = 0x5A
    rc, out = _call(row, node, x, row.n, in_pad=PAD if row.has_in_stride else 0, out_pad=PAD, fill=fill)
    assert rc == abi.OK
    no = want[0].shape[1]
    assert out.shape[1] == no + PAD
    assert np.array_equal(out[:, :no], want[0])
    assert (out[:, no:] == row.out_dtype(fill)).all(), "the padding of the caller's rows was written"
    if want[1] is not None:
        assert np.array_equal(node.counts, want[1])


def _dev_buffers(ctx, row, node):
    e_in = np.dtype(row.in_dtype).itemsize * row.in_comps
    e_out = np.dtype(row.out_dtype).itemsize * row.out_comps
    nbytes = CH * (max(row.in_len(node, row.n) * e_in, row.out_len(node, row.n) * e_out) + 64)
    return ctx.malloc(nbytes), ctx.malloc(nbytes)


# (the tuner bank's entry points take one shared input row and no in_stride: no such case)
@pytest.mark.parametrize("strided", [r for r in ROWS if r.has_in_stride], ids=lambda r: r.__name__)
def test_process_dev_refuses_a_short_in_stride(ctx, strided):
    row = strided()
    node = row.make(ctx)
    a, b = _dev_buffers(ctx, row, node)
    try:
        with pytest.raises(sa.SdrHipError) as e:
            row.dev(node, a, row.n, row.in_len(node, row.n) - 1, b, 0)
        assert e.value.code == abi.E_SIZE, str(e.value)
    finally:
        ctx.free(a); ctx.free(b)


def test_process_dev_refuses_overlapping_buffers(ctx, row):
    node = row.make(ctx)
    a, b = _dev_buffers(ctx, row, node)
    try:
        with pytest.raises(sa.SdrHipError) as e:
            row.dev(node, a, row.n, 0, a, 0)
        assert e.value.code == abi.E_INVALID and "overlap" in str(e.value), str(e.value)
    finally:
        ctx.free(a); ctx.free(b)
