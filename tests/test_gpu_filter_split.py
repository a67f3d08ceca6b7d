"""FilterSink / FilterSource as separate GPU stages (sdrhip_fftsink_* / sdrhip_fftsource_*, reference src/filternode.hh:32-227):
the natural-order 2N-point spectrum stream against numpy, the device-side chain against the oracle's overlap-add filter,
the carried tail across calls and strands, setFreq's transient, and argument errors."""
import numpy as np
import pytest

import libsdr_amd as sa
from libsdr_amd.abi import SdrHipError

pytestmark = pytest.mark.gpu

FS = 2.4e6


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def cplx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def signal(C, n, seed, dtype):
    r = np.random.default_rng(seed)
    return r.standard_normal((C, n, 2)).astype(dtype)


def spectrum(N, fmin, fmax, dtype):
    return sa.design_fftfilt_spectrum(sa.design_fftfilt_kernel(N, fmin, fmax, FS, dtype=dtype))


class Dev:
    """A device buffer with a row stride larger than the data (elements of 2 scalars)."""

    def __init__(self, ctx, rows, stride, dtype):
        self.ctx, self.rows, self.stride, self.dtype = ctx, rows, stride, np.dtype(dtype)
        self.nbytes = rows * stride * 2 * self.dtype.itemsize
        self.p = ctx.malloc(self.nbytes)
        ctx.memset(self.p, 0x7f, self.nbytes)

    def put(self, a):
        full = np.zeros((self.rows, self.stride, 2), self.dtype)
        full[:, :a.shape[1]] = a
        self.ctx.h2d(self.p, full)

    def get(self, n):
        full = np.zeros((self.rows, self.stride, 2), self.dtype)
        self.ctx.synchronize()
        self.ctx.d2h(full, self.p)
        return full[:, :n]

    def free(self):
        self.ctx.free(self.p)


def spectra_ref(x, N):
    C, n = x.shape[:2]
    blocks = cplx(x).reshape(C, n // N, N)
    return np.fft.fft(np.concatenate([blocks, np.zeros_like(blocks)], axis=2), axis=2)


CASES = [(np.float32, 1024, "fused"), (np.float32, 4096, "fused"), (np.float32, 8192, "fused"),
         (np.float32, 1000, "composed"), (np.float32, 1009, "composed"), (np.float32, 12000, "composed"),
         (np.float64, 1024, "composed"), (np.float64, 1000, "composed")]


@pytest.mark.parametrize("dtype,N,form", CASES)
@pytest.mark.parametrize("C", [1, 3, 64])
def test_spectrum_vs_numpy(ctx, dtype, N, form, C):
    nb = 2 if C < 64 else 1
    if C == 64 and N > 4096:
        C = 16
    x = signal(C, nb * N, N + C, dtype)
    sink = sa.FFTSink(ctx, N, channels=C, max_blocks=nb, dtype=dtype)
    assert sink.form == form
    din, dspec = Dev(ctx, C, nb * N + 37, dtype), Dev(ctx, C, nb * 2 * N + 53, dtype)
    try:
        din.put(x)
        sink.process_dev(din.p, nb * N, din.stride, dspec.p, dspec.stride)
        got = cplx(dspec.get(nb * 2 * N)).reshape(C, nb, 2 * N)
        tail = dspec.get(dspec.stride)[:, nb * 2 * N:]
    finally:
        din.free(); dspec.free()
    ref = spectra_ref(x, N)
    tol = 1e-5 if dtype == np.float32 else 1e-12
    for c in range(C):
        assert np.abs(got[c] - ref[c]).max() <= tol * np.abs(ref[c]).max(), c
    assert (tail.view(np.uint8) == 0x7f).all()   # nothing written past the rows
    host = sink.process(x)                           # the host entry point: the same spectra
    assert np.abs(cplx(host) - got).max() <= tol * np.abs(ref).max()


def oracle_blocks(orc, K, x, dtype):
    N = K.shape[0] // 2
    flt = orc.FFTFilterF64(K) if dtype == np.float64 else orc.FFTFilter(K)
    return np.concatenate([flt.process(x[i * N:(i + 1) * N]) for i in range(x.shape[0] // N)])


@pytest.mark.parametrize("dtype,N,golden_h", [(np.float32, 1024, "g7_fftfilt_h1024"), (np.float32, 8192, "g7_fftfilt_h8192"),
                                               (np.float32, 1000, "g15_fftfilt_h1000"),
                                               (np.float64, 1024, "g15_fftfilt_h1024_f64"),
                                               (np.float64, 1000, "g15_fftfilt_h1000_f64")])
def test_sink_to_source_on_device(ctx, golden, orc, dtype, N, golden_h):
    fmin, fmax = (50e3, 150e3) if golden_h.startswith("g7") else (-350e3, -250e3)
    h = sa.design_fftfilt_kernel(N, fmin, fmax, FS, dtype=dtype)
    assert np.array_equal(h.ravel(), golden.load(golden_h).ravel())
    K = sa.design_fftfilt_spectrum(h)
    C, nb = 3, 5
    x = signal(C, nb * N, 7, dtype)
    sink = sa.FFTSink(ctx, N, channels=C, max_blocks=nb, dtype=dtype)
    src = sa.FFTSource(ctx, N, K, channels=C, max_blocks=nb, dtype=dtype)
    din, dspec, dout = Dev(ctx, C, nb * N + 5, dtype), Dev(ctx, C, nb * 2 * N + 3, dtype), Dev(ctx, C, nb * N + 11, dtype)
    try:
        din.put(x)
        sink.process_dev(din.p, nb * N, din.stride, dspec.p, dspec.stride)
        src.process_dev(dspec.p, nb, dspec.stride, dout.p, dout.stride)
        y = dout.get(nb * N)
        beyond = dout.get(dout.stride)[:, nb * N:]
    finally:
        din.free(); dspec.free(); dout.free()
    assert (beyond.view(np.uint8) == 0x7f).all()
    tol = 1e-5 if dtype == np.float32 else 1e-12
    Ko = orc.fftfilt_design_K_f64(h) if dtype == np.float64 else orc.fftfilt_design_K(h)
    for c in range(C):
        ref = oracle_blocks(orc, Ko, x[c], dtype)
        assert np.abs(cplx(y[c]) - cplx(ref)).max() <= tol * np.abs(cplx(ref)).max(), c


@pytest.mark.parametrize("dtype,N", [(np.float32, 1024), (np.float32, 8192), (np.float32, 1000), (np.float64, 1024)])
def test_call_splitting(ctx, dtype, N):
    """7 blocks in calls of 1 + 2 + 4 equal one 7-block call (one channel: every block its own strand on the fused path)."""
    K = spectrum(N, -200e3, 300e3, dtype)
    x = signal(2, 7 * N, 3, dtype)
    sink = sa.FFTSink(ctx, N, channels=2, max_blocks=7, dtype=dtype)
    spec = sink.process(x)
    one = sa.FFTSource(ctx, N, K, channels=2, max_blocks=7, dtype=dtype)
    y1 = one.process(spec)
    parts = sa.FFTSource(ctx, N, K, channels=2, max_blocks=7, dtype=dtype)
    y2 = np.concatenate([parts.process(spec[:, a:b]) for a, b in ((0, 1), (1, 3), (3, 7))], axis=1)
    tol = 1e-6 if dtype == np.float32 else 1e-13
    assert np.abs(cplx(y1) - cplx(y2)).max() <= tol * np.abs(cplx(y1)).max()
    # reset zeroes the tail: the same call again gives the first call's output
    one.reset()
    assert np.abs(cplx(one.process(spec)) - cplx(y1)).max() <= tol * np.abs(cplx(y1)).max()


@pytest.mark.parametrize("dtype,N", [(np.float32, 1024), (np.float64, 1000)])
def test_set_kernel_transient(ctx, orc, dtype, N):
    """FilterSource::setFreq after block 3: block 4 is the OLD kernel's tail plus the NEW kernel's head, as the reference's
    overlap-add gives it; the fused bank (overlap-save underneath) gives a different transient block."""
    K1, K2 = spectrum(N, 50e3, 150e3, dtype), spectrum(N, -300e3, -100e3, dtype)
    nb = 8
    x = signal(1, nb * N, 11, dtype)[0]
    sink = sa.FFTSink(ctx, N, max_blocks=nb, dtype=dtype)
    src = sa.FFTSource(ctx, N, K1, max_blocks=nb, dtype=dtype)
    spec = sink.process(x)
    y = src.process(spec[:, :4])[0]
    src.set_kernel(K2)
    y = np.concatenate([y, src.process(spec[:, 4:])[0]])
    ref_flt = orc.FFTFilterF64(K1.astype(np.float64))
    ref = []
    for b in range(nb):
        if b == 4:
            ref_flt.K = np.ascontiguousarray(K2, np.float64).reshape(-1, 2)
        ref.append(ref_flt.process(x[b * N:(b + 1) * N]))
    ref = np.concatenate(ref)
    tol = 1e-5 if dtype == np.float32 else 1e-12
    assert np.abs(cplx(y) - cplx(ref)).max() <= tol * np.abs(cplx(ref)).max()
    # the bank: same input, same swap point
    bank = sa.FFTConv(ctx, sa.FFTCONV_OLA, 2 * N, K1, max_in=nb * N, dtype=dtype)
    yb = bank.process(x[:4 * N])[0]
    bank.set_kernel(0, K2)
    yb = np.concatenate([yb, bank.process(x[4 * N:])[0]])
    scale = np.abs(cplx(ref)).max()
    assert np.abs(cplx(yb[:4 * N]) - cplx(ref[:4 * N])).max() <= tol * scale            # identical before the swap
    assert np.abs(cplx(yb[4 * N:5 * N]) - cplx(ref[4 * N:5 * N])).max() > 1e3 * tol * scale   # the transient block differs


def test_bad_arguments(ctx):
    from libsdr_amd import abi
    import ctypes as C
    L = abi.lib()
    h = C.c_void_p()
    assert L.sdrhip_fftsink_create(ctx.handle, sa.T_CS16, 1024, 1, 4, C.byref(h)) == -1     # wrong dtype
    assert L.sdrhip_fftsink_create(ctx.handle, sa.T_CF32, 0, 1, 4, C.byref(h)) == -1        # N = 0
    K = np.zeros((2048, 2), np.float32)
    assert L.sdrhip_fftsource_create(ctx.handle, 7, 1024, K.ctypes.data_as(C.c_void_p), 1, 4, C.byref(h)) == -1
    assert L.sdrhip_fftsource_create(ctx.handle, sa.T_CF32, 0, K.ctypes.data_as(C.c_void_p), 1, 4, C.byref(h)) == -1
    sink = sa.FFTSink(ctx, 1024, max_blocks=4)
    with pytest.raises(SdrHipError):
        sink.process(np.zeros((1, 1000, 2), np.float32))             # not a whole number of blocks
    x = np.zeros((1, 1536, 2), np.float32)
    spec = np.full((1, 2, 2048, 2), 7.0, np.float32)
    rc = L.sdrhip_fftsink_process(sink._h, x.ctypes.data_as(C.c_void_p), 1536, 1536, spec.ctypes.data_as(C.c_void_p), 4096)
    assert rc == -1 and (spec == 7.0).all()                          # an error code, nothing written
    with pytest.raises(SdrHipError):
        sink.process(np.zeros((1, 5 * 1024, 2), np.float32))        # more blocks than max_blocks
