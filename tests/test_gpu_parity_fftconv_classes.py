"""GPU parity of every compiled instance of the FFT convolution (tests/fftconv_classes.py: fftconv_fused_kernel<...>,
fftconv_kernel, conv_kernel<float2 | double2>, the big_* passes) and of the routes into them (sdrhip_fir_create, the
overlap-add plans that run as overlap-save). Per case, over three calls of ragged lengths with the history carried: after
every call last_kernels() must be exactly what the case names — a case that lands on another instance FAILS; every channel
is held to a float64 convolution of the same taps, on white noise and on an impulse train that puts a tap value on every
output around a block seam, within the project's contract (RTOL of tests/test_gpu_parity.py for complex<float>, 1e-12 for
complex<double>, of each channel's largest reference magnitude); where the code promises identical bits (the pipelined forms
and the one-block-per-workgroup kernel, the compile-time plans and the run-time plan) they are compared too. The module
runs inside the red-zoned device arena (tests/redzone.py); a case picks the band: 37 elements for rows on every alignment,
38 for 16-byte-aligned rows, which the 16-byte pipelined forms need. Run with `pytest -m gpu` on an MI355X; `-s` prints the
kernels the device reported and every error figure."""
import numpy as np
import pytest

import libsdr_amd as sa

try:   # torch brings its own HIP runtime: it only finds the GPU when it initialises before libsdrhip.so does
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()
except Exception:   # pragma: no cover
    torch = None

import fftconv_classes as fc
from redzone import RedZone
from test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

RTOL_F64 = 1e-12


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in fc.ENV_HOOKS:
        monkeypatch.delenv(k, raising=False)


def set_hooks(monkeypatch, env):
    """The library reads its hooks when a plan is made and again at every launch: exactly `env` is set."""
    for k in fc.ENV_HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in fc.ENV_HOOKS, k
        monkeypatch.setenv(k, v)


def make_node(ctx, case, kernel):
    if case.kind == "fir":
        return sa.FIR(ctx, sa.FIR_CF32, kernel, decim=1, channels=case.C, max_in=case.max_in)
    return sa.FFTConv(ctx, case.mode, case.fft_size, kernel if case.bands > 1 else kernel[0], channels=case.C, max_in=case.max_in,
                      dtype=np.float64 if case.f64 else np.float32)


def run(node, case, chunk):
    """One call through the arena -> [bands, C, n, 2]."""
    before = RedZone.calls
    y = node.process(chunk)
    assert RedZone.active and RedZone.calls == before + 1
    y = y if y.ndim == 4 else y[None]
    assert y.shape == (case.bands, case.C, chunk.shape[1], 2)
    return y


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c.id)
def test_fftconv_class_case(ctx, case, monkeypatch):
    monkeypatch.setattr(RedZone, "band", case.band)
    kernel, taps = fc.case_taps(case)
    assert taps.shape == (case.bands, case.n_taps)
    tol = case.rtol if case.rtol is not None else (RTOL_F64 if case.f64 else RTOL)
    set_hooks(monkeypatch, case.env)
    node = make_node(ctx, case, kernel)
    assert node.last_kernels() == []                                   # nothing launched yet
    twin = None
    if case.twin_expect is not None:
        set_hooks(monkeypatch, case.twin_env)
        twin = make_node(ctx, case, kernel)
    rows = list(range(case.C)) if case.rows is None else case.rows
    worst = {}
    for what, x in fc.case_inputs(case):
        node.reset()
        if twin is not None:
            twin.reset()
        outs = []
        off = 0
        for k, n in enumerate(case.lens):
            chunk = np.ascontiguousarray(x[:, off:off + n])
            off += n
            set_hooks(monkeypatch, case.env)
            y = run(node, case, chunk)
            ran = node.last_kernels()
            print("FFTCONV_CLASS case=%s input=%s call=%d n_in=%d kernels=%s" % (case.id, what, k, chunk.shape[1], ran))
            assert ran == case.expect[k], (case.id, what, "call", k, ran, case.expect[k])
            if twin is not None:
                set_hooks(monkeypatch, case.twin_env)
                yt = run(twin, case, chunk)
                assert twin.last_kernels() == case.twin_expect[k], (case.id, what, "call", k, twin.last_kernels(), case.twin_expect[k])
                assert np.array_equal(y, yt), (case.id, what, "call", k, "differs from the same plan under", case.twin_env)
            outs.append(y)
        y = np.concatenate(outs, axis=2)
        for b in range(case.bands):
            for c in rows:
                ref = fc.reference(x[c], taps[b])
                got = y[b, c, :, 0].astype(np.float64) + 1j * y[b, c, :, 1]
                scale = np.abs(ref).max()
                assert scale > 0
                worst[(what, b, c)] = np.abs(got - ref).max() / scale
        print("FFTCONV_CLASS case=%s input=%s worst_rel_err=%.3e tol=%.1e" % (case.id, what, max(v for k, v in worst.items() if k[0] == what), tol))
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, (case.id, "relative error above %g (input, band, channel)" % tol, bad)
    assert len(worst) == 2 * case.bands * len(rows)
    # a call of 0 samples launches nothing, and says so
    set_hooks(monkeypatch, case.env)
    node.process(x[:, :0])
    assert node.last_kernels() == []


def test_time_domain_fir_and_float_baseband_report_their_kernels(ctx, monkeypatch):
    """sdrhip_fir_last_kernels / sdrhip_fbb_f32_last_kernels where the FIR does not run as FFT convolution: the time-domain
    kernel instance of the last call, and the history roll of a call that completes no output (every instance:
    tests/test_gpu_parity_fir_classes.py)."""
    rng = np.random.default_rng(9)
    alpha = rng.standard_normal(21) / 21
    x = (rng.standard_normal((2, 4096, 2)) * 0.3).astype(np.float32)
    fir = sa.FIR(ctx, sa.FIR_CF32, alpha, decim=1, channels=2, max_in=4096)     # (21 taps on a small plan: the time-domain kernel)
    assert fir.last_kernels() == []
    fir.process(x)
    assert fir.last_kernels() == ["fir_cf32_rt_kernel<4,0>"] and fir.kernel_names(4096) == ["fir_cf32_rt_kernel"]
    fir.process(x[:, :0])
    assert fir.last_kernels() == []
    fbb = sa.FloatBaseBand(ctx, 100e3, 2.4e6, alpha, 8, channels=2, max_in=4096)
    assert fbb.last_kernels() == []
    fbb.process(x)
    ran = fbb.last_kernels()                                                   # the instance; kernel_names keeps the bare name
    assert len(ran) == 1 and ran[0] in ("fir_cf32_rt_kernel<2,8>", "fir_cf32_pipe_kernel<2,8>") and [ran[0].split("<")[0]] == fbb.kernel_names(4096)
    fbb.process(x[:, :3])                                                      # 3 samples at /8: no output, the history rolls
    assert fbb.last_kernels() == ["hist_roll_cf32"]
    fbb.process(x[:, :0])
    assert fbb.last_kernels() == []
    monkeypatch.setenv("SDRHIP_FIR_FFT_ALWAYS", "1")
    small = sa.FIR(ctx, sa.FIR_CF32, alpha, decim=1, channels=2, max_in=4096)   # the same filter as FFT convolution
    small.process(x)
    assert small.last_kernels() == [fc.fused(11, 0, 128)] and small.kernel_names() == ["fftconv_fused_kernel"]
