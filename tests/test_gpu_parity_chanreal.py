"""GPU parity of the channelizer for a real-sampled row (include/sdrhip_chanreal.h, Channelizer(real=True)) against its numpy
float64 restatement (tests/chanreal_restatement.py, folded_real) on the float32-rounded taps: max |y - ref| / max |ref| <= 1e-5,
the project's bound for its float / FFT paths (the complex form measured 3.2e-8 ... 1.8e-7 against it). Bit for bit: a stream cut
into calls against one call, a selected subset holding 0 and H in non-ascending order against those rows of the full run, the
stream after reset against a fresh handle. Against the complex node fed (x, 0) with rows 0 ... H selected: <= 2e-5 of the largest
output (both are within 1e-5 of the same numbers). int16 extremes are in every int16 row; an inf and a NaN sample make exactly the
output times whose tap window holds them non-finite, in every channel, as in the restatement, and leave the others' bits alone.
By its name the module runs in the red-zoned arena (device-pointer calls, guard bands checked after every call); one test takes
the host-pointer path. Every shape has 3 T + 1 output times, T from the header's rule: three full tiles and one more."""
import ctypes as C
import functools

import numpy as np
import pytest

import chanreal_restatement as RR

pytestmark = pytest.mark.gpu

BOUND = 1e-5
DTYPES = ["s16", "f32"]
NP = {"s16": np.int16, "f32": np.float32}


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


def _signal(dtype, n, seed):
    rng = np.random.default_rng(seed)
    if dtype == "s16":
        x = rng.integers(-20000, 20000, n).astype(np.int16)
        x[n // 3], x[n // 3 + 1], x[0], x[n - 1] = 32767, -32768, -32768, 32767
        return x
    return (0.5 * rng.standard_normal(n)).astype(np.float32)


def _lens(n, D):
    head = [0, 1, D - 1, D + 1]
    return head + [n - sum(head)]


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """(taps, x, lens, folded reference [H + 1, n_out] complex128) of a shape: 3 T + 1 output times"""
    M, D, n_taps = shape
    n = (3 * RR.tile_times(M) + 1) * D
    taps, x = RR.prototype(M, n_taps), _signal(dtype, n, 17 * M + D + n_taps)
    ref = RR.folded_real(x, RR.round32(taps), M, D)
    ref.setflags(write=False)
    return taps, x, _lens(n, D), ref


def _node(ctx, shape, dtype, taps, max_in, channels=None):
    import libsdr_amd as sa
    M, D, _ = shape
    node = sa.Channelizer(ctx, NP[dtype], M, D, taps, channels=channels, max_in=max_in, real=True)
    assert node.kernel_names == ["channelizer_real_%s_kernel" % dtype]
    info = node.plan_info()
    assert info["tile_times"] == RR.tile_times(M) and info["branch_taps"] == -(-shape[2] // M) and info["rows"] == node.channels
    assert info["lds_bytes"] == RR.tile_times(M) * RR.image_stride(M) * 8
    return node


def _run(node, x, lens):
    parts, off = [], 0
    for n in lens:
        assert node.out_count(n) == (off + n) // node.D - off // node.D
        parts.append(node.process(x[off:off + n]))
        off += n
    return np.concatenate(parts, axis=1)


def _cplx(y):
    return y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64)


def _err(y, ref):
    """max |y - ref| / max |ref| of float32 rows [rows, n, 2] against complex128 [rows, n]"""
    return float(np.abs(_cplx(y) - ref).max() / np.abs(ref).max())


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", RR.SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_split_stream_against_the_restatement(ctx, shape, dtype):
    import libsdr_amd as sa
    from redzone import RedZone
    M, D, n_taps = shape
    H = M // 2
    taps, x, lens, ref = _case(shape, dtype)
    n, before = len(x), RedZone.calls
    assert ref.shape == (H + 1, 3 * RR.tile_times(M) + 1)
    node = _node(ctx, shape, dtype, taps, n)
    assert node.channels == H + 1 and node.selected == list(range(H + 1))
    y = _run(node, x, lens)
    guarded = len([1 for k, v in enumerate(lens) if v and (sum(lens[:k + 1]) // D - sum(lens[:k]) // D)])
    assert RedZone.calls - before == guarded and guarded >= 1
    err = _err(y, ref)
    print("chanreal %s %s: max |y - folded_real| / max |folded_real| = %.3g" % (shape, dtype, err))
    assert y.shape == (H + 1, ref.shape[1], 2) and err <= BOUND, err
    assert not y[0, :, 1].any() and not y[H, :, 1].any()     # channels 0 and H are real rows
    # the state: the count and the last n_taps - 1 samples as (re, 0) pairs
    s = node.get_state()
    assert s["consumed"] == n
    want_tail = np.zeros((n_taps - 1, 2), np.float32)
    k = min(n_taps - 1, n)
    if k:
        want_tail[n_taps - 1 - k:, 0] = x[n - k:]
    assert same(s["tail"], want_tail)
    # bit for bit: one call on a fresh handle; the same handle after reset; a subset with 0 and H, not ascending
    one = _node(ctx, shape, dtype, taps, n)
    whole = one.process(x)
    assert same(whole, y)
    node.reset()
    assert node.get_state()["consumed"] == 0 and not node.get_state()["tail"].any()
    assert same(_run(node, x, lens), y)
    sel = [H, 0, H // 2, 1, H - 1] if H >= 4 else [H, 0, 1]
    sel = list(dict.fromkeys(sel))
    one.reset()
    one.set_channels(sel)
    assert one.plan_info()["rows"] == len(sel)
    assert same(one.process(x), y[sel])
    node.reset()
    node.set_channels(sel)
    assert same(_run(node, x, lens), y[sel])
    node.close()
    one.close()
    # the complex node on (x, 0), rows 0 ... H: both are within BOUND of the same numbers
    xc = np.stack([x, np.zeros_like(x)], axis=1)
    cnode = sa.Channelizer(ctx, NP[dtype], M, D, taps, channels=list(range(H + 1)), max_in=n)
    yc = cnode.process(xc)
    cnode.close()
    err_c = float(np.abs(_cplx(y) - _cplx(yc)).max() / np.abs(ref).max())
    print("chanreal %s %s: max |y - complex node| / max = %.3g" % (shape, dtype, err_c))
    assert err_c <= 2 * BOUND, err_c


@pytest.mark.parametrize("shape,dtype", [((12, 5, 30), "f32"), ((64, 64, 40), "s16")], ids=["12-5-30-f32", "64-64-40-s16"])
def test_set_taps_in_mid_stream(ctx, shape, dtype):
    import libsdr_amd as sa
    M, D, n_taps = shape
    taps, x, _, ref = _case(shape, dtype)
    other = RR.prototype(M, n_taps)[::-1] * np.linspace(0.5, 1.5, n_taps)
    cut = 5 * D + 1
    node, stream = _node(ctx, shape, dtype, taps, len(x)), RR.Stream(taps, M, D)
    got, want = [node.process(x[:cut])], [stream.process(x[:cut])]
    node.set_taps(other)
    stream.set_taps(other)
    got.append(node.process(x[cut:]))
    want.append(stream.process(x[cut:]))
    assert node.get_state()["consumed"] == len(x) == stream.state()[0]
    y, w = np.concatenate(got, axis=1), np.concatenate(want, axis=1)
    err = _err(y, w)
    print("chanreal set_taps %s %s: %.3g" % (shape, dtype, err))
    assert err <= BOUND, err
    assert _err(y, ref) > 1e-2                              # (the new taps were used)
    bad = other.copy()
    bad[3] = np.inf
    with pytest.raises(sa.SdrHipError) as e:
        node.set_taps(bad)
    assert e.value.code == sa.abi.E_INVALID
    node.close()


@pytest.mark.parametrize("shape", [(12, 5, 30), (64, 64, 40), (1000, 500, 3000)], ids=lambda s: "%d-%d-%d" % s)
def test_inf_and_nan_samples(ctx, shape):
    """An output time is non-finite in every channel exactly where its n_taps-sample window holds the inf or the NaN — the
    restatement's definition says the same — and has the bits of the run with zeros in their place everywhere else."""
    M, D, n_taps = shape
    taps, x, lens, _ = _case(shape, "f32")
    n = len(x)
    i_inf, i_nan = n // 4, (2 * n) // 3
    bad, clean = x.copy(), x.copy()
    bad[i_inf], bad[i_nan] = np.inf, np.nan
    clean[i_inf] = clean[i_nan] = 0
    t = (np.arange(n // D) + 1) * D - 1
    hit = np.zeros(n // D, bool)
    for i in (i_inf, i_nan):
        hit |= (t >= i) & (t - i < n_taps)
    assert hit.any() and not hit.all()
    h = RR.round32(taps)
    j = int(np.flatnonzero(hit)[0])
    with np.errstate(invalid="ignore"):
        d = RR.direct_real(bad.astype(np.float64), h, M, D, max(j - 1, 0), 3)
    assert [bool(np.isfinite(d[:, q]).all()) for q in range(3)] == [not hit[max(j - 1, 0) + q] for q in range(3)]
    assert not np.isfinite(d[:, 1 if j else 0]).any()
    node = _node(ctx, shape, "f32", taps, n)
    yb = _run(node, bad, lens)
    node.reset()
    yc = _run(node, clean, lens)
    node.close()
    finite = np.isfinite(yb).all(axis=2)                    # [rows, n_out]
    assert not finite[:, hit].any() and finite[:, ~hit].all()
    assert same(np.ascontiguousarray(yb[:, ~hit]), np.ascontiguousarray(yc[:, ~hit]))


@pytest.mark.hostptr_only
def test_host_pointer_staging_grows_with_the_selection(ctx):
    """As the complex node's case: two staged rows first, then all M / 2 + 1 through the same staging."""
    shape, dtype = (12, 5, 30), "s16"
    M, D, _ = shape
    taps, x, _, ref = _case(shape, dtype)
    lens = [1, 7, 23, (RR.tile_times(M) + 1) * D]
    lens.append(len(x) - sum(lens))
    node = _node(ctx, shape, dtype, taps, len(x), channels=[5, 0])
    y2 = _run(node, x, lens)
    assert y2.shape == (2, ref.shape[1], 2) and _err(y2, ref[[5, 0]]) <= BOUND
    node.reset()
    node.set_channels(None)
    assert node.plan_info()["rows"] == M // 2 + 1
    y = _run(node, x, lens)
    err = _err(y, ref)
    print("chanreal %s %s, rows 2 -> %d through the staging: %.3g" % (shape, dtype, M // 2 + 1, err))
    assert y.shape == (M // 2 + 1, ref.shape[1], 2) and err <= BOUND, err
    assert same(y[[5, 0]], y2)
    node.reset()
    assert same(node.process(x), y)                         # one call of max_in samples: the largest staged output
    node.close()


@pytest.mark.hostptr_only
def test_host_pointer_calls_and_refusals(ctx):
    import libsdr_amd as sa
    from libsdr_amd import abi
    shape, dtype = (12, 5, 30), "s16"
    M, D, _ = shape
    H = M // 2
    taps, x, lens, ref = _case(shape, dtype)
    n = len(x)
    node = _node(ctx, shape, dtype, taps, n)
    y = _run(node, x, lens)
    assert _err(y, ref) <= BOUND
    node.reset()
    node.set_channels([6, 2])
    assert same(node.process(x), y[[6, 2]])                 # (the staged rows follow the selection)
    node.set_channels(None)
    node.reset()
    assert same(node.process(x), y)
    for idx in ([], [0, 7], [-1], [3, 3], list(range(7)) + [0]):
        with pytest.raises(sa.SdrHipError) as e:
            node.set_channels(idx)
        assert e.value.code == abi.E_INVALID
    assert node.plan_info()["rows"] == H + 1
    # refusals change nothing
    state = node.get_state()
    no = node.out_count(60)
    out = np.full((H + 1, no, 2), 7, np.float32)
    p = lambda a: a.ctypes.data
    xs = np.ascontiguousarray(x[:60])
    assert node._c_process(node._h, p(xs), 60, p(out), no - 1, None) == abi.E_SIZE        # an out stride below the count
    assert node._c_process(node._h, p(xs), n + 1, p(out), no, None) == abi.E_SIZE         # above max_in
    assert node._c_process(node._h, None, 60, p(out), no, None) == abi.E_INVALID
    din, dout = ctx.malloc(xs.nbytes), ctx.malloc(out.nbytes)
    try:
        assert node._c_process_dev(node._h, din, 60, dout, no - 1, None) == abi.E_SIZE
        assert node._c_process_dev(node._h, din, 60, din, no, None) == abi.E_INVALID      # the output over the input
        # the overlap check uses the real element's size: an output that begins inside the 60 int16 samples is refused, too
        assert node._c_process_dev(node._h, din, 60, din + 112, no, None) == abi.E_INVALID
    finally:
        ctx.free(din)
        ctx.free(dout)
    tail = np.zeros((4, 2), np.float32)
    assert node._c_get_state(node._h, None, tail.ctypes.data_as(C.POINTER(C.c_float)), 4) == abi.E_SIZE
    after = node.get_state()
    assert after["consumed"] == state["consumed"] and same(after["tail"], state["tail"]) and np.all(out == 7)
    node.close()
