"""GPU parity of the polyphase channelizer (include/sdrhip_channelizer.h) against its numpy float64 restatement
(tests/channelizer_restatement.py) on the float32-rounded taps: max |y - ref| / max |ref| <= 1e-5, the project's bound for its
float / FFT paths (the bare transform is held to 3e-6 in test_fft_any_size_vs_numpy; the P-term branch sums come on top). Bit for
bit: a stream cut into calls against one call, a selected subset against the same rows of the full run, the stream after reset
against a fresh handle. By its name the module runs in the red-zoned arena (device-pointer calls, strided rows, guard bands
checked after every call); one test takes the host-pointer path. The node has ONE kernel form per input type for every M, so every
shape asserts the same name through kernel_names. The restatement's answers are computed once per shape and type and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import channelizer_restatement as R

pytestmark = pytest.mark.gpu

BOUND = 1e-5
# (M, D, n_taps): the smallest, powers of two, mixed radix (12 = 4 * 3, 1000 = 5^3 * 4 * 2), D = M, M / 2 and a D that divides
# nothing, n_taps below M, a multiple of M, and one above a multiple; (4096, ...) takes more than 64 KiB of LDS; (182, 77, 500)
# has the radices 13 and 7, (1320, 1320, 1500) 11, 5 and 3 beside them
SHAPES = [(2, 2, 3), (8, 8, 24), (8, 3, 21), (12, 6, 30), (64, 64, 200), (64, 32, 64), (1000, 500, 3000), (4096, 4096, 8192),
          (4096, 2048, 4097), (182, 77, 500), (1320, 1320, 1500)]
DTYPES = ["cs16", "cf32"]


def tile_times(M):
    """the header's rule"""
    return min(256, (4096 if M <= 512 else 8192) // M)


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


def _taps(M, n_taps):
    """a windowed sinc of cutoff fs / (2 M), as doubles (any finite prototype would do)"""
    t = np.arange(n_taps) - (n_taps - 1) / 2
    return np.sinc(t / M) / M * np.hanning(n_taps + 2)[1:-1]


def _signal(dtype, n, seed):
    rng = np.random.default_rng(seed)
    if dtype == "cs16":
        x = rng.integers(-20000, 20000, (n, 2)).astype(np.int16)
        x[n // 3], x[n // 3 + 1], x[0], x[n - 1] = (32767, -32768), (-32768, 32767), (-32768, -32768), (32767, 32767)
        return x
    return (0.5 * rng.standard_normal((n, 2))).astype(np.float32)


def _lens(n, D):
    head = [0, 1, D - 1, D + 1]
    return head + [n - sum(head)]


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """(taps, x, lens, folded reference [M, n_out] complex128) of a shape: 3 T + 1 output times"""
    M, D, n_taps = shape
    n = (3 * tile_times(M) + 1) * D
    taps, x = _taps(M, n_taps), _signal(dtype, n, 17 * M + D + n_taps)
    ref = R.folded(R.pairs(x), R.round32(taps), M, D)
    ref.setflags(write=False)
    return taps, x, _lens(n, D), ref


def _node(ctx, shape, dtype, taps, max_in, channels=None):
    import libsdr_amd as sa
    M, D, _ = shape
    node = sa.Channelizer(ctx, np.int16 if dtype == "cs16" else np.float32, M, D, taps, channels=channels, max_in=max_in)
    assert node.kernel_names == ["channelizer_%s_kernel" % dtype]
    info = node.plan_info()
    assert info["tile_times"] == tile_times(M) and info["branch_taps"] == -(-shape[2] // M) and info["rows"] == node.channels
    assert info["lds_bytes"] == tile_times(M) * (M + 1) * 8
    return node


def _run(node, x, lens):
    parts, off = [], 0
    for n in lens:
        assert node.out_count(n) == (off + n) // node.D - off // node.D
        parts.append(node.process(x[off:off + n]))
        off += n
    return np.concatenate(parts, axis=1)


def _err(y, ref):
    """max |y - ref| / max |ref| of float32 rows [rows, n, 2] against complex128 [rows, n]"""
    got = y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_split_stream_against_the_restatement(ctx, shape, dtype):
    from redzone import RedZone
    M, D, n_taps = shape
    taps, x, lens, ref = _case(shape, dtype)
    n, before = len(x), RedZone.calls
    assert ref.shape == (M, 3 * tile_times(M) + 1)
    node = _node(ctx, shape, dtype, taps, n)
    y = _run(node, x, lens)
    guarded = len([1 for k, v in enumerate(lens) if v and (sum(lens[:k + 1]) // D - sum(lens[:k]) // D)])
    assert RedZone.calls - before == guarded and guarded >= 1
    err = _err(y, ref)
    print("channelizer %s %s: max |y - folded| / max |folded| = %.3g" % (shape, dtype, err))
    assert y.shape == (M, ref.shape[1], 2) and err <= BOUND, err
    if M >= 1000:
        rng = np.random.default_rng(M)
        pool = [k for k in range(M) if k not in (0, 1, M // 2, M - 1)]
        chans = [0, 1, M // 2, M - 1] + sorted(int(k) for k in rng.choice(pool, 60, replace=False))
        d = R.direct(R.pairs(x), R.round32(taps), M, D, chans)
        err_d = _err(y[chans], d)
        print("channelizer %s %s: max |y - direct| / max |direct| = %.3g over %d channels" % (shape, dtype, err_d, len(chans)))
        assert err_d <= BOUND, err_d
    # the state: the count and the last n_taps - 1 samples
    s = node.get_state()
    assert s["consumed"] == n
    want_tail = np.zeros((n_taps - 1, 2), np.float32)
    k = min(n_taps - 1, n)
    if k:
        want_tail[n_taps - 1 - k:] = x[n - k:]
    assert same(s["tail"], want_tail)
    # bit for bit: one call on a fresh handle; the same handle after reset; 5 selected rows in reversed order
    one = _node(ctx, shape, dtype, taps, n)
    whole = one.process(x)
    assert same(whole, y)
    node.reset()
    assert node.get_state()["consumed"] == 0 and not node.get_state()["tail"].any()
    assert same(_run(node, x, lens), y)
    sel = sorted({0, 1 % M, M // 2, M - 2, M - 1})[::-1]
    one.reset()
    one.set_channels(sel)
    assert one.plan_info()["rows"] == len(sel)
    assert same(one.process(x), y[sel])
    node.reset()
    node.set_channels(sel)
    assert same(_run(node, x, lens), y[sel])
    node.close()
    one.close()


@pytest.mark.parametrize("shape,dtype", [((12, 6, 30), "cf32"), ((64, 32, 64), "cs16")], ids=["12-6-30-cf32", "64-32-64-cs16"])
def test_set_taps_in_mid_stream(ctx, shape, dtype):
    M, D, n_taps = shape
    taps, x, _, _ = _case(shape, dtype)
    other = _taps(M, n_taps)[::-1] * np.linspace(0.5, 1.5, n_taps)
    cut = 5 * D + 1
    node, ref = _node(ctx, shape, dtype, taps, len(x)), R.Stream(taps, M, D)
    got, want = [node.process(x[:cut])], [ref.process(x[:cut])]
    node.set_taps(other)
    ref.set_taps(other)
    got.append(node.process(x[cut:]))
    want.append(ref.process(x[cut:]))
    assert node.get_state()["consumed"] == len(x) == ref.state()[0]
    y, w = np.concatenate(got, axis=1), np.concatenate(want, axis=1)
    err = _err(y, w)
    print("channelizer set_taps %s %s: %.3g" % (shape, dtype, err))
    assert err <= BOUND, err
    unchanged = R.folded(R.pairs(x), R.round32(taps), M, D)
    assert _err(y, unchanged) > 1e-2                        # (the new taps were used)
    import libsdr_amd as sa
    bad = other.copy()
    bad[3] = np.inf
    with pytest.raises(sa.SdrHipError) as e:
        node.set_taps(bad)
    assert e.value.code == sa.abi.E_INVALID
    node.close()


@pytest.mark.hostptr_only
def test_host_pointer_staging_grows_with_the_selection(ctx):
    """The first host-pointer call stages two rows; set_channels then raises the rows to M, and the staged output has to regrow:
    calls of 1, 7 and 23 samples (blocks of D with a remainder), one of T + 1 outputs (two workgroups) and the rest."""
    shape, dtype = (6, 4, 14), "cs16"
    M, D, _ = shape
    taps, x, _, ref = _case(shape, dtype)
    lens = [1, 7, 23, (tile_times(M) + 1) * D]
    lens.append(len(x) - sum(lens))
    node = _node(ctx, shape, dtype, taps, len(x), channels=[4, 1])
    y2 = _run(node, x, lens)
    assert y2.shape == (2, ref.shape[1], 2) and _err(y2, ref[[4, 1]]) <= BOUND
    node.reset()
    node.set_channels(None)
    assert node.plan_info()["rows"] == M
    y = _run(node, x, lens)
    err = _err(y, ref)
    print("channelizer %s %s, rows 2 -> %d through the staging: %.3g" % (shape, dtype, M, err))
    assert y.shape == (M, ref.shape[1], 2) and err <= BOUND, err
    assert same(y[[4, 1]], y2)
    node.reset()
    assert same(node.process(x), y)                         # one call of max_in samples: the largest staged output
    node.close()


@pytest.mark.hostptr_only
def test_host_pointer_calls_and_refusals(ctx):
    import libsdr_amd as sa
    from libsdr_amd import abi
    shape, dtype = (12, 6, 30), "cs16"
    M, D, _ = shape
    taps, x, lens, ref = _case(shape, dtype)
    n = len(x)
    node = _node(ctx, shape, dtype, taps, n)
    y = _run(node, x, lens)
    assert _err(y, ref) <= BOUND
    node.reset()
    node.set_channels([7, 2])
    assert same(node.process(x), y[[7, 2]])                 # (the staged rows follow the selection)
    node.set_channels(None)
    node.reset()
    assert same(node.process(x), y)
    for idx in ([], [0, 12], [-1], [3, 3], list(range(12)) + [0]):
        with pytest.raises(sa.SdrHipError) as e:
            node.set_channels(idx)
        assert e.value.code == abi.E_INVALID
    assert node.plan_info()["rows"] == M
    # refusals change nothing
    state = node.get_state()
    no = node.out_count(60)
    out = np.full((M, no, 2), 7, np.float32)
    p = lambda a: a.ctypes.data
    xs = np.ascontiguousarray(x[:60])
    assert node._c_process(node._h, p(xs), 60, p(out), no - 1, None) == abi.E_SIZE        # an out stride below the count
    assert node._c_process(node._h, p(xs), n + 1, p(out), no, None) == abi.E_SIZE         # above max_in
    assert node._c_process(node._h, None, 60, p(out), no, None) == abi.E_INVALID
    din, dout = ctx.malloc(xs.nbytes), ctx.malloc(out.nbytes)
    try:
        assert node._c_process_dev(node._h, din, 60, dout, no - 1, None) == abi.E_SIZE
        assert node._c_process_dev(node._h, din, 60, din, no, None) == abi.E_INVALID      # the output over the input
    finally:
        ctx.free(din)
        ctx.free(dout)
    tail = np.zeros((4, 2), np.float32)
    assert node._c_get_state(node._h, None, tail.ctypes.data_as(C.POINTER(C.c_float)), 4) == abi.E_SIZE
    after = node.get_state()
    assert after["consumed"] == state["consumed"] and same(after["tail"], state["tail"]) and np.all(out == 7)
    node.close()

