"""GPU parity of the polyphase synthesis bank (include/sdrhip_synthesis.h) against its numpy float64 restatement
(tests/synthesis_restatement.py) on the float32-rounded taps: max |z - ref| / max |ref| <= 1e-5, the project's bound for its
float / FFT paths; where M >= 1000 also against the definition on a few hundred output times. Bit for bit: any cut of the columns
into calls (calls of 0 and 1 column among them) against one call, the stream after reset against a fresh handle, a selection
against the all-rows call given zero rows for the other channels, rows and idx permuted together. get_state after every call,
the setters between calls against Stream, one NaN column (which pins the skipped terms), the refusals. By its name the module
runs in the red-zoned arena (device-pointer calls, strided input rows, guard bands around the input rows and the output row
checked after every call); the tests marked hostptr_only take the host-pointer path and compare it with the device-pointer one.
The restatement's answers are computed once per shape and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import synthesis_restatement as R

pytestmark = pytest.mark.gpu

BOUND = 1e-5


def tile_times(M):
    """the header's rule"""
    return min(256, (4096 if M <= 512 else 8192) // M)


SEL64 = sorted(int(k) for k in np.random.default_rng(64).choice(1024, 64, replace=False))
# name -> (M, D, n_taps, channels, columns per call)
SHAPES = {
    "8-8-17": (8, 8, 17, None, (0, 1, 9)),
    "12-5-30": (12, 5, 30, (3, 0, 11), (11,)),
    "26-26-52": (26, 26, 52, None, (5,)),
    "77-40-300": (77, 40, 300, (76, 1), (7,)),
    "6-1-7": (6, 1, 7, None, (20,)),                                # Q = 7
    "16-2-128": (16, 2, 128, (5,), (70,)),                          # Q = 64
    "16-16-5": (16, 16, 5, None, (6,)),                             # n_taps < D: outputs with no term
    "1024-512-4096": (1024, 512, 4096, None, (16,)),
    "1024-512-4096-sel64": (1024, 512, 4096, tuple(SEL64), (16,)),
    "4096-4096-8192": (4096, 4096, 8192, None, (3,)),               # more than 64 KiB of LDS
    "64-32-100-tile": (64, 32, 100, None, (tile_times(64) + 1,)),   # a tile boundary inside the call
    "12-5-30-tile": (12, 5, 30, (3, 0, 11), (tile_times(12) + 1,)),
}


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


def _taps(M, D, n_taps):
    """a windowed sinc of cutoff fs / (2 M) with the interpolation's gain, as doubles (any finite prototype would do)"""
    t = np.arange(n_taps) - (n_taps - 1) / 2
    return np.sinc(t / M) * np.hanning(n_taps + 2)[1:-1] * D / M


@functools.lru_cache(maxsize=None)
def _case(name):
    """(taps, x [rows, n, 2] float32, folded reference [n D] complex128) of a shape"""
    M, D, n_taps, channels, lens = SHAPES[name]
    rows, n = M if channels is None else len(channels), sum(lens)
    rng = np.random.default_rng(17 * M + D + n_taps + rows)
    x = (0.5 * rng.standard_normal((rows, n, 2))).astype(np.float32)
    taps = _taps(M, D, n_taps)
    ref = R.folded(R.rows_of(x), R.round32(taps), M, D, channels)
    for a in (x, ref):
        a.setflags(write=False)
    return taps, x, ref


def _node(ctx, name, max_in, channels="shape"):
    import libsdr_amd as sa
    M, D, n_taps, sel, _ = SHAPES[name]
    sel = sel if channels == "shape" else channels
    node = sa.Synthesis(ctx, M, D, _taps(M, D, n_taps), channels=None if sel is None else list(sel), max_in=max_in)
    assert node.kernel_names == ["synthesis_transform_kernel", "synthesis_overlap_kernel"]
    info = node.plan_info()
    assert info == {"tile_times": tile_times(M), "branch_taps": -(-n_taps // D), "lds_bytes": tile_times(M) * (M + 1) * 8, "rows": node.channels}
    return node


def _run(node, x, lens, each=None):
    """the calls of lens, one after the other -> [n D, 2]; each(columns so far) behind every call"""
    parts, off = [], 0
    for n in lens:
        assert node.out_count(n) == n * node.D
        parts.append(node.process(x[:, off:off + n]))
        off += n
        if each:
            each(off)
    return np.concatenate(parts)


def _err(z, ref):
    """max |z - ref| / max |ref| of float32 [..., 2] against complex128 [...]"""
    got = z[..., 0].astype(np.float64) + 1j * z[..., 1].astype(np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def _cuts(n):
    """cuts of n columns into calls, calls of 0 and 1 column among them"""
    cuts = [[1] * n if n <= 20 else [1, n - 2, 1], [0, 1, 0, n - 1], [n - n // 2, 0, n // 2]]
    return [c for c in cuts if all(k >= 0 for k in c)]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_split_stream_against_the_restatement(ctx, name):
    from redzone import RedZone
    M, D, n_taps, channels, lens = SHAPES[name]
    taps, x, ref = _case(name)
    n, Q, before = x.shape[1], -(-n_taps // D), RedZone.calls
    node, stream = _node(ctx, name, n), R.Stream(taps, M, D, channels)
    if name.endswith("tile"):
        assert n == node.plan_info()["tile_times"] + 1
    fed = [0]

    def state_follows(off):
        """the count is exact, the columns are within the tolerance"""
        stream.process(R.rows_of(x[:, fed[0]:off]))
        fed[0] = off
        s, (consumed, cols) = node.get_state(), stream.state()
        assert s["consumed"] == off == consumed and s["cols"].shape == (Q - 1, M, 2)
        if Q > 1 and np.abs(cols).max() > 0:
            assert _err(s["cols"], cols) <= BOUND
            assert not s["cols"][:max(Q - 1 - off, 0)].any()          # zeros where the stream is shorter
        else:
            assert not s["cols"].any()

    z = _run(node, x, lens, state_follows)
    assert RedZone.calls - before == len([k for k in lens if k])      # every call with columns ran in the arena
    err = _err(z, ref)
    print("synthesis %s: max |z - folded| / max |folded| = %.3g" % (name, err))
    assert z.shape == (n * D, 2) and err <= BOUND, err
    if M >= 1000:
        rng = np.random.default_rng(M)
        times = np.unique(np.concatenate([[0, 1, D - 1, D, n * D - 1], rng.integers(0, n * D, 300)]))
        d = R.direct(R.rows_of(x), R.round32(taps), M, D, channels, times)
        err_d = float(np.abs((z[times, 0].astype(np.float64) + 1j * z[times, 1]) - d).max() / np.abs(ref).max())
        print("synthesis %s: max |z - direct| / max |folded| = %.3g over %d output times" % (name, err_d, len(times)))
        assert err_d <= BOUND, err_d
    if n_taps < D:                                                    # outputs with no term are exactly 0
        assert not z.reshape(n, D, 2)[:, n_taps:].any()
    # bit for bit: one call on a fresh handle; other cuts on the same handle after reset
    one = _node(ctx, name, n)
    assert same(one.process(x), z)
    for cut in _cuts(n):
        node.reset()
        s = node.get_state()
        assert s["consumed"] == 0 and not s["cols"].any()
        assert same(_run(node, x, cut), z), cut
    # rows and idx permuted together
    sel = list(range(M)) if channels is None else list(channels)
    perm = np.random.default_rng(n_taps).permutation(len(sel))
    one.reset()
    one.set_channels([sel[i] for i in perm])
    assert same(one.process(x[perm]), z)
    # a selection against the all-rows call given zero rows for the other channels
    if channels is not None:
        full = np.zeros((M, n, 2), np.float32)
        full[list(channels)] = x
        one.reset()
        one.set_channels(None)
        assert one.plan_info()["rows"] == M
        assert same(one.process(full), z)
    node.close()
    one.close()


def test_setters_between_calls(ctx):
    for name in ("12-5-30", "16-2-128"):
        _setters_between_calls(ctx, name)


def _setters_between_calls(ctx, name):
    M, D, n_taps, channels, _ = SHAPES[name]
    taps, x, ref = _case(name)
    n = x.shape[1]
    other = taps[::-1] * np.linspace(0.5, 1.5, n_taps)
    sel2 = [channels[0], (channels[0] + 1) % M] if len(channels) == 1 else list(channels[::-1][:2])
    x2 = x[:len(sel2)] if len(sel2) <= len(x) else np.concatenate([x, x[:1] * 0.5])
    cut1, cut2 = n // 3, 2 * n // 3
    node, stream = _node(ctx, name, n), R.Stream(taps, M, D, channels)
    got, want = [node.process(x[:, :cut1])], [stream.process(R.rows_of(x[:, :cut1]))]
    node.set_taps(other)
    stream.set_taps(other)
    got.append(node.process(x[:, cut1:cut2]))
    want.append(stream.process(R.rows_of(x[:, cut1:cut2])))
    node.set_channels(sel2)
    stream.set_channels(sel2)
    assert node.plan_info()["rows"] == len(sel2)
    got.append(node.process(x2[:, cut2:]))
    want.append(stream.process(R.rows_of(x2[:, cut2:])))
    assert node.get_state()["consumed"] == n == stream.state()[0]
    z, w = np.concatenate(got), np.concatenate(want)
    err = _err(z, w)
    print("synthesis setters %s: %.3g" % (name, err))
    assert err <= BOUND, err
    assert _err(z, ref) > 1e-2                                        # (the new taps and rows were used)
    import libsdr_amd as sa
    bad = other.copy()
    bad[3] = np.inf
    with pytest.raises(sa.SdrHipError) as e:
        node.set_taps(bad)
    assert e.value.code == sa.abi.E_INVALID
    node.close()


def test_one_nan_column(ctx):
    """The outputs are non-finite exactly for t in [m D, m D + n_taps) and equal the restatement elsewhere: a term at
    q D + d >= n_taps is skipped, not multiplied by a padded zero (0 * NaN would spread the column further). Shapes with
    n_taps no multiple of D, n_taps < D and Q = 64."""
    for name, m in (("77-40-300", 1), ("16-16-5", 3), ("16-2-128", 20)):
        _one_nan_column(ctx, name, m)


def _one_nan_column(ctx, name, m):
    M, D, n_taps, channels, _ = SHAPES[name]
    taps = _taps(M, D, n_taps)
    rows, n = M if channels is None else len(channels), m + -(-n_taps // D) + 3
    rng = np.random.default_rng(m)
    x = (0.5 * rng.standard_normal((rows, n, 2))).astype(np.float32)
    clean = x.copy()
    clean[:, m] = 0
    x[rows // 2, m] = np.nan
    ref = R.folded(R.rows_of(clean), R.round32(taps), M, D, channels)
    node = _node(ctx, name, n)
    z = node.process(x)
    t = np.arange(n * D)
    hit = (t >= m * D) & (t < m * D + n_taps)
    assert hit.any() and (~hit).any()
    # (a complex value is non-finite where a component is)
    assert (~np.isfinite(z[hit])).any(axis=1).all() and np.isfinite(z[~hit]).all(), name
    assert _err(z[~hit], ref[~hit]) <= BOUND, name
    node.close()


def _dev_call(ctx, node, x, in_stride=0):
    """x through process_dev on device buffers of the test's own -> [n D, 2]"""
    rows, n = x.shape[0], x.shape[1]
    stride = in_stride or n
    host = np.zeros((rows, stride, 2), np.float32)
    host[:, :n] = x
    out = np.zeros((n * node.D, 2), np.float32)
    din, dout = ctx.malloc(max(host.nbytes, 16)), ctx.malloc(max(out.nbytes, 16))
    try:
        ctx.h2d(din, host)
        assert node.process_dev(din, n, in_stride, dout) == n * node.D
        ctx.synchronize()
        ctx.d2h(out, dout)
    finally:
        ctx.free(din)
        ctx.free(dout)
    return out


@pytest.mark.hostptr_only
def test_host_pointer_path_equals_the_device_pointer_path(ctx):
    """The host-pointer calls of a cut stream, bit for bit the device-pointer call's; the staged input rows regrow when
    set_channels raises the rows from 3 to M."""
    name = "12-5-30"
    M, D, n_taps, channels, _ = SHAPES[name]
    taps, x, ref = _case(name)
    n = x.shape[1]
    node = _node(ctx, name, n)
    z = _run(node, x, [1, 0, 4, n - 5])
    assert _err(z, ref) <= BOUND
    dev = _node(ctx, name, n)
    assert same(_dev_call(ctx, dev, x), z)
    dev.reset()
    assert same(_dev_call(ctx, dev, x, in_stride=n + 7), z)           # strided rows
    full = np.zeros((M, n, 2), np.float32)
    full[list(channels)] = x
    node.reset()
    node.set_channels(None)
    assert same(_run(node, full, [n]), z)                             # one call of max_in columns of M rows: the largest staged input
    node.close()
    dev.close()


@pytest.mark.hostptr_only
def test_refusals_change_nothing(ctx):
    import libsdr_amd as sa
    from libsdr_amd import abi
    name = "12-5-30"
    M, D, n_taps, channels, _ = SHAPES[name]
    taps, x, ref = _case(name)
    n = x.shape[1]
    node = _node(ctx, name, n)
    node.process(x[:, :6])
    for idx in ([], [0, 12], [-1], [3, 3], list(range(12)) + [0]):
        with pytest.raises(sa.SdrHipError) as e:
            node.set_channels(idx)
        assert e.value.code == abi.E_INVALID
    assert node.plan_info()["rows"] == 3
    state = node.get_state()
    xs = np.ascontiguousarray(x[:, 6:10])
    out = np.full((4 * D, 2), 7, np.float32)
    p = lambda a: a.ctypes.data
    assert node._c_process(node._h, p(xs), 4, 3, p(out), None) == abi.E_SIZE              # an input stride below n
    assert node._c_process(node._h, p(xs), n + 1, 0, p(out), None) == abi.E_SIZE          # above max_in
    assert node._c_process(node._h, None, 4, 0, p(out), None) == abi.E_INVALID
    assert node._c_process(node._h, p(xs), 4, 0, None, None) == abi.E_INVALID
    din, dout = ctx.malloc(xs.nbytes), ctx.malloc(out.nbytes)
    try:
        assert node._c_process_dev(node._h, din, 4, 3, dout, None) == abi.E_SIZE
        assert node._c_process_dev(node._h, din, n + 1, 0, dout, None) == abi.E_SIZE
        assert node._c_process_dev(node._h, din, 4, 0, din + 8, None) == abi.E_INVALID    # the output over the input
        got = C.c_size_t(9)
        assert node._c_process_dev(node._h, din, 0, 0, dout, C.byref(got)) == abi.OK and got.value == 0   # n = 0 is legal
    finally:
        ctx.free(din)
        ctx.free(dout)
    cols = np.zeros((4, 2), np.float32)
    assert node._c_get_state(node._h, None, cols.ctypes.data_as(C.POINTER(C.c_float)), 4) == abi.E_SIZE
    after = node.get_state()
    assert after["consumed"] == state["consumed"] == 6 and same(after["cols"], state["cols"]) and np.all(out == 7)
    assert _err(node.process(x[:, 6:]), ref[6 * D:]) <= BOUND                             # the stream went on where it was
    node.close()
