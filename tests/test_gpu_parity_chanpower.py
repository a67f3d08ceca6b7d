"""GPU parity of the channel power monitor (include/sdrhip_chanpower.h). Per shape and input type, a stream cut into calls:
  1  every call's sums against the numpy float64 restatement (tests/chanpower_restatement.py on the float32-rounded taps):
     max |sum - ref| / max ref <= 1e-5, the project's bound for its float paths;
  2  every call's sums against the PLAIN channelizer's float32 rows of the same calls on the same device, squared and added in
     numpy float64: per channel |sum - ref| <= 1e-12 ref (the terms are non-negative, so any summation order is within
     (J - 1) 2^-53 < 1e-13 for J <= 769) — the monitor sees the channelizer's spectra;
  3  level, open and occupied after every call against the restatement's state step fed the DEVICE's sums: levels bit for bit;
  4  the same under SDRHIP_CHANPOWER_GRID = 1 and 3 (four tiles: the tile loop, and an uneven share of the tiles);
  5  process_dev with a NULL sum leaves the same state;  6  reset against a fresh handle, bit for bit;
  7  set_taps / set_alpha / set_thresholds between calls;  8  a NaN sample on a cf32 row;  9  the host-pointer path;
  10 kernel_names.
By its name the module runs in the red-zoned arena: the sums are ONE output row of M doubles cut from the arena, guard bands
checked after every call. The restatement's answers and the plain channelizer's rows are computed once per shape and type."""
import functools

import numpy as np
import pytest

import channelizer_restatement as R
import chanpower_restatement as P

pytestmark = pytest.mark.gpu

BOUND, BOUND_ROWS = 1e-5, 1e-12
# (M, D, n_taps): the smallest, a D that divides nothing, mixed radix (12 = 4 * 3, 1000 = 5^3 * 4 * 2, 182 = 13 * 7 * 2), n_taps
# below M, a multiple of M and one above a multiple; M = 182 and 1000 are no multiple of the 256 lanes that share the channels,
# M = 4096 gives every lane 16 of them and takes more than 64 KiB of LDS
SHAPES = [(2, 2, 3), (8, 3, 21), (12, 6, 30), (64, 32, 64), (182, 77, 500), (1000, 500, 3000), (4096, 2048, 4097)]
DTYPES = ["cs16", "cf32"]
ALPHA = 0.375


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


def _counts(lens, D):
    """the outputs of every call"""
    off, out = 0, []
    for n in lens:
        out.append((off + n) // D - off // D)
        off += n
    return out


def _per_call(e, counts):
    """[M, n_out] float64 terms -> the sums of every call [calls, M]"""
    out, j = [], 0
    for c in counts:
        out.append(e[:, j:j + c].sum(axis=1))
        j += c
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """(taps, x, lens, counts, the restatement's sums per call [calls, M] float64, thresholds) of a shape: 3 T + 1 output times,
    four tiles. The thresholds come from the restatement: open at the median over the channels of its level behind the last call,
    close at half of it, so that some flags open and some do not."""
    M, D, n_taps = shape
    n = (3 * tile_times(M) + 1) * D
    taps, x = _taps(M, n_taps), _signal(dtype, n, 17 * M + D + n_taps)
    lens = _lens(n, D)
    counts = _counts(lens, D)
    y = R.folded(R.pairs(x), R.round32(taps), M, D)
    ref = _per_call(y.real * y.real + y.imag * y.imag, counts)
    ref.setflags(write=False)
    free = P.Monitor(taps, M, D, ALPHA)
    for s, J in zip(ref, counts):
        free.update(s, J)
    thr = float(np.median(free.level))
    return taps, x, lens, counts, ref, (thr, 0.5 * thr)


_ROWS = {}


def _channelizer_sums(ctx, shape, dtype):
    """the PLAIN channelizer's float32 rows of the same calls on this device, squared and added in float64: [calls, M]"""
    if (shape, dtype) not in _ROWS:
        import libsdr_amd as sa
        taps, x, lens, counts, _, _ = _case(shape, dtype)
        node = sa.Channelizer(ctx, np.int16 if dtype == "cs16" else np.float32, shape[0], shape[1], taps, max_in=len(x))
        parts, off = [], 0
        for n in lens:
            parts.append(node.process(x[off:off + n]).astype(np.float64))
            off += n
        node.close()
        rows = np.concatenate(parts, axis=1)
        sums = _per_call(rows[..., 0] * rows[..., 0] + rows[..., 1] * rows[..., 1], counts)
        sums.setflags(write=False)
        _ROWS[shape, dtype] = sums
    return _ROWS[shape, dtype]


def _node(ctx, shape, dtype, taps, max_in, grid=None, alpha=ALPHA):
    import libsdr_amd as sa
    M, D, n_taps = shape
    node = sa.ChannelPower(ctx, np.int16 if dtype == "cs16" else np.float32, M, D, taps, alpha=alpha, max_in=max_in)
    assert node.kernel_names == ["chanpower_%s_kernel" % dtype, "chanpower_finish_kernel"]
    info = node.plan_info()
    assert info["tile_times"] == tile_times(M) and info["branch_taps"] == -(-n_taps // M) and info["lds_bytes"] == tile_times(M) * (M + 1) * 8
    tiles = -(-(-(-max_in // D)) // tile_times(M))
    assert info["grid"] == (min(grid, tiles) if grid else tiles) and info["partial_bytes"] == info["grid"] * M * 8   # (few tiles here)
    return node


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def _run(node, x, lens, model=None, thresholds=None):
    """every call's sums [calls, M]; with a model (the restatement's state step), check 3 after every call"""
    sums, off = [], 0
    if thresholds is not None:
        node.set_thresholds(*thresholds)
        if model is not None:
            model.set_thresholds(*thresholds)
    for n in lens:
        J = node.out_count(n)
        assert J == (off + n) // node.D - off // node.D
        s = node.process(x[off:off + n])
        off += n
        assert s.shape == (node.M,) and s.dtype == np.float64
        if J == 0:
            assert not s.any()
        sums.append(s)
        if model is not None:
            model.update(s, J)
            level, flags = node.levels()
            assert same(level, model.level), (n, np.abs(level - model.level).max())
            assert np.array_equal(flags, model.open) and node.occupied() == model.occupied()
            assert node.get_state()["calls"] == model.calls
    return np.array(sums)


def _check_rows(sums, rows):
    worst = 0.0
    for s, r in zip(sums, rows):
        assert np.all(np.abs(s - r) <= BOUND_ROWS * r), float((np.abs(s - r) / np.maximum(r, 1e-300)).max())
        if r.max() > 0:
            worst = max(worst, float((np.abs(s - r) / np.maximum(r, 1e-300)).max()))
    return worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_split_stream_against_the_restatement_and_the_channelizer(ctx, shape, dtype):
    from redzone import RedZone
    M, D, n_taps = shape
    taps, x, lens, counts, ref, thr = _case(shape, dtype)
    rows = _channelizer_sums(ctx, shape, dtype)
    n, before = len(x), RedZone.calls
    node, model = _node(ctx, shape, dtype, taps, n), P.Monitor(taps, M, D, ALPHA)
    sums = _run(node, x, lens, model, thr)
    assert RedZone.calls - before == len([v for v in lens if v])          # (a call with J = 0 is guarded too: it writes zeros)
    assert sums.shape == ref.shape == (len(lens), M) and model.calls == len([c for c in counts if c])
    err = float(np.abs(sums - ref).max() / ref.max())
    worst = _check_rows(sums, rows)
    print("chanpower %s %s: max |sum - ref| / max ref = %.3g; against the channelizer's rows %.3g; %d of %d open"
          % (shape, dtype, err, worst, len(model.occupied()), M))
    assert err <= BOUND, err
    assert 0 < len(model.occupied()) and (len(model.occupied()) < M or M == 2)   # (the flags were worth comparing)
    s = node.get_state()
    assert s["consumed"] == n and s["calls"] == model.calls
    level, flags = node.levels()
    # 5: the state alone, through raw device pointers with a NULL sum, on a handle of its own
    quiet = _node(ctx, shape, dtype, taps, n)
    quiet.set_thresholds(*thr)
    din = ctx.malloc(max(x.nbytes, 16))
    try:
        off = 0
        for k, v in enumerate(lens):
            if v:
                ctx.h2d(din, np.ascontiguousarray(x[off:off + v]))
            assert quiet.process_dev(din, v) == counts[k]
            ctx.synchronize()
            off += v
    finally:
        ctx.free(din)
    ql, qf = quiet.levels()
    assert same(ql, level) and np.array_equal(qf, flags) and quiet.occupied() == node.occupied()
    assert quiet.get_state()["calls"] == s["calls"] and quiet.get_state()["consumed"] == n
    quiet.close()
    # 6: reset — the levels, flags and calls go, the thresholds stay — and the same stream again, bit for bit
    node.reset()
    level0, flags0 = node.levels()
    assert not level0.any() and not flags0.any() and node.occupied() == []
    assert node.get_state()["consumed"] == 0 and node.get_state()["calls"] == 0 and not node.get_state()["tail"].any()
    again = _run(node, x, lens)
    assert same(again, sums)
    level2, flags2 = node.levels()
    assert same(level2, level) and np.array_equal(flags2, flags)
    node.close()


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_a_bounded_grid_walks_the_tiles(ctx, shape, dtype, grid, monkeypatch):
    M, D, n_taps = shape
    taps, x, lens, counts, ref, thr = _case(shape, dtype)
    rows = _channelizer_sums(ctx, shape, dtype)
    monkeypatch.setenv("SDRHIP_CHANPOWER_GRID", str(grid))
    node = _node(ctx, shape, dtype, taps, len(x), grid=grid)
    assert node.plan_info()["grid"] == grid
    model = P.Monitor(taps, M, D, ALPHA)
    sums = _run(node, x, lens, model, thr)
    _check_rows(sums, rows)
    assert float(np.abs(sums - ref).max() / ref.max()) <= BOUND
    node.close()


@pytest.mark.parametrize("shape,dtype", [((12, 6, 30), "cf32"), ((64, 32, 64), "cs16")], ids=["12-6-30-cf32", "64-32-64-cs16"])
def test_setters_between_calls(ctx, shape, dtype):
    import libsdr_amd as sa
    M, D, n_taps = shape
    taps, x, _, _, _, thr = _case(shape, dtype)
    other = _taps(M, n_taps)[::-1] * np.linspace(0.5, 1.5, n_taps)
    cuts = [0, 5 * D + 1, 11 * D, 40 * D + 3, len(x)]
    node, ref = _node(ctx, shape, dtype, taps, len(x)), P.Monitor(taps, M, D, ALPHA)
    dev = P.Monitor(taps, M, D, ALPHA)              # the state step alone, fed the device's sums
    steps = [lambda v: v.set_thresholds(*thr), lambda v: v.set_taps(other), lambda v: v.set_alpha(1.0),
             lambda v: v.set_thresholds(np.linspace(2.0, 0.5, M) * thr[0], 0.25 * thr[0])]
    for k in range(4):
        for v in (node, ref, dev):
            steps[k](v)
        chunk = x[cuts[k]:cuts[k + 1]]
        J = node.out_count(len(chunk))
        s, w = node.process(chunk), ref.process(chunk)
        dev.update(s, J)
        err = float(np.abs(s - w).max() / w.max())
        assert err <= BOUND, (k, err)
        level, flags = node.levels()
        assert same(level, dev.level) and np.array_equal(flags, dev.open) and node.occupied() == dev.occupied(), k
        assert np.abs(level - ref.level).max() <= BOUND * ref.level.max()
    assert node.get_state()["consumed"] == len(x) and node.get_state()["calls"] == 4
    # refusals change nothing
    before = (node.levels(), node.occupied())
    for bad in ((np.ones(M), 2.0 * np.ones(M)), (1.0, -1.0), (np.nan, 0.0), (1.0, np.nan)):
        with pytest.raises(sa.SdrHipError) as e:
            node.set_thresholds(*bad)
        assert e.value.code == sa.abi.E_INVALID
    for bad in (0.0, 1.5, np.nan):
        with pytest.raises(sa.SdrHipError) as e:
            node.set_alpha(bad)
        assert e.value.code == sa.abi.E_INVALID
    worse = other.copy()
    worse[3] = np.inf
    with pytest.raises(sa.SdrHipError):
        node.set_taps(worse)
    assert node.alpha == 1.0
    assert same(node.levels()[0], before[0][0]) and np.array_equal(node.levels()[1], before[0][1]) and node.occupied() == before[1]
    chunk = x[:7 * D]
    J = node.out_count(len(chunk))
    s = node.process(chunk)
    dev.update(s, J)
    assert same(node.levels()[0], dev.level) and np.array_equal(node.levels()[1], dev.open)   # (the old thresholds and alpha held)
    node.close()


def test_thresholds_hold_from_the_next_call_on(ctx):
    """set_thresholds leaves level and open as the last call left them — thresholds under which every flag would flip — and the
    next call applies them. Calls of 1, 7 and 23 samples, one of T + 1 outputs (two tiles), the rest."""
    shape, dtype = (6, 4, 14), "cs16"
    M, D, _ = shape
    taps, x, _, _, _, thr = _case(shape, dtype)
    lens = [1, 7, 23, (tile_times(M) + 1) * D]
    lens.append(len(x) - sum(lens))
    node, ref, dev = _node(ctx, shape, dtype, taps, len(x)), P.Monitor(taps, M, D, ALPHA), P.Monitor(taps, M, D, ALPHA)
    # (no output); every flag opens; every flag closes; opens; the restatement's median level decides
    settings = [(0.0, 0.0), (0.0, 0.0), (np.inf, np.inf), (0.0, 0.0), thr]
    off = 0
    for n, t in zip(lens, settings):
        level, flags = node.levels()
        for v in (node, ref, dev):
            v.set_thresholds(*t)
        after = node.levels()
        assert same(after[0], level) and np.array_equal(after[1], flags) and np.array_equal(flags, dev.open)   # not this call's
        J = node.out_count(n)
        s, w = node.process(x[off:off + n]), ref.process(x[off:off + n])
        off += n
        dev.update(s, J)
        assert (np.abs(s - w).max() <= BOUND * w.max()) if J else not s.any()
        level, flags = node.levels()
        assert same(level, dev.level) and np.array_equal(flags, dev.open) and node.occupied() == dev.occupied(), n
        if t == (0.0, 0.0) or t == (np.inf, np.inf):
            assert np.array_equal(flags, np.full(M, bool(J) and t[0] == 0.0))
    assert dev.calls == 4 == node.get_state()["calls"]
    node.close()


def test_a_nan_sample_on_a_float_row(ctx):
    shape, dtype = (12, 6, 30), "cf32"
    M, D, n_taps = shape
    taps, x, _, _, _, _ = _case(shape, dtype)
    cpu = P.Monitor(taps, M, D, ALPHA)
    cpu.process(x[:20 * D])
    thr = float(np.median(cpu.level))               # the first call's level is its mean: about half the channels open
    node = _node(ctx, shape, dtype, taps, len(x))
    node.set_thresholds(thr, 0.5 * thr)
    first = node.process(x[:20 * D])
    level, flags = node.levels()
    assert flags.any() and not flags.all() and np.isfinite(level).all()
    bad = x[20 * D:40 * D].copy()
    bad[7, 1] = np.nan
    s = node.process(bad)
    assert np.isnan(s).all()                        # the transform spreads it to every channel
    level, after = node.levels()
    assert np.isnan(level).all() and np.array_equal(after, flags)
    clean = node.process(x[40 * D:60 * D])           # the stream is clean again (n_taps - 1 < 20 D), the levels are not
    assert np.isfinite(clean).all()
    level, after = node.levels()
    assert np.isnan(level).all() and np.array_equal(after, flags) and node.get_state()["calls"] == 3
    node.reset()
    assert same(node.process(x[:20 * D]), first)
    level, after = node.levels()
    assert np.isfinite(level).all() and np.array_equal(after, flags)
    node.close()


@pytest.mark.hostptr_only
def test_host_pointer_calls_and_refusals(ctx):
    import ctypes as C
    from libsdr_amd import abi
    shape, dtype = (12, 6, 30), "cs16"
    M, D, _ = shape
    taps, x, lens, counts, ref, thr = _case(shape, dtype)
    rows = _channelizer_sums(ctx, shape, dtype)
    n = len(x)
    node, model = _node(ctx, shape, dtype, taps, n), P.Monitor(taps, M, D, ALPHA)
    sums = _run(node, x, lens, model, thr)
    _check_rows(sums, rows)
    assert float(np.abs(sums - ref).max() / ref.max()) <= BOUND
    # refusals change nothing
    state, levels = node.get_state(), node.levels()
    out = np.full(M, 7.0)
    p = lambda a: a.ctypes.data
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    xs = np.ascontiguousarray(x[:60])
    assert node._c_process(node._h, p(xs), n + 1, dp(out), None) == abi.E_SIZE           # above max_in
    assert node._c_process(node._h, None, 60, dp(out), None) == abi.E_INVALID
    assert node._c_process(node._h, p(xs), 60, None, None) == abi.E_INVALID              # the host call wants its sums
    din = ctx.malloc(xs.nbytes)
    try:
        assert node._c_process_dev(node._h, din, 60, din + 8, None) == abi.E_INVALID     # the sums over the input
        assert node._c_process_dev(node._h, None, 60, None, None) == abi.E_INVALID
    finally:
        ctx.free(din)
    short = np.zeros(M - 1)
    assert node._c_get_levels(node._h, dp(short), None, M - 1) == abi.E_SIZE
    few, cnt = np.full(2, -1, np.intc), C.c_int(-1)
    assert node._c_get_occupied(node._h, few.ctypes.data_as(C.POINTER(C.c_int)), 1, C.byref(cnt)) == abi.OK
    occ = node.occupied()
    assert cnt.value == len(occ) >= 2 and few.tolist() == [occ[0], -1]                   # the full count, cap indices written
    assert node._c_get_occupied(node._h, None, 0, C.byref(cnt)) == abi.OK and cnt.value == len(occ)
    after = node.get_state()
    assert after["consumed"] == state["consumed"] and after["calls"] == state["calls"] and np.all(out == 7.0)
    assert same(node.levels()[0], levels[0]) and np.array_equal(node.levels()[1], levels[1])
    node.close()
