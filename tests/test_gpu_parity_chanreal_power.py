"""GPU parity of the channel power monitor for a real-sampled row (include/sdrhip_chanreal.h, ChannelPower(real=True)). Per
shape and input type, a stream cut into calls:
  1  every call's sums against the numpy float64 restatement (tests/chanreal_restatement.py, folded_real, squared and added):
     max |sum - ref| / max ref <= 1e-5;
  2  every call's sums against the REAL PLAIN channelizer's float32 rows of the same calls on the same device, squared and added
     in numpy float64: per channel |sum - ref| <= 1e-12 ref (non-negative terms: any order is within (J - 1) 2^-53) — the
     monitor sees the channelizer's spectra;
  3  level, open and occupied after every call against chanpower_restatement.Monitor.update fed the DEVICE's sums: levels bit
     for bit;
  4  the same under SDRHIP_CHANPOWER_GRID = 1 and 3 (four tiles: the tile loop, and an uneven share of the tiles);
  5  reset against the first run, bit for bit;  6  occupied() handed to a real Channelizer.set_channels;  7  kernel_names.
By its name the module runs in the red-zoned arena: the sums are ONE output row of K = M / 2 + 1 doubles cut from the arena."""
import functools

import numpy as np
import pytest

import chanpower_restatement as P
import chanreal_restatement as RR

pytestmark = pytest.mark.gpu

BOUND, BOUND_ROWS = 1e-5, 1e-12
SHAPES = [(8, 8, 24), (64, 32, 64), (1000, 500, 3000)]
DTYPES = ["s16", "f32"]
NP = {"s16": np.int16, "f32": np.float32}
ALPHA = 0.375


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


def _counts(lens, D):
    off, out = 0, []
    for n in lens:
        out.append((off + n) // D - off // D)
        off += n
    return out


def _per_call(e, counts):
    """[K, n_out] float64 terms -> the sums of every call [calls, K]"""
    out, j = [], 0
    for c in counts:
        out.append(e[:, j:j + c].sum(axis=1))
        j += c
    return np.array(out)


def _model(taps, M, D):
    """the state step alone, over the K channels (its own stream is not used)"""
    return P.Monitor(taps, M // 2 + 1, D, ALPHA)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """(taps, x, lens, counts, the restatement's sums per call [calls, K], thresholds): 3 T + 1 output times, four tiles. The
    thresholds come from the restatement: open at the median over the channels of its level behind the last call, close at half."""
    M, D, n_taps = shape
    n = (3 * RR.tile_times(M) + 1) * D
    rng = np.random.default_rng(17 * M + D + n_taps)
    x = rng.integers(-20000, 20000, n).astype(np.int16) if dtype == "s16" else (0.5 * rng.standard_normal(n)).astype(np.float32)
    taps = RR.prototype(M, n_taps)
    head = [0, 1, D - 1, D + 1]
    lens = head + [n - sum(head)]
    counts = _counts(lens, D)
    y = RR.folded_real(x, RR.round32(taps), M, D)
    ref = _per_call(y.real * y.real + y.imag * y.imag, counts)
    ref.setflags(write=False)
    free = _model(taps, M, D)
    for s, J in zip(ref, counts):
        free.update(s, J)
    thr = float(np.median(free.level))
    return taps, x, lens, counts, ref, (thr, 0.5 * thr)


_ROWS = {}


def _channelizer_sums(ctx, shape, dtype):
    """the real plain channelizer's float32 rows of the same calls on this device, squared and added in float64: [calls, K]"""
    if (shape, dtype) not in _ROWS:
        import libsdr_amd as sa
        taps, x, lens, counts, _, _ = _case(shape, dtype)
        node = sa.Channelizer(ctx, NP[dtype], shape[0], shape[1], taps, max_in=len(x), real=True)
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


def _node(ctx, shape, dtype, taps, max_in, grid=None):
    import libsdr_amd as sa
    M, D, n_taps = shape
    K, T = M // 2 + 1, RR.tile_times(M)
    node = sa.ChannelPower(ctx, NP[dtype], M, D, taps, alpha=ALPHA, max_in=max_in, real=True)
    assert node.kernel_names == ["chanpower_real_%s_kernel" % dtype, "chanpower_finish_kernel"]
    info = node.plan_info()
    assert info["tile_times"] == T and info["branch_taps"] == -(-n_taps // M) and info["lds_bytes"] == T * RR.image_stride(M) * 8
    tiles = -(-(-(-max_in // D)) // T)
    assert info["grid"] == (min(grid, tiles) if grid else tiles) and info["partial_bytes"] == info["grid"] * K * 8
    return node


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def _run(node, x, lens, model=None, thresholds=None):
    """every call's sums [calls, K]; with a model (the restatement's state step), check 3 after every call"""
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
        assert s.shape == (node.M // 2 + 1,) and s.dtype == np.float64
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


def _check(sums, rows, ref):
    for s, r in zip(sums, rows):
        assert np.all(np.abs(s - r) <= BOUND_ROWS * r), float((np.abs(s - r) / np.maximum(r, 1e-300)).max())
    err = float(np.abs(sums - ref).max() / ref.max())
    assert err <= BOUND, err
    return err


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_split_stream_against_the_restatement_and_the_channelizer(ctx, shape, dtype):
    import libsdr_amd as sa
    from redzone import RedZone
    M, D, n_taps = shape
    K = M // 2 + 1
    taps, x, lens, counts, ref, thr = _case(shape, dtype)
    rows = _channelizer_sums(ctx, shape, dtype)
    n, before = len(x), RedZone.calls
    node, model = _node(ctx, shape, dtype, taps, n), _model(taps, M, D)
    sums = _run(node, x, lens, model, thr)
    assert RedZone.calls - before == len([v for v in lens if v])
    assert sums.shape == ref.shape == (len(lens), K) and model.calls == len([c for c in counts if c])
    err = _check(sums, rows, ref)
    occ = node.occupied()
    print("chanreal power %s %s: max |sum - ref| / max ref = %.3g; %d of %d open" % (shape, dtype, err, len(occ), K))
    assert 0 < len(occ) < K and occ == sorted(occ) and 0 <= occ[0] and occ[-1] <= M // 2      # (the flags were worth comparing)
    s = node.get_state()
    assert s["consumed"] == n and s["calls"] == model.calls and not s["tail"][:, 1].any()
    level, flags = node.levels()
    # occupied() is what a real Channelizer's set_channels takes
    plain = sa.Channelizer(ctx, NP[dtype], M, D, taps, channels=occ, max_in=n, real=True)
    assert plain.selected == occ and plain.process(x).shape == (len(occ), n // D, 2)
    plain.close()
    # reset — the levels, flags and calls go, the thresholds stay — and the same stream again, bit for bit
    node.reset()
    level0, flags0 = node.levels()
    assert not level0.any() and not flags0.any() and node.occupied() == []
    assert node.get_state()["consumed"] == 0 and node.get_state()["calls"] == 0 and not node.get_state()["tail"].any()
    assert same(_run(node, x, lens), sums)
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
    sums = _run(node, x, lens, _model(taps, M, D), thr)
    _check(sums, rows, ref)
    node.close()
