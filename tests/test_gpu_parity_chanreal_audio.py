"""GPU parity of the audio channelizer for a real-sampled row (include/sdrhip_chanreal.h, AudioChannelizer(real=True)), every
case BIT FOR BIT. The reference is the real plain Channelizer's float32 rows of the same input cut into the same calls, converted
by sdrhip_chanaudio.h's numpy rule and demodulated by tests/chanaudio_restatement.py; after every call get_state's `last` equals
the restatement's. Modes are FM / AM / USB mixed over the K = M / 2 + 1 channels, channels 0 and H among them (FM and, at the
shapes here, AM or USB). By its name the module runs in the red-zoned arena.

Shapes: (8, 8, 24) has T = 256 output times per tile, so the FM halo runs across the tiles of short calls; (64, 32, 64) carries the
selection and the setters; at (1000, 500, 3000) a tile holds 16 times. A stream is made of calls that emit 0, 1, 2, T, T + 1 and
2 T + 1 outputs, and is cut two more ways."""
import functools

import numpy as np
import pytest

import chanaudio_restatement as A
import chanreal_restatement as RR

pytestmark = pytest.mark.gpu

FM, AM, USB = A.FM, A.AM, A.USB
SHAPES = [(8, 8, 24), (64, 32, 64), (1000, 500, 3000)]
DTYPES = ["s16", "f32"]
NP = {"s16": np.int16, "f32": np.float32}


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


def _splits(M, D):
    """three cuts of one stream: calls that emit 0, 1, 2, T, T + 1, 2 T + 1 and 1 outputs; the same cut elsewhere, with an empty
    call and one sample alone; one call"""
    T = RR.tile_times(M)
    a = [D - 1, D, 2 * D, T * D, (T + 1) * D, (2 * T + 1) * D, 1]
    n = sum(a)
    b = [3 * D + 1, 0, 1, (T + 2) * D, 0]
    b.append(n - sum(b))
    assert b[-1] > 0
    return [a, b, [n]]


def _modes(K):
    return [(FM, AM, USB)[k % 3] for k in range(K)]


def _gains(K, dtype):
    """around the level that brings a channel's output to some thousands; channels 1 and 3 saturate"""
    g = np.array([0.75 + 0.5 * (k % 5) for k in range(K)], np.float32) * (np.float32(1) if dtype == "s16" else np.float32(20000))
    g[1] *= 64
    g[3] *= 64
    return g


@functools.lru_cache(maxsize=None)
def _stream(shape, dtype):
    M, D, n_taps = shape
    n = sum(_splits(M, D)[0])
    rng = np.random.default_rng(31 * M + D + n_taps)
    x = rng.integers(-20000, 20000, n).astype(np.int16) if dtype == "s16" else (0.5 * rng.standard_normal(n)).astype(np.float32)
    x.setflags(write=False)
    return RR.prototype(M, n_taps), x


def _pair(ctx, shape, dtype, max_in, modes=None, gains=None, channels=None):
    """(the audio node, the real plain channelizer that makes its reference rows), the same selection on both"""
    import libsdr_amd as sa
    M, D, n_taps = shape
    taps, _ = _stream(shape, dtype)
    node = sa.AudioChannelizer(ctx, NP[dtype], M, D, taps, modes=modes, gains=gains, channels=channels, max_in=max_in, real=True)
    plain = sa.Channelizer(ctx, NP[dtype], M, D, taps, channels=channels, max_in=max_in, real=True)
    assert node.kernel_names == ["chanaudio_real_%s_kernel" % dtype]
    info = node.plan_info()
    T = RR.tile_times(M)
    assert info["tile_times"] == T and info["branch_taps"] == -(-n_taps // M) and info["rows"] == node.channels
    assert info["lds_bytes"] == (T + 1) * RR.image_stride(M) * 8
    return node, plain


def _run(node, plain, ref, x, lens, rows=None):
    """the calls of one cut -> the node's rows; every call is compared, and `last` after it"""
    got, off = [], 0
    for n in lens:
        assert node.out_count(n) == (off + n) // node.D - off // node.D
        part = x[off:off + n]
        y = node.process(part)
        w = ref.process(plain.process(part), rows)
        assert y.dtype == np.int16 and y.shape == w.shape, (y.shape, w.shape)
        assert np.array_equal(y, w), (off, n, np.argwhere(y != w)[:5].tolist())
        idx = range(len(ref.modes)) if rows is None else rows
        assert node.get_state()["last"].tolist() == [ref.last[r] for r in idx], (off, n)
        got.append(y)
        off += n
    assert node.get_state()["consumed"] == off == plain.get_state()["consumed"]
    return np.concatenate(got, axis=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_three_cuts_of_a_stream_against_the_reference(ctx, shape, dtype):
    M, D, n_taps = shape
    K = M // 2 + 1
    _, x = _stream(shape, dtype)
    modes, gains = _modes(K), _gains(K, dtype)
    assert modes[0] == FM and modes[K - 1] in (AM, USB)
    node, plain = _pair(ctx, shape, dtype, len(x), modes, gains)
    assert node.channels == K and node.get_modes() == modes and np.array_equal(node.get_gains(), gains)
    outs = []
    for lens in _splits(M, D):
        outs.append(_run(node, plain, A.Rows(modes, gains), x, lens))
        node.reset()
        plain.reset()
        assert not node.get_state()["last"].any() and node.get_state()["consumed"] == 0
    n_out = len(x) // D
    assert outs[0].shape == (K, n_out) and n_out == 4 * RR.tile_times(M) + 6
    # AM and USB rows do not depend on the cut (FM rows do, by the per-call convention: each cut has its own reference above)
    am_usb = [k for k in range(K) if modes[k] != FM]
    for y in outs[:2]:
        assert np.array_equal(y[am_usb], outs[2][am_usb])
    # channel H as FM too: the modes the other way round
    rev = modes[::-1]
    node2, plain2 = _pair(ctx, shape, dtype, len(x), rev, gains)
    _run(node2, plain2, A.Rows(rev, gains), x, _splits(M, D)[1])
    node2.close()
    plain2.close()
    # the saturating gains reach both clamps
    q = A.convert(plain.process(x)[3], gains[3])
    assert q.max() == 32767 and q.min() == -32768
    node.close()
    plain.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_selection_and_setters_between_calls(ctx, dtype):
    import libsdr_amd as sa
    from libsdr_amd import abi
    shape = (64, 32, 64)
    M, D, _ = shape
    K = M // 2 + 1
    _, x = _stream(shape, dtype)
    modes, gains, lens = _modes(K), _gains(K, dtype), _splits(M, D)[1]
    node, plain = _pair(ctx, shape, dtype, len(x), modes, gains)
    full = _run(node, plain, A.Rows(modes, gains), x, lens)
    for sel in ([32, 3, 0, 17], [5, 32, 4]):          # with 0 and H, not ascending — and one without an FM row: no halo image
        node.reset()
        plain.reset()
        node.set_channels(sel)
        plain.set_channels(sel)
        info = node.plan_info()
        assert info["rows"] == len(sel) and info["fm_rows"] == [modes[k] for k in sel].count(FM)
        assert node.get_modes() == [modes[k] for k in sel] and np.array_equal(node.get_gains(), gains[sel])
        assert np.array_equal(_run(node, plain, A.Rows(modes, gains), x, lens, rows=sel), full[sel])
    node.set_channels(None)
    plain.set_channels(None)
    node.reset()
    plain.reset()
    # setters between calls: FM -> FM restarts from last = 0, channel H becomes FM, channel 0 USB; a gain changes and keeps last
    ref = A.Rows(modes, gains)
    cuts = [0, 7 * D + 3, 20 * D, 20 * D + 1, len(x)]
    seg = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]

    def step(part):
        y, w = node.process(part), ref.process(plain.process(part), None)
        assert np.array_equal(y, w), np.argwhere(y != w)[:5].tolist()
        assert node.get_state()["last"].tolist() == list(ref.last)

    step(seg[0])
    before = node.get_state()["last"].copy()
    assert before[3] != 0
    for row, mode in ((3, FM), (K - 1, FM), (0, USB)):
        node.set_mode(row, mode)
        ref.set_mode(row, mode)
    node.set_gain(6, 2.5)
    ref.set_gain(6, 2.5)
    after = node.get_state()["last"]
    assert after[3] == 0 and after[K - 1] == 0 and after[0] == 0 and after[6] == before[6]
    assert node.get_modes()[K - 1] == FM and node.get_modes()[0] == USB and node.get_gains()[6] == np.float32(2.5)
    step(seg[1])
    step(seg[2])                                    # one sample, no output
    for call, code in ((lambda: node.set_mode(0, abi.EPI_NONE), abi.E_UNSUPPORTED), (lambda: node.set_mode(K, FM), abi.E_INVALID),
                       (lambda: node.set_gain(K, 1.0), abi.E_INVALID), (lambda: node.set_channels([K]), abi.E_INVALID),
                       (lambda: node.set_channels(list(range(K)) + [0]), abi.E_INVALID)):
        with pytest.raises(sa.SdrHipError) as e:
            call()
        assert e.value.code == code
    step(seg[3])
    node.close()
    plain.close()
