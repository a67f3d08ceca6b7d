"""GPU parity of the audio channelizer (include/sdrhip_chanaudio.h), every case BIT FOR BIT. The reference is the existing
Channelizer's float32 rows of the same input cut into the same calls, converted by the header's numpy rule and demodulated by
tests/chanaudio_restatement.py (which tests/test_chanaudio_restatement.py holds to the oracle); FM rows are also checked against
sa.Demod (FM, cs16, inplace_fm0 = 1) fed the converted rows call by call. After every call get_state's `last` equals the
restatement's. By its name the module runs in the red-zoned arena (device-pointer calls, strided rows, guard bands checked after
every call); one test takes the host-pointer path.

Shapes are the smallest at which each mechanism can fail: M = 2 has T = 256 output times per tile, so the FM halo runs across
several tiles of one short call; (12, 5, 30) divides nothing and is mixed radix; (64, 32, 512) carries the selection and setter
cases; 1000 is 5^3 * 8; at M = 4096 a tile holds T = 2 times, the halo is half a tile, and LDS is above 64 KiB. A stream is made
of calls that emit 0, 1, 2, T, T + 1 and 2 T + 1 outputs, and is cut two more ways."""
import functools

import numpy as np
import pytest

import chanaudio_restatement as A

pytestmark = pytest.mark.gpu

FM, AM, USB = A.FM, A.AM, A.USB
# (M, D, n_taps)
SHAPES = [(2, 1, 1), (2, 1, 128), (12, 5, 30), (64, 32, 512), (1000, 500, 3000), (4096, 4096, 8192)]
DTYPES = ["cs16", "cf32"]


def tile_times(M):
    """the channelizer's rule"""
    return min(256, (4096 if M <= 512 else 8192) // M)


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


def _taps(M, n_taps):
    t = np.arange(n_taps) - (n_taps - 1) / 2
    return np.sinc(t / M) / M * np.hanning(n_taps + 2)[1:-1]


def _signal(dtype, n, seed):
    rng = np.random.default_rng(seed)
    if dtype == "cs16":
        return rng.integers(-20000, 20000, (n, 2)).astype(np.int16)
    return (0.5 * rng.standard_normal((n, 2))).astype(np.float32)


def _splits(M, D):
    """three cuts of one stream: calls that emit 0, 1, 2, T, T + 1, 2 T + 1 and 1 outputs (behind D - 1 samples a call of c D
    samples emits c); the same cut elsewhere, with an empty call and one sample alone; one call"""
    T = tile_times(M)
    a = [D - 1, D, 2 * D, T * D, (T + 1) * D, (2 * T + 1) * D, 1]
    n = sum(a)
    b = [3 * D + 1, 0, 1, (T + 2) * D, 0]
    b.append(n - sum(b))
    assert b[-1] > 0
    return [a, b, [n]]


def _modes(M):
    return [(FM, AM, USB)[k % 3] for k in range(M)]


def _gains(M, dtype):
    """around the level that brings a channel's output to some thousands; channel 1 (M >= 12) saturates"""
    g = np.array([0.75 + 0.5 * (k % 5) for k in range(M)], np.float32) * (np.float32(1) if dtype == "cs16" else np.float32(20000))
    if M >= 12:
        g[1] *= 64
        g[3] *= 64
    return g


def _dt(dtype):
    return np.int16 if dtype == "cs16" else np.float32


@functools.lru_cache(maxsize=None)
def _stream(shape, dtype):
    M, D, n_taps = shape
    n = sum(_splits(M, D)[0])
    x = _signal(dtype, n, 31 * M + D + n_taps)
    x.setflags(write=False)
    return _taps(M, n_taps), x


def _pair(ctx, shape, dtype, max_in, modes=None, gains=None, channels=None):
    """(the audio node, the plain channelizer that makes its reference rows), the same selection on both"""
    import libsdr_amd as sa
    M, D, n_taps = shape
    taps, _ = _stream(shape, dtype)
    node = sa.AudioChannelizer(ctx, _dt(dtype), M, D, taps, modes=modes, gains=gains, channels=channels, max_in=max_in)
    plain = sa.Channelizer(ctx, _dt(dtype), M, D, taps, channels=channels, max_in=max_in)
    assert node.kernel_names == ["chanaudio_%s_kernel" % dtype]
    info = node.plan_info()
    T = tile_times(M)
    assert info["tile_times"] == T and info["branch_taps"] == -(-n_taps // M) and info["rows"] == node.channels
    assert info["lds_bytes"] == (T + 1) * (M + 1) * 8
    return node, plain


def _run(node, plain, ref, x, lens, rows=None, demods=None):
    """the calls of one cut -> (the node's parts, the reference's); `last` is compared after every call. demods: {row: sa.Demod}
    for FM rows, fed the converted rows."""
    got, want, off = [], [], 0
    for n in lens:
        assert node.out_count(n) == (off + n) // node.D - off // node.D
        part = x[off:off + n]
        y = node.process(part)
        y32 = plain.process(part)
        w = ref.process(y32, rows)
        assert y.dtype == np.int16 and y.shape == w.shape, (y.shape, w.shape)
        assert np.array_equal(y, w), (off, n, np.argwhere(y != w)[:5].tolist())
        idx = range(len(ref.modes)) if rows is None else rows
        assert node.get_state()["last"].tolist() == [ref.last[r] for r in idx], (off, n)
        for i, d in (demods or {}).items():
            if y.shape[1]:
                q = A.convert(y32[i], ref.gains[idx[i]])
                assert np.array_equal(d.process(q[None])[0], y[i]), (off, n, i)
        got.append(y)
        want.append(w)
        off += n
    assert node.get_state()["consumed"] == off == plain.get_state()["consumed"]
    return np.concatenate(got, axis=1), np.concatenate(want, axis=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_three_cuts_of_a_stream_against_the_reference(ctx, shape, dtype):
    import libsdr_amd as sa
    M, D, n_taps = shape
    _, x = _stream(shape, dtype)
    modes, gains = _modes(M), _gains(M, dtype)
    node, plain = _pair(ctx, shape, dtype, len(x), modes, gains)
    assert node.get_modes() == modes and np.array_equal(node.get_gains(), gains)
    fm_rows = [0, 3] if M >= 12 else [0]
    outs = []
    for lens in _splits(M, D):
        ref = A.Rows(modes, gains)
        demods = {i: sa.Demod(ctx, sa.EPI_FM, channels=1, max_in=len(x), inplace_fm0=True) for i in fm_rows}
        y, w = _run(node, plain, ref, x, lens, demods=demods)
        outs.append(y)
        for d in demods.values():
            d.close()
        node.reset()
        plain.reset()
        assert not node.get_state()["last"].any() and node.get_state()["consumed"] == 0
    n_out = len(x) // D
    assert outs[0].shape == (M, n_out) and n_out == 4 * tile_times(M) + 6
    # AM and USB rows do not depend on the cut (FM rows do, by the per-call convention: each cut has its own reference above)
    am_usb = [k for k in range(M) if modes[k] != FM]
    for y in outs[:2]:
        assert np.array_equal(y[am_usb], outs[2][am_usb])
    if M in (12, 64):      # the saturating gains reach both clamps
        q = A.convert(plain.process(x)[3], gains[3])
        assert q.max() == 32767 and q.min() == -32768
    node.close()
    plain.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_selected_rows_equal_the_rows_of_the_full_run(ctx, dtype):
    shape = (64, 32, 512)
    M, D, _ = shape
    _, x = _stream(shape, dtype)
    modes, gains, lens = _modes(M), _gains(M, dtype), _splits(M, D)[1]
    node, plain = _pair(ctx, shape, dtype, len(x), modes, gains)
    full, _ = _run(node, plain, A.Rows(modes, gains), x, lens)
    for sel in ([40, 3, 17], [5, 62, 4]):          # scrambled: AM FM USB — and one without an FM row: no halo image
        node.reset()
        plain.reset()
        node.set_channels(sel)
        plain.set_channels(sel)
        info = node.plan_info()
        assert info["rows"] == 3 and info["fm_rows"] == [modes[k] for k in sel].count(FM)
        assert node.get_modes() == [modes[k] for k in sel] and np.array_equal(node.get_gains(), gains[sel])
        y, _ = _run(node, plain, A.Rows(modes, gains), x, lens, rows=sel)
        assert np.array_equal(y, full[sel])
    node.close()
    plain.close()


def test_saturation_inf_and_nan(ctx):
    shape, dtype = (12, 5, 30), "cf32"
    M, D, _ = shape
    x = np.array(_stream(shape, dtype)[1])
    x[100, 0], x[101, 1], x[400, 0] = np.inf, np.nan, -np.inf
    modes, gains = _modes(M), np.full(M, 3e4, np.float32)
    gains[6:] = [1e30, -1e30, 1e38, 0.0, -0.0, 1e-30]
    node, plain = _pair(ctx, shape, dtype, len(x), modes, gains)
    y, _ = _run(node, plain, A.Rows(modes, gains), x, _splits(M, D)[0])
    plain.reset()
    y32 = plain.process(x)
    bad = ~np.isfinite(y32).all(axis=(0, 2))                 # the output times an inf or the NaN reaches
    assert bad.any() and not bad.all() and np.isnan(y32).any()
    q = A.convert(y32, gains[:, None, None])
    assert q.max() == 32767 and q.min() == -32768 and not q[np.isnan(y32)].any()
    assert not y[9].any() and not y[10].any()                # gains 0 and -0: zeros also where the spectrum is not finite
    assert y[:6, bad].any()
    node.close()
    plain.close()


def test_setters_between_calls(ctx):
    import libsdr_amd as sa
    from libsdr_amd import abi
    shape, dtype = (64, 32, 512), "cs16"
    M, D, _ = shape
    _, x = _stream(shape, dtype)
    modes, gains = _modes(M), _gains(M, dtype)
    node, plain = _pair(ctx, shape, dtype, len(x), modes, gains)
    ref = A.Rows(modes, gains)
    cuts = [0, 7 * D + 3, 20 * D, 20 * D + 1, 90 * D + 9, 150 * D, 200 * D + 5, len(x)]
    seg = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    sel = list(range(M))

    def step(part, rows=None):
        y, w = node.process(part), ref.process(plain.process(part), rows)
        assert np.array_equal(y, w), np.argwhere(y != w)[:5].tolist()
        assert node.get_state()["last"].tolist() == [ref.last[r] for r in (sel if rows is None else rows)]
        return y

    step(seg[0])
    before = node.get_state()["last"].copy()
    assert before[0] != 0 and before[3] != 0
    # FM -> FM restarts row 0 from last = 0, an AM row becomes FM, an FM row USB; a gain changes and keeps last; the others go on
    for row, mode in ((0, FM), (1, FM), (6, USB)):
        node.set_mode(row, mode)
        ref.set_mode(row, mode)
    node.set_gain(3, 2.5)
    ref.set_gain(3, 2.5)
    after = node.get_state()["last"]
    assert after[0] == 0 and after[1] == 0 and after[6] == 0 and after[3] == before[3] and np.array_equal(after[7:], before[7:])
    assert node.get_modes()[:7] == [FM, FM, USB, FM, AM, USB, USB] and node.get_gains()[3] == np.float32(2.5)
    step(seg[1])
    step(seg[2])                                    # one sample, no output
    # a subset and back: the channels keep their modes, gains and last, deselected ones move on as well
    sub = [9, 0, 33, 6]
    node.set_channels(sub)
    assert node.plan_info()["fm_rows"] == 3 and node.get_modes() == [FM, FM, FM, USB]
    y = node.process(seg[3])
    w_all = ref.process(plain.process(seg[3]))      # (the restatement carries every channel, as the node does)
    assert np.array_equal(y, w_all[sub]) and node.get_state()["last"].tolist() == [ref.last[r] for r in sub]
    node.set_mode(2, AM)                            # row 2 of the selection is channel 33
    ref.set_mode(33, AM)
    node.set_channels(None)
    assert node.get_modes()[33] == AM and node.get_state()["last"].tolist() == ref.last
    step(seg[4])
    # refusals change nothing
    state = node.get_state()
    for call, code in ((lambda: node.set_mode(0, abi.EPI_NONE), abi.E_UNSUPPORTED), (lambda: node.set_mode(0, 4), abi.E_INVALID),
                       (lambda: node.set_mode(M, FM), abi.E_INVALID), (lambda: node.set_mode(-1, FM), abi.E_INVALID),
                       (lambda: node.set_gain(M, 1.0), abi.E_INVALID), (lambda: node.set_gain(0, float("nan")), abi.E_INVALID),
                       (lambda: node.set_gain(0, float("inf")), abi.E_INVALID), (lambda: node.set_channels([1, 1]), abi.E_INVALID)):
        with pytest.raises(sa.SdrHipError) as e:
            call()
        assert e.value.code == code
    assert node.get_state()["last"].tolist() == state["last"].tolist() and node.get_modes() == ref.modes
    step(seg[5])
    # reset: t = 0 and every last 0, the modes and gains stay
    node.reset()
    plain.reset()
    ref.reset()
    assert not node.get_state()["last"].any() and node.get_modes() == ref.modes
    step(seg[6])
    node.close()
    plain.close()


@pytest.mark.hostptr_only
def test_host_pointer_staging_grows_with_the_selection(ctx):
    """The first host-pointer call stages two rows (reordered: get_modes and get_gains follow the rows); set_channels then
    raises the rows to M, and the staged output has to regrow. Calls of 1, 7 and 23 samples, one of T + 1 outputs, the rest."""
    shape, dtype = (6, 4, 14), "cs16"
    M, D, _ = shape
    _, x = _stream(shape, dtype)
    modes, gains = _modes(M), _gains(M, dtype)
    lens = [1, 7, 23, (tile_times(M) + 1) * D]
    lens.append(len(x) - sum(lens))
    sel = [3, 0]                                             # both FM
    node, plain = _pair(ctx, shape, dtype, len(x), modes, gains, channels=sel)
    assert node.get_modes() == [modes[k] for k in sel] and np.array_equal(node.get_gains(), gains[sel])
    ref = A.Rows(modes, gains)
    _run(node, plain, ref, x, lens, rows=sel)
    before = node.get_state()["last"].tolist()
    assert before[0] != 0 and before[1] != 0
    node.set_mode(1, FM)                                    # row 1 is channel 0: its `last` starts from 0, channel 3's stays
    ref.set_mode(0, FM)
    assert node.get_state()["last"].tolist() == [ref.last[3], ref.last[0]] == [before[0], 0]
    part = x[:23]
    assert np.array_equal(node.process(part), ref.process(plain.process(part), sel))
    for v in (node, plain):
        v.reset()
        v.set_channels(None)
    assert node.plan_info()["rows"] == M and node.get_modes() == modes and np.array_equal(node.get_gains(), gains)
    y, w = _run(node, plain, A.Rows(modes, gains), x, lens)
    assert y.shape == (M, len(x) // D)
    for v in (node, plain):
        v.reset()
    _run(node, plain, A.Rows(modes, gains), x, [len(x)])    # one call of max_in samples: the largest staged output
    # set_taps in mid-stream: the node and the plain channelizer take the new prototype; one that is not finite changes nothing
    import libsdr_amd as sa
    other = _taps(M, 14)[::-1] * np.linspace(0.5, 1.5, 14)
    bad = other.copy()
    bad[3] = np.inf
    ref = A.Rows(modes, gains)
    for v in (node, plain):
        v.reset()
    _run(node, plain, ref, x, [7, 23])
    for v in (node, plain):
        v.set_taps(other)
    with pytest.raises(sa.SdrHipError) as e:
        node.set_taps(bad)
    assert e.value.code == sa.abi.E_INVALID
    part = x[30:30 + (tile_times(M) + 1) * D]
    y, y32 = node.process(part), plain.process(part)
    assert np.array_equal(y, ref.process(y32)) and node.get_state()["last"].tolist() == ref.last
    node.close()
    plain.close()


@pytest.mark.hostptr_only
def test_host_pointer_calls_and_refusals(ctx):
    from libsdr_amd import abi
    shape, dtype = (12, 5, 30), "cs16"
    M, D, _ = shape
    _, x = _stream(shape, dtype)
    modes, gains = _modes(M), _gains(M, dtype)
    node, plain = _pair(ctx, shape, dtype, len(x), modes, gains)
    _run(node, plain, A.Rows(modes, gains), x, _splits(M, D)[1])
    node.reset()
    plain.reset()
    node.set_channels([7, 2, 0])
    plain.set_channels([7, 2, 0])
    _run(node, plain, A.Rows(modes, gains), x, _splits(M, D)[0], rows=[7, 2, 0])     # (the staged rows follow the selection)
    state = node.get_state()
    no = node.out_count(60)
    out = np.full((3, no), 7, np.int16)
    p = lambda a: a.ctypes.data
    xs = np.ascontiguousarray(x[:60])
    assert node._c_process(node._h, p(xs), 60, p(out), no - 1, None) == abi.E_SIZE        # an out stride below the count
    assert node._c_process(node._h, p(xs), len(x) + 1, p(out), no, None) == abi.E_SIZE    # above max_in
    assert node._c_process(node._h, None, 60, p(out), no, None) == abi.E_INVALID
    din, dout = ctx.malloc(xs.nbytes), ctx.malloc(out.nbytes)
    try:
        assert node._c_process_dev(node._h, din, 60, dout, no - 1, None) == abi.E_SIZE
        assert node._c_process_dev(node._h, din, 60, din, no, None) == abi.E_INVALID      # the output over the input
    finally:
        ctx.free(din)
        ctx.free(dout)
    last = np.zeros(2, np.intc)
    assert node._c_get_state(node._h, None, None, 0, last.ctypes.data_as(node._c_get_state.argtypes[4]), 2) == abi.E_SIZE
    after = node.get_state()
    assert after["consumed"] == state["consumed"] and after["last"].tolist() == state["last"].tolist() and np.all(out == 7)
    node.close()
    plain.close()
