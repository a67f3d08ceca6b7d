"""GPU parity of the interpolating resampler bank (include/sdrhip_resample.h): the device is held BIT FOR BIT to the numpy
restatement (tests/resample_restatement.py) — outputs, counts, mu and the line after every call — for the four element types and
for both tables (the reference's own from g21_psk31_table.bin, and sdrhip_design_inpol_taps), and to the fixtures cut from the
reference (tests/golden/g22_inpol_*). By its name the module runs in the red-zoned arena: device-pointer calls, row strides above
n and above the capacity, guard bands checked after every call; one test takes the host-pointer path. Float rows are compared
by their bit patterns except where both sides are NaN. The restatement's answers are computed once per case and shared."""
import functools

import numpy as np
import pytest

import resample_restatement as R

pytestmark = pytest.mark.gpu

T, G = 256, 4                                        # the plan every test asserts
EDGE_N = [0, 1, 7, T - 1, T, T + 1, 3 * T + 5, 300]
# per-row frac by the bank's rows (1, G, G + 1), together the whole set: the list's worst case (0.125), the pass-through row (1),
# the mu == 1 rows (0.5, 1.5, 2), tiles without an output (300), and frac = 2 alone against the odd call lengths
FRACS = {1: [2.0], G: [0.5, 1.378125, 1.5, 7.9], G + 1: [0.125, 1.0, 2.0, 45.35, 300.0]}
assert sorted(f for v in FRACS.values() for f in v) == sorted([0.125, 0.5, 1.0, 1.378125, 1.5, 2.0, 7.9, 45.35, 300.0, 2.0])


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _table(which):
    if which == "reference":
        return R.table()
    import libsdr_amd as sa
    return sa.design_inpol_taps()


def _signal(dtype, n, rows, seed, full_scale=False):
    """rows of noise [rows, n(, 2)] of the type's input; full_scale: the int16 types hold a stretch of 32767 and one of -32768"""
    rng = np.random.default_rng(seed)
    shape = (rows, n, 2) if R.IQ[dtype] else (rows, n)
    if R.IN_DT[dtype] == np.int16:
        x = rng.integers(-20000, 20000, shape).astype(np.int16)
        if full_scale:
            x[:, 40:90], x[:, 90:140] = 32767, -32768
        return x
    return (0.5 * rng.standard_normal(shape)).astype(np.float32)


def _node(ctx, dtype, fracs, table, max_in=1024):
    import libsdr_amd as sa
    node = sa.InpolSubSamplerBank(ctx, R.CODE[dtype], fracs, table=_table(table), max_in=max_in)
    assert node.plan_info() == {"tile_samples": T, "channels_per_group": G}
    assert node.kernel_names == ["resample_%s_kernel" % dtype]
    return node


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def _state(node):
    s = node.get_state()
    return s["mu"].view(np.uint32).copy(), s["line"]


def _run(node, x, lens, ops=None):
    """the calls of `lens` -> (output arrays per call and row, state after every call); ops: {call index: f(node)} run before it"""
    got, states, off = [], [], 0
    for b, n in enumerate(lens):
        if ops and b in ops:
            ops[b](node)
        got.append(node.process(x[:, off:off + n]))
        states.append(_state(node))
        off += n
    return got, states


def _run_ref(bank, x, lens, ops=None):
    got, states, off = [], [], 0
    for b, n in enumerate(lens):
        if ops and b in ops:
            ops[b](bank)
        got.append(bank.process(x[:, off:off + n]))
        states.append(bank.state())
        off += n
    return got, states


def _same_run(got, want, states, want_states):
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w)
        for r in range(len(g)):
            assert len(g[r]) == len(w[r]), ("count", b, r, len(g[r]), len(w[r]))
            assert same(g[r], w[r]), ("outputs", b, r)
        assert np.array_equal(states[b][0], want_states[b][0]), ("mu", b, states[b][0].tolist(), want_states[b][0].tolist())
        assert same(states[b][1], want_states[b][1]), ("line", b)


@functools.lru_cache(maxsize=None)
def _edge_ref(dtype, table, rows):
    x = _signal(dtype, sum(EDGE_N), rows, 11 + rows, full_scale=True)
    bank = R.Bank(dtype, FRACS[rows], _table(table))
    return x, _run_ref(bank, x, EDGE_N)


@pytest.mark.parametrize("rows", sorted(FRACS))
@pytest.mark.parametrize("table", ["reference", "designed"])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_edge_shapes_rows_and_per_row_frac(ctx, dtype, table, rows):
    from redzone import RedZone
    x, (want, want_states) = _edge_ref(dtype, table, rows)
    before = RedZone.calls
    node = _node(ctx, dtype, FRACS[rows], table)
    for n in EDGE_N:
        assert node.out_capacity(n) == R.out_capacity(FRACS[rows], n)
    got, states = _run(node, x, EDGE_N)
    _same_run(got, want, states, want_states)
    assert RedZone.calls - before == len([n for n in EDGE_N if n])
    if rows == 1:      # frac = 2: a call that ends on mu == 1 with no input left takes a last output at table row 128
        mu, last_rows = np.float32(0), []
        for n, g in zip(EDGE_N, got):
            _, taken, mu = R.chain(2.0, mu, n)
            assert len(g[0]) == len(taken)
            last_rows.append(int(taken[-1]) if len(taken) else None)
        assert last_rows == [None, 128, 0, 128, 128, 0, 128, 128]
    node.close()


@functools.lru_cache(maxsize=None)
def _ops_ref(dtype):
    lens = [300, 257, 255, 300]
    x = _signal(dtype, sum(lens), 3, 5)
    bank = R.Bank(dtype, [1.378125, 2.0, 0.5], R.table())
    ops = {1: lambda b: b.reset_row(1, 0.25), 2: lambda b: b.reset_row(2, 1.0), 3: lambda b: b.reset()}
    return lens, x, _run_ref(bank, x, lens, ops)


@pytest.mark.parametrize("dtype", ["cf32", "i16"])
def test_set_channel_and_reset_between_calls(ctx, dtype):
    """set_channel raises the bank's capacity (0.25 in place of 2) and makes a row a pass-through; the other rows stream on"""
    import libsdr_amd as sa
    lens, x, (want, want_states) = _ops_ref(dtype)
    node = _node(ctx, dtype, [1.378125, 2.0, 0.5], "reference")
    assert node.out_capacity(300) == 604
    got, states = _run(node, x, lens, {1: lambda n: n.set_channel(1, 0.25), 2: lambda n: n.set_channel(2, 1.0), 3: lambda n: n.reset()})
    _same_run(got, want, states, want_states)
    assert node.out_capacity(300) == 1206 and node.get_state()["frac"].tolist() == [np.float32(1.378125), 0.25, 1.0]
    for c, frac in ((3, 2.0), (-1, 2.0), (0, 0.1), (0, 5000.0), (0, float("nan"))):
        with pytest.raises(sa.SdrHipError) as e:
            node.set_channel(c, frac)
        assert e.value.code == sa.abi.E_INVALID
    mu, line = _state(node)
    assert np.array_equal(mu, states[-1][0]) and same(line, states[-1][1])   # (a refused call changes nothing)
    assert node.get_state()["frac"].tolist() == [np.float32(1.378125), 0.25, 1.0]
    node.close()


@functools.lru_cache(maxsize=None)
def _fixture_ref(dtype):
    """the fixtures of one type side by side in the restatement: names, per-call outputs, states"""
    names = [n for n in R.fixture_names() if R.manifest()[n]["dtype"] == dtype]
    fx = [R.fixture(n) for n in names]
    lens = fx[0][0]["lens"]
    bank = R.Bank(dtype, [m["frac"] for m, _, _, _ in fx], R.table())
    x = np.stack([x for _, x, _, _ in fx])
    return names, lens, x, _run_ref(bank, x, lens)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_fixtures_of_the_reference(ctx, dtype):
    """the four fixtures of a type as the four rows of one bank: the reference's outputs, counts, mu and line after every call"""
    names, lens, x, (want, want_states) = _fixture_ref(dtype)
    node = _node(ctx, dtype, [R.manifest()[n]["frac"] for n in names], "reference")
    got, states = _run(node, x, lens)
    _same_run(got, want, states, want_states)
    for k, name in enumerate(names):
        m, _, y, lines = R.fixture(name)
        assert [len(g[k]) for g in got] == m["counts"]
        assert same(np.concatenate([g[k] for g in got]), y), name
        assert [int(s[0][k]) for s in states] == m["mu_bits"], name
        assert same(np.stack([s[1][k] for s in states]), lines), name
    node.close()


def test_the_int16_accumulator_wraps(ctx):
    """a full-scale step at frac = 1.5: the int16 node wraps where the float node overshoots, as the restatement and the reference do"""
    x = np.zeros((1, 300), np.int16)
    x[:, 20:150], x[:, 150:] = 32767, -32768
    node, fl = _node(ctx, "i16", [1.5], "reference"), _node(ctx, "f32", [1.5], "reference")
    want = R.Bank("i16", [1.5], R.table()).process(x)[0]
    y, yf = node.process(x)[0], fl.process(x.astype(np.float32))[0]
    assert same(y, want)
    over = np.flatnonzero(yf > 32800)
    # wrapped: the float value less 65536, within the 8 truncations (below 1 each) of the accumulator's 8 conversions
    assert over.size and np.all(y[over] < 0) and np.all(np.abs(y[over].astype(np.float64) + 65536 - yf[over]) < 8.5), (y[over], yf[over])
    node.close()
    fl.close()


def test_an_inf_sample_in_a_float_row(ctx):
    """inf * 0 leaves NaNs in the outputs that hold the sample under a zero tap (frac = 0.5 takes rows 0 and 128; the rows that
    frac = 1.378125 takes have none, its outputs are infinite); compared except where both sides are NaN"""
    x = _signal("f32", 600, 2, 3)
    x[0, 100], x[1, 417] = np.inf, -np.inf
    lens = [300, 300]
    want, want_states = _run_ref(R.Bank("f32", [0.5, 1.378125], R.table()), x, lens)
    node = _node(ctx, "f32", [0.5, 1.378125], "reference")
    got, states = _run(node, x, lens)
    _same_run(got, want, states, want_states)
    assert np.isnan(got[0][0]).any() and np.isinf(got[0][0]).any() and np.isinf(got[1][1]).any()
    node.close()


@pytest.mark.hostptr_only
def test_host_pointer_calls_and_refusals(ctx):
    from libsdr_amd import abi
    rows = G + 1
    x, (want, want_states) = _edge_ref("cs16_cf32", "reference", rows)
    node = _node(ctx, "cs16_cf32", FRACS[rows], "reference")
    got, states = _run(node, x, EDGE_N)
    _same_run(got, want, states, want_states)
    cap = node.out_capacity(773)
    assert cap == 8 * 774 + 2 and node.out_capacity(0) == 0
    out, counts = np.full((rows, cap, 2), 7, np.float32), np.zeros(rows, np.uint32)
    p = lambda a: a.ctypes.data
    xs = np.ascontiguousarray(x[:, :773])
    assert node._c_process(node._h, p(xs), 773, 773, p(out), cap - 1, p(counts)) == abi.E_SIZE      # an out stride below the capacity
    assert node._c_process(node._h, p(xs), 773, 772, p(out), cap, p(counts)) == abi.E_SIZE
    assert node._c_process(node._h, p(xs), 1025, 1025, p(out), cap, p(counts)) == abi.E_SIZE        # above max_in
    din, dout, dcnt = ctx.malloc(xs.nbytes), ctx.malloc(out.nbytes), ctx.malloc(4 * rows)
    try:
        assert node._c_process_dev(node._h, din, 773, 773, dout, cap - 1, dcnt) == abi.E_SIZE
        assert node._c_process_dev(node._h, din, 773, 773, din, cap, dcnt) == abi.E_INVALID             # the output over the input
    finally:
        for q in (din, dout, dcnt):
            ctx.free(q)
    mu, line = _state(node)
    assert np.array_equal(mu, states[-1][0]) and same(line, states[-1][1]) and np.all(out == 7)
    # the elements of a row behind its count come back as zeros
    assert node._c_process(node._h, p(xs), 773, 773, p(out), cap, p(counts)) == abi.OK
    assert counts.max() <= cap and counts[1] == 773                                                 # (row 1 passes through)
    for r in range(rows):
        assert not out[r, counts[r]:].any(), r
    node.close()


# ---- behind a tuner bank, on its device rows ---------------------------------------------------------------------------------------

FS, D, ORDER, N = 64000.0, 8, 127, 4096
CARRIERS = [8000.0, -12000.0, 20000.0]
RATES = [1.378125, 0.5, 1.0]


@pytest.mark.hostptr_only
@pytest.mark.parametrize("mode", ["iq", "usb"])
def test_tuner_bank_rows_through_process_dev(ctx, mode):
    """a small tuner bank's DEVICE rows (SDRHIP_EPI_NONE cs16 -> CS16_CF32, USB int16 -> I16), strided as the tuner left them, go
    through process_dev; the result equals the restatement run on a host copy of the same rows"""
    import libsdr_amd as sa
    rng = np.random.default_rng(64)
    x = rng.integers(-12000, 12000, (2 * N, 2)).astype(np.int16)
    taps = np.stack([sa.design_iqbb_taps(f, 2000.0, FS, ORDER) for f in CARRIERS])
    inc, neg = [sa.design_freqshift_inc(f, FS) for f in CARRIERS], [f < 0 for f in CARRIERS]
    lut = sa.design_freqshift_lut_i16()
    C, iq = len(CARRIERS), mode == "iq"
    dtype = "cs16_cf32" if iq else "i16"
    epi = sa.EPI_NONE if iq else sa.EPI_USB
    rows_cap = N // D + 1
    stride = rows_cap + 24
    tuner = sa.TunerBankI16(ctx, taps, lut, inc, neg, D, max_in=N, epilogue=epi)
    tuner_host = sa.TunerBankI16(ctx, taps, lut, inc, neg, D, max_in=N, epilogue=epi)
    node = sa.InpolSubSamplerBank(ctx, R.CODE[dtype], RATES, max_in=rows_cap)         # the library's own table
    ref = R.Bank(dtype, RATES, sa.design_inpol_taps())
    cap = node.out_capacity(rows_cap)
    in_b, out_b = (4, 8) if iq else (2, 2)
    din, drows, dout, dcnt = ctx.malloc(N * 4), ctx.malloc(C * stride * in_b), ctx.malloc(C * cap * out_b), ctx.malloc(4 * C)
    try:
        for k in range(2):
            chunk = np.ascontiguousarray(x[k * N:(k + 1) * N])
            ctx.h2d(din, chunk)
            no = tuner.process_dev(din, N, drows, stride)
            assert 0 < no <= rows_cap
            node.process_dev(drows, no, stride, dout, cap, dcnt)     # the tuner's device rows, strided as it left them
            ctx.synchronize()
            out = np.zeros((C, cap, 2), np.float32) if iq else np.zeros((C, cap), np.int16)
            counts = np.zeros(C, np.uint32)
            ctx.d2h(out, dout)
            ctx.d2h(counts, dcnt)
            rows = tuner_host.process(chunk)                          # the same rows through the host
            assert rows.shape == ((C, no, 2) if iq else (C, no))
            want = ref.process(rows)
            for c in range(C):
                assert counts[c] == len(want[c]) and same(out[c, :counts[c]], want[c]), (k, c)
        mu, line = _state(node)
        assert np.array_equal(mu, ref.state()[0]) and same(line, ref.state()[1])
    finally:
        for q in (din, drows, dout, dcnt):
            ctx.free(q)
        for v in (tuner, tuner_host, node):
            v.close()
