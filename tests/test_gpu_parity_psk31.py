"""GPU parity of the BPSK31 bank (include/sdrhip_psk31.h): the device is held BIT FOR BIT to the numpy restatement with the
defined sincos (tests/psk31_restatement.py) — bits, counts and the state P, F, mu, omega, hist_idx, last after every call — and to
the fixtures cut from the reference (tests/golden/g21_psk31_*) in bits and counts. By its name the module runs in the red-zoned
arena: device-pointer calls, row strides above n and above the capacity, guard bands checked after every call; one test takes the
host-pointer path. The restatement's answers are computed once per signal and shared."""
import functools

import numpy as np
import pytest

import psk31_restatement as R

pytestmark = pytest.mark.gpu

DT = {"cs16": np.int16, "cf32": np.float32}
EDGE_N = [0, 1, 7, 255, 256, 257, 773, 300]    # tile = 256: tile - 1, tile, tile + 1, 3 tiles + 5
DFS = [0.1, 0.05, 0.2, 0.002, 0.1]             # one more row than a workgroup takes


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


def _signal(dtype, Fs, n, rows, seed):
    """rows PSK31 signals [rows, n, 2] with their own bits, carrier offsets and phases, light noise"""
    rng = np.random.default_rng(seed)
    x = np.zeros((rows, n, 2), DT[dtype])
    for r in range(rows):
        bits = rng.integers(0, 2, int(n / (Fs / 31.25)) + 3)
        z = R.modulate(Fs, bits, n, offset_hz=rng.uniform(-4, 4), phase=rng.uniform(0, 6), amp=0.5)
        z = z + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        v = np.stack([z.real, z.imag], axis=1)
        x[r] = np.round(v * 32767).astype(np.int16) if dtype == "cs16" else v.astype(np.float32)
    return x


def _state(node):
    s = node.get_state()
    v = lambda a: a.view(np.uint32).astype(np.int64)
    return np.stack([v(s["P"]), v(s["F"]), v(s["mu"]), v(s["omega"]), s["hist_idx"].astype(np.int64), s["last"].astype(np.int64)], axis=1)


def _run(node, x, lens, ops=None):
    """the calls of `lens` -> (bit arrays per call and row, state after every call); ops: {call index: f(node)} run before it"""
    got, states, off = [], [], 0
    for b, L in enumerate(lens):
        if ops and b in ops:
            ops[b](node)
        got.append(node.process(x[:, off:off + L]))
        states.append(_state(node))
        off += L
    return got, states


def _same(got, want, states, want_states, rows=None):
    for b, (g, w) in enumerate(zip(got, want)):
        for r in range(len(g)):
            assert np.array_equal(g[r], w[r]), ("bits", b, r, len(g[r]), len(w[r]))
        ws = want_states[b] if rows is None else want_states[b][:rows]
        assert np.array_equal(states[b], ws), ("state", b, states[b].tolist(), ws.tolist())


@functools.lru_cache(maxsize=None)
def _edge_ref(dtype, Fs):
    x = _signal(dtype, Fs, sum(EDGE_N), len(DFS), 7 + int(Fs))
    bank = R.Bank(Fs, DFS, R.table())
    return x, _run_ref(bank, x, EDGE_N)


def _run_ref(bank, x, lens, ops=None):
    got, states, off = [], [], 0
    for b, L in enumerate(lens):
        if ops and b in ops:
            ops[b](bank)
        got.append(bank.process(x[:, off:off + L]))
        states.append(bank.state())
        off += L
    return got, states


@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("dtype,Fs", [("cs16", 8000.0), ("cf32", 8000.0), ("cs16", 2000.0), ("cf32", 2000.0)])
def test_edge_shapes_rows_and_per_row_dF(ctx, dtype, Fs, rows):
    import libsdr_amd as sa
    from redzone import RedZone
    x, (want, want_states) = _edge_ref(dtype, Fs)
    before = RedZone.calls
    node = sa.BPSK31Bank(ctx, DT[dtype], Fs, DFS[:rows], table=R.table(), max_in=1024)
    assert node.plan_info() == {"tile_samples": 256, "channels_per_group": 4}
    assert node.kernel_names == ["psk31_%s_kernel" % dtype]
    got, states = _run(node, x[:rows], EDGE_N)
    _same(got, [w[:rows] for w in want], states, want_states, rows)
    assert RedZone.calls - before == len([n for n in EDGE_N if n])
    assert sum(len(g[0]) for g in got) >= 1   # (the signal is long enough for bits to come)
    node.close()


SPLITS = {"one": [2100], "ones": [1] * 40 + [2060], "33": [33] * 10 + [1770], "999": [999, 999, 102], "mixed": [1, 33, 999, 0, 1, 33, 999, 34]}


@functools.lru_cache(maxsize=None)
def _split_ref(dtype):
    x = _signal(dtype, 8000.0, 2100, 2, 99)
    bank = R.Bank(8000.0, 0.1, R.table(), rows=2)
    got, states = _run_ref(bank, x, [2100])
    return x, got[0], states[0]


@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("dtype", ["cs16", "cf32"])
def test_the_stream_does_not_depend_on_the_call_lengths(ctx, dtype, split):
    import libsdr_amd as sa
    x, want, want_state = _split_ref(dtype)
    node = sa.BPSK31(ctx, DT[dtype], 8000.0, 0.1, channels=2, table=R.table(), max_in=4096)
    got, states = _run(node, x, SPLITS[split])
    for r in range(2):
        assert np.array_equal(np.concatenate([g[r] for g in got]), want[r]), (split, r)
    assert np.array_equal(states[-1], want_state)
    node.close()


@functools.lru_cache(maxsize=None)
def _ops_ref():
    lens = [700, 500, 600, 300]
    x = _signal("cs16", 8000.0, sum(lens), 3, 5)
    bank = R.Bank(8000.0, [0.1, 0.1, 0.05], R.table())
    ops = {1: lambda b: b.reset_row(1, 0.02), 3: lambda b: b.reset()}
    return lens, x, _run_ref(bank, x, lens, ops)


def test_set_channel_and_reset_between_calls(ctx):
    import libsdr_amd as sa
    lens, x, (want, want_states) = _ops_ref()
    node = sa.BPSK31Bank(ctx, np.int16, 8000.0, [0.1, 0.1, 0.05], table=R.table(), max_in=1024)
    got, states = _run(node, x, lens, {1: lambda n: n.set_channel(1, 0.02), 3: lambda n: n.reset()})
    _same(got, want, states, want_states)
    with pytest.raises(sa.SdrHipError):
        node.set_channel(3, 0.1)
    with pytest.raises(sa.SdrHipError):
        node.set_channel(0, 0.0)
    assert np.array_equal(_state(node), states[-1])   # (a refused call changes nothing)
    node.close()


def test_set_channel_refuses_a_row_outside_the_bank(ctx):
    """The smallest bank that has two rows to tell apart: 2 rows, max_in 64, one call each. Rows -1 and 2 are refused with the
    range in the message and nothing changed; a set_channel that succeeds leaves row 0 as it is in a bank never touched."""
    import libsdr_amd as sa
    n, dF = 64, [0.1, 0.05]
    x = _signal("cs16", 8000.0, 2 * n, 2, 17)
    ref = R.Bank(8000.0, dF, R.table())
    node, twin = (sa.BPSK31Bank(ctx, np.int16, 8000.0, dF, table=R.table(), max_in=n) for _ in range(2))
    for c in (-1, 2):
        with pytest.raises(sa.SdrHipError) as e:
            node.set_channel(c, 0.02)
        assert e.value.code == sa.abi.E_INVALID and "outside [0,2)" in str(e.value), (c, str(e.value))
    ops = {1: lambda b: b.set_channel(1, 0.02)}
    got, states = _run(node, x, [n, n], ops)
    und, und_states = _run(twin, x, [n, n])
    want, want_states = _run_ref(ref, x, [n, n], {1: lambda b: b.reset_row(1, 0.02)})
    _same(got, want, states, want_states)
    assert np.array_equal(states[0], und_states[0])                                           # the refused calls changed nothing
    assert np.array_equal(got[1][0], und[1][0]) and np.array_equal(states[1][0], und_states[1][0])   # row 0 streamed on
    assert not np.array_equal(states[1][1], und_states[1][1])                                 # and row 1 is a fresh node
    node.close()
    twin.close()


@functools.lru_cache(maxsize=None)
def _fixture_ref(Fs):
    """the fixtures of one sample rate side by side in the restatement (defined sincos): names, per-call bits, states"""
    names = [n for n in R.fixture_names() if R.manifest()[n]["Fs"] == Fs]
    fx = [R.fixture(n) for n in names]
    lens = fx[0][0]["lens"]
    assert all(m["lens"] == lens for m, _, _ in fx)
    bank = R.Bank(Fs, [m["dF"] for m, _, _ in fx], R.table())
    x = np.stack([x.astype(np.float32) for _, x, _ in fx])
    return names, lens, _run_ref(bank, x, lens)


@pytest.mark.parametrize("name", R.fixture_names())
def test_fixtures_bits_of_the_reference_and_state_of_the_restatement(ctx, name):
    import libsdr_amd as sa
    m, x, bits = R.fixture(name)
    names, lens, (want, want_states) = _fixture_ref(m["Fs"])
    k = names.index(name)
    node = sa.BPSK31(ctx, DT[m["dtype"]], m["Fs"], m["dF"], table=R.table(), max_in=8000)
    got, states = _run(node, x[None], lens)
    assert [len(g[0]) for g in got] == m["counts"]
    assert np.array_equal(np.concatenate([g[0] for g in got]), bits)
    for b in range(len(lens)):
        assert np.array_equal(got[b][0], want[b][k]), (name, b)
        assert np.array_equal(states[b][0], want_states[b][k]), (name, b, states[b][0].tolist(), want_states[b][k].tolist())
    node.close()


@pytest.mark.hostptr_only
def test_host_pointer_calls_and_refusals(ctx):
    import libsdr_amd as sa
    from libsdr_amd import abi
    x, (want, want_states) = _edge_ref("cf32", 8000.0)
    node = sa.BPSK31Bank(ctx, np.float32, 8000.0, DFS, table=R.table(), max_in=1024)
    got, states = _run(node, x, EDGE_N)
    _same(got, want, states, want_states)
    cap = node.out_capacity(773)
    assert cap == R.out_capacity(8000.0, 773) and node.out_capacity(0) == 0
    bits, counts = np.zeros((5, cap), np.uint8), np.zeros(5, np.uint32)
    p = lambda a: a.ctypes.data
    assert node._c_process(node._h, p(x), 773, 773, p(bits), cap - 1, p(counts)) == abi.E_SIZE      # an out stride below the capacity
    assert node._c_process(node._h, p(x), 773, 772, p(bits), cap, p(counts)) == abi.E_SIZE
    assert node._c_process(node._h, p(x), 1025, 1025, p(bits), cap, p(counts)) == abi.E_SIZE        # above max_in
    assert np.array_equal(_state(node), states[-1])
    node.close()


def test_the_designed_table_decodes_a_clean_signal(ctx):
    """the library's own table (the default): the text sent comes back, and the device equals the restatement with that table"""
    import libsdr_amd as sa
    text = "cq psk"
    tx = R.varicode_bits(text, idle=20)
    n = int((len(tx) + 6) * 256)
    z = R.modulate(8000.0, tx, n, offset_hz=2.0, phase=0.7)
    x = np.stack([z.real, z.imag], axis=1).astype(np.float32)[None]
    node = sa.BPSK31(ctx, np.float32, 8000.0, max_in=8192)
    bank = R.Bank(8000.0, 0.1, sa.design_inpol_taps(), rows=1)
    vc, text_dev, text_ref = sa.Varicode(1), "", ""
    vr = sa.Varicode(1)
    for off in range(0, n, 8192):
        g, w = node.process(x[:, off:off + 8192]), bank.process(x[:, off:off + 8192])
        assert np.array_equal(g[0], w[0])
        text_dev += vc.feed(g)[0]
        text_ref += vr.feed(w)[0]
    assert np.array_equal(_state(node), bank.state())
    assert text_dev == text_ref and text in text_dev, (text_dev, text_ref)
    node.close()
