"""GPU parity of the AGC bank (sdrhip_agc_*, include/sdrhip_agc.h) with the g20_agc_* fixtures of the compiled reference and with
the restatement (tests/agc_restatement.py, held against the same fixtures by tests/test_agc_restatement.py). Every comparison
is bit for bit; there is no tolerance. Float rows are compared bit for bit except where BOTH sides are NaN (x86's inf * 0 is the
negative quiet NaN, the GPU's the positive one), and every case outside the silence ones asserts that its expectation holds no
NaN at all, so that rule hides nothing. process() runs inside the red-zoned arena (row strides n + 37); the cases with their own
strides and the in-place ones bring their own device buffers, whose bytes around the rows must survive. Edge shapes come from
sdrhip_agc_plan_info. Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import libsdr_amd as sa

try:   # torch brings its own HIP runtime: it only finds the GPU when it initialises before libsdrhip.so does
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()
except Exception:   # pragma: no cover
    torch = None

import agc_restatement as R

pytestmark = pytest.mark.gpu

DT = {"i16": np.int16, "f32": np.float32}
KERNEL = {"i16": "agc_i16_kernel", "f32": "agc_f32_kernel"}
MAN = R.manifest()
FILL = 0x5A
LAMS = [R.design_lambda(t, fs) for t, fs in ((0.1, 22050.0), (0.02, 22050.0), (0.002, 48000.0), (0.01, 8000.0), (0.0005, 8000.0))]


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def same_state(bank, ref):
    g, s, e = bank.get_state()
    return R.same(g, ref.gain) and R.same(s, ref.sd) and np.array_equal(e, ref.enabled)


def seeded_rows(dtype, C, n, seed):
    """Noise at a level per row, with runs of zeros (short: sd stays normal, no inf, no NaN) and full-scale samples."""
    r = np.random.default_rng(seed)
    level = r.uniform(0.002, 0.6, (C, 1))
    x = r.uniform(-1, 1, (C, n)) * level
    for c in range(C):
        for _ in range(1 + n // 400):
            a = int(r.integers(0, max(1, n)))
            x[c, a:a + int(r.integers(1, 60))] = 0.0
            b = int(r.integers(0, max(1, n)))
            x[c, b:b + int(r.integers(1, 9))] = r.choice([-1.0, 1.0])
    if np.dtype(dtype) == np.int16:
        y = np.clip(np.floor(x * 32767 + 0.5), -32768, 32767)
        y[x == -1.0] = -32768
        return y.astype(np.int16)
    return x.astype(np.float32)


def params(dtype, C, seed):
    """Per row a lambda and a target of its own; rows 3, 10, ... disabled with a held gain, rows 5, 12, ... pass-through."""
    r = np.random.default_rng(seed)
    lam = np.array([LAMS[int(i)] for i in r.integers(0, len(LAMS), C)], np.float32)
    scale = 16000.0 if np.dtype(dtype) == np.int16 else 0.5
    target = (r.uniform(0.2, 1.5, C) * scale).astype(np.float32)
    target[::4] = 0.0   # (the type's default)
    held = [c for c in range(C) if c % 7 == 3]
    passed = [c for c in range(C) if c % 7 == 5]
    return lam, target, held, passed


def make_pair(ctx, dtype, C, seed, max_in):
    """-> (bank, restatement) with equal parameters and state; the held and pass-through rows are made with the setters"""
    lam, target, held, passed = params(dtype, C, seed)
    en = np.ones(C, bool)
    en[held + passed] = False
    bank = sa.AGCBank(ctx, dtype, lam, target, en, max_in=max_in)
    ref = R.Bank(dtype, lam, target, en)
    for c in held:
        bank.set_gain(c, 2.5 + c)
        ref.gain[c] = np.float32(2.5 + c)
    for c in passed:
        bank.set_gain(c, 0.0)
        ref.gain[c] = np.float32(0)
    assert same_state(bank, ref)
    return bank, ref


def own_buffers(ctx, bank, x, in_stride, out_stride, inplace=False):
    """x [C, n] through process_dev on this test's device rows of the given strides (in place: one buffer, equal strides).
    The bytes between and behind the rows must keep their fill, and the input rows their samples."""
    C, n = x.shape
    eb = x.dtype.itemsize
    hin = np.full((C, in_stride), 0, x.dtype)
    hin.view(np.uint8)[...] = FILL
    hin[:, :n] = x
    hout = np.full((C, out_stride), 0, x.dtype)
    hout.view(np.uint8)[...] = FILL
    din = ctx.malloc(max(hin.nbytes, 16))
    dout = din if inplace else ctx.malloc(max(hout.nbytes, 16))
    try:
        ctx.h2d(din, hin)
        if not inplace:
            ctx.h2d(dout, hout)
        bank.process_dev(din, n, in_stride, dout, in_stride if inplace else out_stride)
        ctx.synchronize()
        got_in, got_out = np.empty_like(hin), np.empty_like(hin if inplace else hout)
        ctx.d2h(got_in, din)
        ctx.d2h(got_out, dout)
    finally:
        ctx.free(din)
        if not inplace:
            ctx.free(dout)
    if not inplace:
        assert np.array_equal(got_in.view(np.uint8), hin.view(np.uint8)), "the call wrote into its input rows"
    assert np.all(got_out[:, n:].view(np.uint8) == FILL), "bytes behind a row's n samples were written"
    return got_out[:, :n].copy()


# ---- 1. the fixture streams ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(MAN))
def test_fixture_stream_as_rows_of_one_bank(ctx, name):
    """Rows 1 and 3 of a five-row bank are the reference's node on the fixture stream, in its recorded call split with its
    setter calls; rows 0, 2 and 4 have other parameters and follow the restatement."""
    m, x, y = R.load(name, MAN)
    dtype, C, mine = x.dtype, 5, (1, 3)
    lam, target, _, _ = params(dtype, C, seed=len(name))
    for c in mine:
        lam[c], target[c] = R.bits_f32(m["lambda_bits"]), np.float32(m["target"])
    bank = sa.AGCBank(ctx, dtype, lam, target, max_in=max(m["lens"]))
    assert bank.kernel_names == [KERNEL[m["dtype"]]]
    ref = R.Bank(dtype, lam, target)
    assert all(ref.target[c].view(np.uint32) == m["target_bits"] for c in mine)
    rows = seeded_rows(dtype, C, x.size, seed=7 + len(name))
    for c in mine:
        rows[c] = x
    for b, (off, n) in enumerate(R.buffers(m)):
        for c in mine:
            R.apply_ops(bank, c, m, b)
            R.apply_ops(ref, c, m, b)
        got = bank.process(rows[:, off:off + n])
        want = ref.process(rows[:, off:off + n])
        if not name.endswith("silence"):
            assert not np.isnan(want.astype(np.float64)).any()
        for c in mine:
            assert R.same(got[c], y[off:off + n]), (name, b, c)
        assert R.same(got, want), (name, b)
        g, s, e = bank.get_state()
        for c in mine:
            assert (g.view(np.uint32)[c], s.view(np.uint32)[c], int(e[c])) == tuple(m["state_bits"][b]), (name, b, c)
        assert same_state(bank, ref), (name, b)


@pytest.mark.parametrize("t", ["i16", "f32"])
def test_silence_zeros_nans_denormal_sd_and_infinite_gain(ctx, t):
    m, x, y = R.load("g20_agc_%s_silence" % t, MAN)
    bank = sa.AGC(ctx, DT[t], m["Fs"], m["tau"], channels=3, max_in=x.size)
    assert np.float32(bank.lam).view(np.uint32) == m["lambda_bits"]
    (o0, n0), (o1, n1) = R.buffers(m)[:2]
    got = np.concatenate([bank.process(np.tile(x[o:o + n], (3, 1))) for o, n in ((o0, n0), (o1, n1))], axis=1)
    want = y[:o1 + n1]
    for c in range(3):
        if t == "f32":
            assert np.array_equal(np.isnan(got[c]), np.isnan(want)) and np.isnan(want).sum() > 400
            assert R.same(got[c], want)
        else:
            assert np.array_equal(got[c], want) and np.all(got[c, 1000:] == 0)
    g, s, e = bank.get_state()
    assert np.all(np.isposinf(g)) and np.all(s > 0) and np.all(s < np.finfo(np.float32).tiny) and e.all()
    assert (g.view(np.uint32)[0], s.view(np.uint32)[0]) == tuple(m["state_bits"][1][:2])


# ---- 2. edge shapes, from the plan ---------------------------------------------------------------------------------------------

def _geometry(ctx, dtype):
    bank = sa.AGC(ctx, dtype, 22050.0, channels=1, max_in=16)
    p = bank.plan_info(16)
    bank.close()
    assert p["tile_samples"] >= 2 and p["channels_per_group"] >= 2
    return p["tile_samples"], p["channels_per_group"]


@pytest.mark.parametrize("which", ["1", "G-1", "G", "G+1", "2G+2"])
@pytest.mark.parametrize("t", ["i16", "f32"])
def test_edge_shapes(ctx, t, which):
    """Calls of 0, 1, T-1, T, T+1 and 2T+3 samples on 1, G-1, G, G+1 and 2G+2 rows: through the arena, on rows with strides
    larger than n, and in place. The state carries from call to call."""
    dtype = DT[t]
    T, G = _geometry(ctx, dtype)
    C = {"1": 1, "G-1": G - 1, "G": G, "G+1": G + 1, "2G+2": 2 * G + 2}[which]
    lens = [0, 1, T - 1, T, T + 1, 2 * T + 3]
    bank, ref = make_pair(ctx, dtype, C, seed=C, max_in=max(lens))
    assert bank.plan_info(max(lens)) == {"tile_samples": T, "channels_per_group": G}
    x = seeded_rows(dtype, C, 3 * sum(lens), seed=100 + C)
    off = 0
    for rnd, how in enumerate(("arena", "strides", "inplace")):
        for k, n in enumerate(lens):
            chunk = np.ascontiguousarray(x[:, off:off + n])
            off += n
            want = ref.process(chunk)
            assert not np.isnan(want.astype(np.float64)).any()
            if how == "arena":
                got = bank.process(chunk)
            elif how == "strides":
                got = own_buffers(ctx, bank, chunk, n + 5 + k, n + 11)
            else:
                got = own_buffers(ctx, bank, chunk, n + 3, n + 3, inplace=True)
            assert got.dtype == dtype and R.same(got, want), (how, n, np.flatnonzero((got != want).any(axis=1))[:8])
            assert same_state(bank, ref), (how, n)
    assert bank.kernel_names == [KERNEL[t]]


@pytest.mark.parametrize("t", ["i16", "f32"])
def test_overlapping_rows_are_refused_and_change_nothing(ctx, t):
    bank, ref = make_pair(ctx, DT[t], 4, seed=5, max_in=64)
    eb = np.dtype(DT[t]).itemsize
    p = ctx.malloc(4 * 80 * eb + 64)
    try:
        ctx.memset(p, 0, 4 * 80 * eb + 64)
        for out, so in ((p + eb, 64), (p, 70), (p + 3 * 64 * eb, 64)):   # shifted, in place with another stride, one row overlapping
            with pytest.raises(sa.SdrHipError) as e:
                bank.process_dev(p, 64, 64, out, so)
            assert e.value.code == sa.abi.E_INVALID
        with pytest.raises(sa.SdrHipError) as e:
            bank.process_dev(p, 65, 80, p + 2048, 80)
        assert e.value.code == sa.abi.E_SIZE   # n > max_in: what every equal-length node answers
        bank.process_dev(p, 64, 64, p, 64)     # in place
        ref.process(np.zeros((4, 64), DT[t]))
        assert same_state(bank, ref)
    finally:
        ctx.free(p)


# ---- 3. split invariance --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", ["i16", "f32"])
def test_one_call_equals_three_ragged_calls(ctx, t):
    dtype = DT[t]
    T, G = _geometry(ctx, dtype)
    C, N = G + 3, 3 * T + 41
    x = seeded_rows(dtype, C, N, seed=31)
    one, ref = make_pair(ctx, dtype, C, seed=9, max_in=N)
    three, _ = make_pair(ctx, dtype, C, seed=9, max_in=N)
    whole = one.process(x)
    want = ref.process(x)
    assert not np.isnan(want.astype(np.float64)).any() and R.same(whole, want)
    cuts = [0, 1, T + 7, N]
    parts = np.concatenate([three.process(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    assert R.same(parts, whole)
    for a, b in zip(one.get_state(), three.get_state()):
        assert R.same(a, b)
    assert same_state(one, ref)


# ---- 4. the setters between calls -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", ["i16", "f32"])
def test_setters_touch_one_row_and_refused_ones_nothing(ctx, t):
    dtype = DT[t]
    T, G = _geometry(ctx, dtype)
    C, n = G + 2, T + 9
    x = seeded_rows(dtype, C, 5 * n, seed=77)
    bank, ref = make_pair(ctx, dtype, C, seed=13, max_in=n)
    twin, _ = make_pair(ctx, dtype, C, seed=13, max_in=n)
    touched = set()
    new_target = 777.0 if t == "i16" else 0.125

    def step(k, change=None):
        if change:
            change()
        chunk = x[:, k * n:(k + 1) * n]
        got, und, want = bank.process(chunk), twin.process(chunk), ref.process(chunk)
        assert not np.isnan(want.astype(np.float64)).any()
        assert R.same(got, want), k
        rest = [c for c in range(C) if c not in touched]
        assert R.same(got[rest], und[rest]), k
        gs, ts = bank.get_state(), twin.get_state()
        for a, b in zip(gs, ts):
            assert R.same(a[rest], b[rest]), k
        assert same_state(bank, ref), k

    step(0)

    def fresh():   # a fresh node behind row 2, the last row's decay changed
        touched.update((2, C - 1))
        bank.set_channel(2, LAMS[2], new_target)
        ref.set_channel(2, LAMS[2], new_target)
        bank.set_lambda(C - 1, LAMS[4])
        ref.lam[C - 1] = LAMS[4]
    step(1, fresh)

    def hold():   # row 0 disabled: its gain is held; row 1 disabled and set to 3
        touched.update((0, 1))
        bank.set_enabled(0, False); ref.enabled[0] = False
        bank.set_enabled(1, False); ref.enabled[1] = False
        bank.set_gain(1, 3.0); ref.gain[1] = np.float32(3)
    step(2, hold)

    def refused():
        before = bank.get_state()
        for call in (lambda: bank.set_channel(C, LAMS[0], new_target), lambda: bank.set_channel(-1, LAMS[0], new_target),
                     lambda: bank.set_channel(4, 1.0, new_target), lambda: bank.set_channel(4, LAMS[0], -1.0),
                     lambda: bank.set_channel(4, LAMS[0], float("inf")), lambda: bank.set_lambda(4, -0.1), lambda: bank.set_lambda(C, 0.5),
                     lambda: bank.set_enabled(C, True), lambda: bank.set_gain(-1, 2.0)):
            with pytest.raises(sa.SdrHipError) as e:
                call()
            assert e.value.code == sa.abi.E_INVALID
        for a, b in zip(before, bank.get_state()):
            assert R.same(a, b)
    step(3, refused)

    def back():   # row 0 enabled again, row 1 pass-through
        bank.set_enabled(0, True); ref.enabled[0] = True
        bank.set_gain(1, 0.0); ref.gain[1] = np.float32(0)
    step(4, back)
    bank.reset()
    ref.reset()
    assert same_state(bank, ref)


@pytest.mark.parametrize("t", ["i16", "f32"])
def test_every_setter_refuses_a_row_outside_the_bank(ctx, t):
    """The smallest bank that has two rows to tell apart: 2 rows, max_in 64, one call each. Rows -1 and 2 are refused by every
    setter with the range in the message and nothing changed; a set_channel that succeeds leaves the other row as it is in a
    bank that was never touched."""
    dtype, C, n = DT[t], 2, 64
    x = seeded_rows(dtype, C, 2 * n, seed=55)
    bank, ref = make_pair(ctx, dtype, C, seed=21, max_in=n)
    twin, _ = make_pair(ctx, dtype, C, seed=21, max_in=n)
    for c in (-1, C):
        for call in (lambda: bank.set_channel(c, LAMS[0], 1.0), lambda: bank.set_lambda(c, LAMS[0]), lambda: bank.set_enabled(c, False),
                     lambda: bank.set_gain(c, 2.0)):
            with pytest.raises(sa.SdrHipError) as e:
                call()
            assert e.value.code == sa.abi.E_INVALID and "outside [0,2)" in str(e.value), (c, str(e.value))
    got, und, want = bank.process(x[:, :n]), twin.process(x[:, :n]), ref.process(x[:, :n])
    assert not np.isnan(want.astype(np.float64)).any()
    assert R.same(got, want) and R.same(got, und) and same_state(bank, ref)
    new_target = 777.0 if t == "i16" else 0.125
    bank.set_channel(1, LAMS[2], new_target)
    ref.set_channel(1, LAMS[2], new_target)
    got, und, want = bank.process(x[:, n:]), twin.process(x[:, n:]), ref.process(x[:, n:])
    assert not np.isnan(want.astype(np.float64)).any()
    assert R.same(got, want) and R.same(got[:1], und[:1]) and same_state(bank, ref)
    for a, b in zip(bank.get_state(), twin.get_state()):
        assert R.same(a[:1], b[:1])


@pytest.mark.parametrize("t", ["i16", "f32"])
def test_pass_through_rows_copy_and_held_rows_follow(ctx, t):
    dtype = DT[t]
    C, n = 9, 300
    bank, ref = make_pair(ctx, dtype, C, seed=3, max_in=n)
    _, _, held, passed = params(dtype, C, 3)
    assert held and passed
    x = seeded_rows(dtype, C, n, seed=41)
    before = bank.get_state()
    got, want = bank.process(x), ref.process(x)
    assert R.same(got, want) and not np.isnan(want.astype(np.float64)).any()
    after = bank.get_state()
    for c in passed:
        assert np.array_equal(got[c], x[c])
        assert all(R.same(a[c:c + 1], b[c:c + 1]) for a, b in zip(before, after))
    for c in held:
        assert after[0][c] == before[0][c] and after[1][c] != before[1][c] and not np.array_equal(got[c], x[c])
    assert same_state(bank, ref)


# ---- 5. behind a tuner bank, on its device rows -----------------------------------------------------------------------------------

def test_device_chain_behind_a_tuner_bank(ctx, orc):
    from test_gpu_parity_tuner import FS, Ref, bank_tunes
    C, N, D, order = 8, 4096, 8, 127
    modes = [sa.EPI_AM, sa.EPI_USB] * (C // 2)
    tunes = bank_tunes(C, order, seed=20)
    lut = sa.design_freqshift_lut_i16()
    taps = np.stack([np.asarray(tn[0], np.int32).reshape(-1, 2) for tn in tunes])
    tuner = sa.TunerBankI16(ctx, taps, lut, [tn[1] for tn in tunes], [tn[2] for tn in tunes], D, max_in=N, modes=modes)
    x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3), (210e3, 9000, 1.0), (700e3, 5000, 2.0)]).next_cs16(2 * N)
    cap = N // D + 1   # (a call's output count depends on where the decimator stands: the tuner reports it)
    lam = np.full(C, R.design_lambda(0.01, FS / D), np.float32)
    agc = sa.AGCBank(ctx, np.int16, lam, max_in=cap)
    ref = R.Bank(np.int16, lam)
    refs = [Ref(orc, tn[0], lut, tn[1], tn[2], D, m) for tn, m in zip(tunes, modes)]
    stride = cap + 24
    din, drows, dout = ctx.malloc(x[:N].nbytes), ctx.malloc(C * stride * 2), ctx.malloc(C * stride * 2)
    try:
        for k in range(2):
            chunk = np.ascontiguousarray(x[k * N:(k + 1) * N])
            ctx.h2d(din, chunk)
            no = tuner.process_dev(din, N, drows, stride)
            assert 0 < no <= cap
            agc.process_dev(drows, no, stride, dout, stride)   # the tuner's device rows, no host copy in between
            ctx.synchronize()
            got = np.zeros((C, stride), np.int16)
            ctx.d2h(got, dout)
            audio = np.stack([r.process(chunk) for r in refs])
            assert audio.shape == (C, no)
            want = ref.process(audio)
            assert np.array_equal(got[:, :no], want), k
            assert np.abs(want.astype(np.int32)).max() > 0
        g, s, e = agc.get_state()
        assert R.same(s, ref.sd) and R.same(g, ref.gain)   # sd: the rows' signal levels
    finally:
        for p in (din, drows, dout):
            ctx.free(p)


def test_every_compiled_instance_was_named(ctx):
    """The code object holds two AGC kernels (tests/test_agc_abi.py); a bank of each type reports its own."""
    names = set()
    for t in ("i16", "f32"):
        bank = sa.AGC(ctx, DT[t], 8000.0, channels=2, max_in=8)
        bank.process(np.ones((2, 8), DT[t]))
        names.update(bank.kernel_names)
    assert names == set(KERNEL.values())
