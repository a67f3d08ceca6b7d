"""The numpy restatement of the interpolating resampler bank (tests/resample_restatement.py) against the fixtures cut from the
unmodified reference InpolSubSampler (tools/golden_resample -> tests/golden/g22_inpol_*): outputs, counts, mu and the line after
every call, BIT FOR BIT (float rows by their bit patterns except where both sides are NaN — the fixtures hold none). Then what
the contract says follows from the loop: the capacity bound over a sweep of fractions and call lengths, and the three edge
streams with the table rows they take."""
import numpy as np
import pytest

import resample_restatement as R

f32 = np.float32


def same(a, b):
    """bit for bit, except where both sides are NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def test_the_fixtures_are_all_there_and_small():
    names = R.fixture_names()
    assert len(names) == 16 and {R.manifest()[n]["dtype"] for n in names} == set(R.DTYPES)
    for n in names:
        m, x, y, lines = R.fixture(n)
        assert m["Fs"] == 8000 and sum(m["lens"]) == m["count"] == len(x) and sum(m["counts"]) == m["outputs"] == len(y)
        assert m["lens"][:5] == [5, 5, 1, 256, 257] and 0 in m["lens"]
        assert f32(m["frac"]).view(np.uint32) == m["frac_bits"]
        for a in (x, y, lines):
            assert a.nbytes < (1 << 20) and (a.dtype != np.float32 or not np.isnan(a).any())
    assert sorted({f32(R.manifest()[n]["frac"]) for n in names}) == [f32(0.5), f32(1.378125), f32(2.0), f32(7.9)]
    for d in ("i16", "cs16_cf32"):       # the full-scale stretch
        x = R.fixture("g22_inpol_%s_2" % d)[1]
        assert (x == 32767).sum() >= 100 and (x == -32768).sum() >= 100


@pytest.mark.parametrize("name", R.fixture_names())
def test_restatement_equals_the_reference(name):
    m, x, y, lines = R.fixture(name)
    bank = R.Bank(m["dtype"], [m["frac"]], R.table())
    off = at = 0
    for b, n in enumerate(m["lens"]):
        got = bank.process(x[None, off:off + n])[0]
        off += n
        assert len(got) == m["counts"][b], (name, b, len(got), m["counts"][b])
        assert len(got) <= bank.out_capacity(n)
        assert same(got, y[at:at + len(got)]), (name, b)
        at += len(got)
        mu, line = bank.state()
        assert int(mu[0]) == m["mu_bits"][b], (name, b)
        assert same(line[0], lines[b]), (name, b)
    assert at == len(y)


def test_the_int16_accumulator_wraps_where_the_float_node_overshoots():
    """the full-scale step at frac = 1.378125: where the float node overshoots full scale, the reference's int16 output has
    wrapped to the other sign — it does not saturate"""
    m, x, y, _ = R.fixture("g22_inpol_i16_1p378125")
    fl = R.Bank("f32", [m["frac"]], R.table())
    yf = np.concatenate([fl.process(x[None, o:o + n].astype(f32))[0] for o, n in zip(np.cumsum([0] + m["lens"][:-1]), m["lens"])])
    over = np.flatnonzero(np.abs(yf) > f32(32800))
    assert over.size, "the float node never overshoots: the fixture does not reach the wrap"
    assert np.all(np.sign(y[over].astype(np.int64)) == -np.sign(yf[over])), (y[over][:8], yf[over][:8])


FRACS = [0.0625, 0.13, 0.3, 0.5, 0.999, 1.0000001, 1.378125, 1.5, 2.0, 3.7, 7.9, 45.35, 256.0]
LENS = [1, 2, 7, 64, 255, 300, 773]


def test_capacity_bound_holds_and_is_reached():
    """13 fractions from 0.0625 (below what the node takes: the bound is the chain's) to 256, seven call lengths, six consecutive
    calls each: no call writes more than floor((n + 1) / frac) + 2. In exact arithmetic the most is floor((n + 1) / frac) + 1 (a
    fresh row that ends its call on mu = 1 + frac); the last + 1 is the allowance for the float chain's roundings, which no
    case of this sweep uses: the bound less that allowance is what is reached."""
    reached = False
    for frac in FRACS:
        for n in LENS:
            mu = f32(0)
            cap = R.out_capacity([frac], n)
            for _ in range(6):
                pos, rows, mu = R.chain(frac, mu, n)
                assert len(pos) <= cap, (frac, n, len(pos), cap)
                assert f32(0) <= mu <= f32(1) + f32(frac)
                reached |= len(pos) == cap - 1
                assert rows.min(initial=0) >= 0 and rows.max(initial=0) <= 128
    assert reached
    assert R.out_capacity([2.0], 0) == 0 and R.out_capacity([1.0], 300) == 300 and R.out_capacity([1.0, 0.5], 300) == 604
    assert R.out_capacity([0.125], 256) == 8 * 256 + 10 and R.out_capacity([300.0], 255) == 2


def test_a_fresh_rows_first_output_comes_from_the_zero_line():
    x = np.arange(1, 5, dtype=f32)
    bank = R.Bank("f32", [1.5], R.table())
    y = bank.process(x[None])[0]
    pos, rows, _ = R.chain(1.5, 0.0, 4)
    assert pos[0] == 0 and rows[0] == 0 and y[0] == 0
    assert bank.process(x[None, :0])[0].size == 0          # n = 0 emits nothing and changes nothing
    mu, line = bank.state()
    assert np.array_equal(line[0, 4:], x)
    assert same(bank.state()[0], mu)


def test_frac_half_takes_every_second_output_at_row_128():
    pos, rows, mu = R.chain(0.5, 0.0, 6)
    # three outputs from the fresh line (mu = 0, 0.5, 1), then two behind every sample (mu = 0.5, 1)
    assert rows.tolist() == [0, 64, 128] + [64, 128] * 6 and mu == f32(1.5)
    assert pos.tolist() == [0, 0, 0] + [p for p in range(1, 7) for _ in range(2)]


def test_frac_two_odd_calls_end_on_row_128():
    def rows_of(lens):
        mu, out, counts = f32(0), [], []
        for n in lens:
            _, rows, mu = R.chain(2.0, mu, n)
            out += rows.tolist()
            counts.append(len(rows))
        return out, counts
    assert rows_of([5, 5]) == ([0, 0, 0, 128, 0, 0], [4, 2])
    assert rows_of([10]) == ([0] * 6, [6])
    assert rows_of([4, 6]) == ([0] * 6, [3, 3])
    # Row 0 is the impulse at tap 4: the output at window position p is sample p - 4 (0 before the stream). The unsplit stream
    # takes p = 0, 2, ..., 10. The split one takes row 128 at p = 5 where the unsplit one takes row 0 at p = 6 (sample 2, value 3):
    # with the reference's table row 128 is all zeros; with a table whose row 128 is the impulse at tap 3 it is sample p - 5 = 0.
    x = np.arange(1, 11, dtype=f32)
    tab = R.table()
    assert not tab[128].any() and tab[0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]

    def streams(t):
        split, whole = R.Bank("f32", [2.0], t), R.Bank("f32", [2.0], t)
        return np.concatenate([split.process(x[None, :5])[0], split.process(x[None, 5:])[0]]).tolist(), whole.process(x[None])[0].tolist()
    assert streams(tab) == ([0, 0, 1, 0, 5, 7], [0, 0, 1, 3, 5, 7])
    own = np.zeros((129, 8), f32)
    own[0, 4] = own[128, 3] = 1
    assert streams(own) == ([0, 0, 1, 1, 5, 7], [0, 0, 1, 3, 5, 7])
