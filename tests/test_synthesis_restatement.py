"""The synthesis bank's restatement (tests/synthesis_restatement.py) checked against itself, without a GPU: the definition
against the fast form (<= 1e-12 of the largest output, on the shapes of the GPU parity test), Stream against one call whatever
the cut, Stream's state, and the margins of the synthesis -> analysis chain (tests/test_gpu_synthesis_chain.py) on the two
restatements alone, before any device is involved."""
import numpy as np
import pytest

import channelizer_restatement as CR
import synthesis_restatement as R

# (M, D, n_taps, channels, columns): the GPU parity test's shapes
SHAPES = [(8, 8, 17, None, 10), (12, 5, 30, [3, 0, 11], 11), (26, 26, 52, None, 5), (77, 40, 300, [76, 1], 7), (6, 1, 7, None, 20),
          (16, 2, 128, [5], 70), (16, 16, 5, None, 6), (1024, 512, 4096, None, 16), (4096, 4096, 8192, None, 3)]


def case(M, D, n_taps, channels, n, seed=0):
    rng = np.random.default_rng(1000 * M + D + n_taps + seed)
    rows = M if channels is None else len(channels)
    c = rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))
    t = np.arange(n_taps) - (n_taps - 1) / 2
    g = R.round32(np.sinc(t / M) * np.hanning(n_taps + 2)[1:-1] * D / M)
    return c, g


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s[:3])
def test_direct_against_folded(shape):
    M, D, n_taps, channels, n = shape
    c, g = case(*shape)
    f = R.folded(c, g, M, D, channels)
    assert f.shape == (n * D,)
    times = np.arange(n * D)
    if n * D > 600:                                   # a few hundred output times, the first and the last among them
        rng = np.random.default_rng(M)
        times = np.unique(np.concatenate([[0, 1, D - 1, D, n * D - 1], rng.integers(0, n * D, 300)]))
    d = R.direct(c, g, M, D, channels, times)
    err = np.abs(d - f[times]).max() / np.abs(f).max()
    assert err <= 1e-12, err


def test_outputs_without_a_term_are_zero():
    M, D, n_taps, channels, n = 16, 16, 5, None, 6
    c, g = case(M, D, n_taps, channels, n)
    f = R.folded(c, g, M, D).reshape(n, D)
    assert np.all(f[:, n_taps:] == 0) and np.all(f[:, :n_taps] != 0)
    assert np.all(R.direct(c, g, M, D).reshape(n, D)[:, n_taps:] == 0)


@pytest.mark.parametrize("shape", SHAPES[:7], ids=lambda s: "%d-%d-%d" % s[:3])
def test_stream_split_invariance(shape):
    M, D, n_taps, channels, n = shape
    c, g = case(*shape)
    whole = R.folded(c, g, M, D, channels)
    for lens in ([n], [0, 1, n - 1], [1] * n, [n // 2, 0, n - n // 2]):
        s = R.Stream(g, M, D, channels)
        parts, off = [], 0
        for k in lens:
            assert s.out_count(k) == k * D
            parts.append(s.process(c[:, off:off + k]))
            off += k
        assert np.array_equal(np.concatenate(parts), whole), lens
        consumed, cols = s.state()
        Q = -(-n_taps // D)
        assert consumed == n and cols.shape == (Q - 1, M)
        v = R.transform(c, M, channels)
        k = min(Q - 1, n)
        assert np.array_equal(cols[Q - 1 - k:], v[n - k:]) and not cols[:Q - 1 - k].any()
        s.reset()
        assert s.state()[0] == 0 and np.array_equal(s.process(c), whole)


def test_stream_setters_between_calls():
    M, D, n_taps, n = 12, 5, 30, 11
    c, g = case(M, D, n_taps, None, n)
    s = R.Stream(g, M, D)
    a = s.process(c[:, :4])
    s.set_channels([3, 0, 11])
    s.set_taps(g[::-1])
    b = s.process(c[[3, 0, 11], 4:])
    zeroed = c.copy()
    zeroed[[k for k in range(M) if k not in (3, 0, 11)], 4:] = 0
    v = R.transform(zeroed, M)
    assert np.array_equal(a, R.overlap(v, g, M, D, 0, 4)) and np.array_equal(b, R.overlap(v, g[::-1], M, D, 4, n - 4))


def test_a_selection_is_the_full_call_with_zero_rows():
    M, D, n_taps, channels, n = 77, 40, 300, [76, 1], 7
    c, g = case(M, D, n_taps, channels, n)
    full = np.zeros((M, n), np.complex128)
    full[channels] = c
    assert np.array_equal(R.folded(c, g, M, D, channels), R.folded(full, g, M, D))
    assert np.array_equal(R.folded(c[::-1], g, M, D, channels[::-1]), R.folded(c, g, M, D, channels))


def test_the_chain_margins_hold_on_the_restatements():
    """synthesis (taps D h) -> analysis (taps h): the used channels come back delayed by 15 columns, the others stay 60 dB down"""
    k = R.chain_case()
    for form in ("folded", "direct"):
        if form == "folded":
            z = R.folded(R.rows_of(k["x"]), R.round32(k["D"] * k["h"]), k["M"], k["D"], k["channels"])
            z32 = R.as_pairs(z).astype(np.float32)       # (the row the channelizer reads is float32)
            y = CR.folded(CR.pairs(z32), CR.round32(k["h"]), k["M"], k["D"])
        else:
            z = R.direct(R.rows_of(k["x"]), R.round32(k["D"] * k["h"]), k["M"], k["D"], k["channels"])
            y = CR.direct(z, CR.round32(k["h"]), k["M"], k["D"], list(range(k["M"])))
        assert y.shape == (16, 96)
        err, db = R.chain_margins(k, y)
        print("chain on the restatements (%s): row error %.3g of the amplitude, strongest other channel %.1f dB" % (form, err, db))
        assert err <= 1e-2 and db <= -60.0, (form, err, db)
