"""The restatement of the real-input channelizer family (tests/chanreal_restatement.py) against itself, no GPU: the definition
(direct_real: channelizer_restatement.direct on (x, 0)) against the fast form in the header's order (folded_real) to <= 1e-12 of
the largest output over the shapes of the GPU parity test; any cut of a stream into calls against one call; y_0 and y_H real."""
import numpy as np
import pytest

import chanreal_restatement as RR

BOUND = 1e-12


def _signal(n, seed):
    return np.random.default_rng(seed).integers(-20000, 20000, n).astype(np.float64)


@pytest.mark.parametrize("shape", RR.SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_the_fast_form_is_the_definition(shape):
    M, D, n_taps = shape
    T = RR.tile_times(M)
    n_out = 3 * T + 1
    x, h = _signal(n_out * D, M + D + n_taps), RR.round32(RR.prototype(M, n_taps))
    # (M = 4096: the definition's phase matrix is 2049 x 8192 per output time — the first six and the last two)
    spans = [(0, n_out)] if M < 4096 else [(0, 6), (n_out - 2, 2)]
    for first, count in spans:
        d, f = RR.direct_real(x, h, M, D, first, count), RR.folded_real(x, h, M, D, first, count)
        assert d.shape == f.shape == (M // 2 + 1, count)
        err = float(np.abs(d - f).max() / np.abs(d).max())
        print("chanreal restatement %s [%d, +%d): max |direct - folded| / max |direct| = %.3g" % (shape, first, count, err))
        assert err <= BOUND, err
        # channel 0 and channel H are real rows
        assert not f[0].imag.any() and not f[M // 2].imag.any()
        assert np.abs(d[[0, M // 2]].imag).max() <= BOUND * np.abs(d).max()


def test_plan_rule():
    assert [RR.tile_times(M) for M in (4, 512, 514, 1000, 4096)] == [256, 8, 15, 8, 2]
    assert [RR.image_stride(M) for M in (4, 26, 1000, 4096)] == [3, 15, 501, 2049]
    # a workgroup's images: 8 T ld <= 4 E + 16 T bytes — 32 KiB and at most 232 bytes (M = 546), four workgroups to a 160 KiB CU
    assert 2 * 2049 * 8 == 32768 + 16
    worst = max(RR.tile_times(M) * RR.image_stride(M) * 8 for M in range(4, 4097, 2))
    assert worst == 32768 + 232 and 4 * worst <= 160 * 1024


@pytest.mark.parametrize("shape", [(4, 3, 9), (12, 5, 30), (26, 13, 57), (64, 64, 40)], ids=lambda s: "%d-%d-%d" % s)
@pytest.mark.parametrize("form", [RR.folded_real, RR.direct_real], ids=["folded", "direct"])
def test_any_split_of_the_stream(shape, form):
    M, D, n_taps = shape
    n = 9 * D + 2
    x, taps = _signal(n, 3 * M + D), RR.prototype(M, n_taps)
    whole = RR.Stream(taps, M, D, form=form).process(x)
    assert whole.shape == (M // 2 + 1, n // D)
    rng = np.random.default_rng(M)
    for cuts in ([0, 1, D - 1, D + 1], sorted(int(c) for c in rng.integers(0, n, 6))):
        s, parts, off = RR.Stream(taps, M, D, form=form), [], 0
        lens = [0, 1, D - 1, D + 1, n - 2 * D - 1] if cuts == [0, 1, D - 1, D + 1] else list(np.diff([0] + cuts + [n]))
        for length in lens:
            assert s.out_count(length) == (off + length) // D - off // D
            parts.append(s.process(x[off:off + length]))
            off += length
        assert off == n and np.array_equal(np.concatenate(parts, axis=1), whole)
        consumed, tail = s.state()
        assert consumed == n and tail.shape == (n_taps - 1, 2) and not tail[:, 1].any()
        k = min(n_taps - 1, n)
        assert np.array_equal(tail[n_taps - 1 - k:, 0], x[n - k:])


def test_selection_and_set_taps():
    M, D, n_taps = 12, 5, 30
    x, taps = _signal(61, 5), RR.prototype(M, n_taps)
    full = RR.Stream(taps, M, D)
    sel = RR.Stream(taps, M, D, [6, 0, 3])
    a, b = full.process(x[:31]), sel.process(x[:31])
    assert np.array_equal(a[[6, 0, 3]], b)
    other = taps[::-1] * np.linspace(0.5, 1.5, n_taps)
    full.set_taps(other)
    sel.set_taps(other)
    sel.set_channels(None)
    assert np.array_equal(full.process(x[31:]), sel.process(x[31:]))
    full.reset()
    assert full.state()[0] == 0 and np.array_equal(full.process(x[:31]), RR.Stream(other, M, D).process(x[:31]))
