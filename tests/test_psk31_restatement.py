"""The BPSK31 node's contract (include/sdrhip_psk31.h) on the CPU: the numpy restatement against the fixtures cut from the
reference (tests/golden/g21_psk31_*, tools/golden_psk31), the defined sincos, the library's interpolation-table designer, the
capacity bound and the host-side Varicode decoder."""
import functools
import os

import numpy as np
import pytest

import psk31_restatement as R

f32, f64 = np.float32, np.float64
OTHER_SPLIT = {8000.0: [7999, 1, 8000, 0, 33, 7967], 2000.0: [1999, 1, 2000, 0, 33, 1967]}


@functools.lru_cache(maxsize=None)
def _run(Fs, sincos, other):
    """the fixtures of one sample rate side by side -> names, the call lengths, per call the rows' bits and the state"""
    names = [n for n in R.fixture_names() if R.manifest()[n]["Fs"] == Fs]
    fx = [R.fixture(n) for n in names]
    lens = OTHER_SPLIT[Fs] if other else fx[0][0]["lens"]
    bank = R.Bank(Fs, [m["dF"] for m, _, _ in fx], R.table(), sincos=sincos)
    x = np.stack([x.astype(f32) for _, x, _ in fx])
    assert sum(lens) == x.shape[1]
    got, states, off = [], [], 0
    for L in lens:
        got.append(bank.process(x[:, off:off + L]))
        states.append(bank.state())
        off += L
    return names, lens, got, states, bank.row128


@pytest.mark.parametrize("Fs", [8000.0, 2000.0])
def test_a_libm_sincos_reproduces_the_reference_bit_for_bit(Fs):
    """Skips only where the local C library's sincosf is not the one that cut the fixtures (the recorded probe says)."""
    if not R.libm_matches_probe():
        pytest.skip("the local sincosf differs from the one recorded with the fixtures")
    names, lens, got, states, _ = _run(Fs, "libm", False)
    for k, name in enumerate(names):
        m, _, bits = R.fixture(name)
        assert [len(g[k]) for g in got] == m["counts"], name
        assert np.array_equal(np.concatenate([g[k] for g in got]), bits), name
        for b in range(len(lens)):
            assert states[b][k].tolist() == m["state_bits"][b], (name, b)
    # other call lengths: the same stream, the same state at the end
    _, _, got2, states2, _ = _run(Fs, "libm", True)
    for k, name in enumerate(names):
        m, _, bits = R.fixture(name)
        assert np.array_equal(np.concatenate([g[k] for g in got2]), bits), name
        assert states2[-1][k].tolist() == m["state_bits"][-1], name


@pytest.mark.parametrize("Fs", [8000.0, 2000.0])
def test_b_defined_sincos_gives_the_fixtures_bits_and_counts(Fs):
    names, lens, got, states, row128 = _run(Fs, "defined", False)
    worst = 0.0
    for k, name in enumerate(names):
        m, _, bits = R.fixture(name)
        assert [len(g[k]) for g in got] == m["counts"], name
        assert np.array_equal(np.concatenate([g[k] for g in got]), bits), name
        for b in range(len(lens)):
            a = states[b][k][:4].astype(np.uint32).view(f32)
            w = np.array(m["state_bits"][b][:4], np.uint32).view(f32)
            worst = max(worst, float(np.max(np.abs(a - w))))
    print("largest deviation of P, F, mu, omega from the reference at %g Hz: %g" % (Fs, worst))   # (no bar: recorded in the manifest)
    if Fs == 8000.0:
        assert row128 > 0   # the fixtures reach the table's all-zero row 128
        assert sum(R.manifest()[n]["row128_sub_samples"] for n in names) > 0


def test_fixtures_cover_what_they_are_for():
    m = R.manifest()
    assert {m[n]["dtype"] for n in R.fixture_names()} == {"cs16", "cf32"} and {m[n]["Fs"] for n in R.fixture_names()} == {2000, 8000}
    for n in R.fixture_names():
        assert max(m[n]["lens"]) <= m[n]["Fs"], n   # calls of at most one second
        assert os.path.getsize(os.path.join(R.GOLDEN, m[n]["x"])) < (1 << 20)
    F = lambda n, b: np.array([m[n]["state_bits"][b][1]], np.uint32).view(f32)[0]
    w = lambda n, b: np.array([m[n]["state_bits"][b][3]], np.uint32).view(f32)[0]
    clamp = "g21_psk31_cs16_clamp"
    assert any(abs(F(clamp, b)) == f32(m[clamp]["dF"]) for b in range(len(m[clamp]["lens"])))          # F rides its clamp
    baud = "g21_psk31_cs16_baud"
    lo, hi = (np.array([m[baud][k]], np.uint32).view(f32)[0] for k in ("min_omega_bits", "max_omega_bits"))
    assert any(w(baud, b) in (lo, hi) for b in range(len(m[baud]["lens"])))                             # omega rides its clamp
    _, x, _ = R.fixture("g21_psk31_cf32_zeros")
    assert not x[:2500].any() and x[2500:].any()
    a, b = R.pll_gains()
    assert a.view(np.uint32) == m[clamp]["alpha_bits"] and b.view(np.uint32) == m[clamp]["beta_bits"]
    for n in R.fixture_names():
        _, lo, hi = R.omegas(m[n]["Fs"])
        assert lo.view(np.uint32) == m[n]["min_omega_bits"] and hi.view(np.uint32) == m[n]["max_omega_bits"], n


def _ulp_err(got, exact):
    """|got - exact| in units of the float32 spacing at exact (exact: float64)"""
    ref = exact.astype(f32)
    ulp = np.spacing(np.abs(ref)).astype(f64)
    return np.abs(got.astype(f64) - ref.astype(f64)) / ulp


def test_c_psk_sincos_is_within_one_ulp():
    """2^24 evenly spaced float bit patterns of [-2 pi, 2 pi], both ends and every binade edge"""
    top = int(f32(2 * np.pi).view(np.uint32))   # (float(2 pi) lies just above 2 pi; P never exceeds it after the wrap)
    pos = np.linspace(0, top, 1 << 23).astype(np.uint32)
    edges = np.array([e << 23 for e in range(1, 130)] + [(e << 23) - 1 for e in range(1, 130)] + [0, 1, top, top - 1], np.uint32)
    edges = edges[edges <= top]
    worst = 0.0
    for chunk in np.array_split(np.concatenate([pos, edges]), 16):
        for sign in (0, 0x80000000):
            P = (chunk | np.uint32(sign)).view(f32)
            s, c = R.psk_sincos(P)
            d = P.astype(f64)
            es, ec = _ulp_err(s, np.sin(d)), _ulp_err(c, np.cos(d))
            worst = max(worst, float(es.max()), float(ec.max()))
    print("psk_sincos: worst error %.3f ulp of float(sin(double)) / float(cos(double))" % worst)
    assert worst <= 1.0
    s, c = R.psk_sincos(np.array([np.nan], f32))
    assert np.isnan(s[0]) and np.isnan(c[0])


def _tone_error(tab, rows):
    """worst |interpolated - exact| of a complex tone at 0.1 cycles per sample over the table rows given"""
    w, k = 2 * np.pi * 0.1, np.arange(8) - 4
    return max(abs(np.sum(tab[r].astype(f64) * np.exp(1j * w * k)) - np.exp(-1j * w * r / 128.0)) for r in rows)


def test_d_designed_table():
    import libsdr_amd as sa
    t, ref = sa.design_inpol_taps(), R.table()
    assert t.shape == (129, 8) and t.dtype == f32 and np.all(np.isfinite(t))
    assert t[0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and t[128].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert np.array_equal(t, t[::-1, ::-1])   # row r mirrors row 128 - r
    ours, theirs = _tone_error(t, range(65)), _tone_error(ref, range(65))
    print("tone at 0.1 cycles/sample, rows 0 ... 64: designed %.6g, reference %.6g" % (ours, theirs))
    assert ours <= 2 * theirs
    # the whole designed table interpolates; the reference's rows behind 64 sit one place early and row 128 is all zeros
    assert _tone_error(t, range(129)) <= 2 * theirs
    assert not ref[128].any() and np.array_equal(ref[65], ref[62][::-1])
    m = R.manifest()
    if "designer" in m:
        assert abs(m["designer"]["designed_worst_error"] - ours) < 1e-9 and abs(m["designer"]["reference_worst_error"] - theirs) < 1e-9


def test_e_capacity_bound_holds_for_the_densest_stream():
    """omega at its lower clamp and err = -1 all the way (mu advances by min_omega - 0.01), transitions at every 33rd sub-sample,
    a call that inherits a history one short of a bit: the restatement's loop on such a stream stays within the bound"""
    for Fs in (2000.0, 2001.0, 8000.0, 48000.0):
        _, lo, hi = R.omegas(Fs)
        for n in (1, 2, 33, 500, 2000, 8000):
            mu, subs, i = f32(0.0), 0, 0
            while i < n:                      # the loop of the contract with the smallest advance
                if mu > 1:
                    mu = f32(mu - f32(1)); i += 1
                else:
                    subs += 1
                    mu = f32(mu + f32(lo + f32(f32(0.01) * f32(-1))))
            bits = 1 + (subs - 1) // 33 if subs else 0
            assert bits <= R.out_capacity(Fs, n), (Fs, n, subs, bits)
            assert subs <= int(np.floor((n + 3.0 + float(hi)) / (float(lo) - 0.0100001))) + 1
    assert R.out_capacity(8000.0, 0) == 0
    # and the fixtures' calls
    m = R.manifest()
    for name in R.fixture_names():
        for L, c in zip(m[name]["lens"], m[name]["counts"]):
            assert c <= R.out_capacity(m[name]["Fs"], L), (name, L, c)


def test_f_varicode_against_the_reference():
    import libsdr_amd as sa
    from libsdr_amd.psk31 import VARICODE
    m = R.manifest()["g21_varicode"]
    bits = np.fromfile(os.path.join(R.GOLDEN, m["bits"]), np.uint8)
    text = open(os.path.join(R.GOLDEN, m["text"]), "rb").read().decode("latin1")
    assert len(bits) == m["count"] and len(text) == m["chars"]
    assert sa.Varicode(1).feed([bits])[0] == text
    # the fixture's own calls end inside codes; the characters of every call are the reference's
    v, off, got = sa.Varicode(2), 0, []
    for L, c in zip(m["lens"], m["counts"]):
        a, b = v.feed([bits[off:off + L], bits[off:off + L]])
        assert a == b and len(a) == c
        got.append(a)
        off += L
    assert "".join(got) == text
    one = sa.Varicode(1)
    assert "".join(one.feed([bits[i:i + 1]])[0] for i in range(len(bits))) == text
    assert VARICODE[0b1011101011] == "\n" and VARICODE[0b11101] == "\n" and 0b1011010101 not in VARICODE
    assert set(text) == set(VARICODE.values())
    one.feed([[1, 0, 1]]); one.reset()
    assert one.feed([[1, 1, 0, 0]])[0] == "e"
