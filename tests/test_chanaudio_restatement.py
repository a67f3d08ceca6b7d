"""tests/chanaudio_restatement.py held to the oracle: its vectorised fast_atan2 against the oracle's fast_atan2_i16 (the golden
triples and a sweep), its three demodulators against the oracle's cs16 FM / AM / USB on random cs16 rows cut into calls, the
per-call FM convention with calls of 0, 1 and 2 outputs, and the rounding edges of the conversion."""
import numpy as np

import chanaudio_restatement as A

INF, NAN = np.float32("inf"), np.float32("nan")


def test_fast_atan2_against_the_oracle(golden, orc):
    t = golden.load("g8_fast_atan2_triples").reshape(-1, 3).astype(np.int64)
    assert np.array_equal(A.fast_atan2(t[:, 0], t[:, 1]), t[:, 2])
    rng = np.random.default_rng(5)
    ab = np.concatenate([rng.integers(-32768, 32768, (3000, 2)), rng.integers(-5, 6, (300, 2)),
                         [(0, 0), (-32768, -32768), (32767, -32768), (-32768, 32767), (-32768, 0), (0, -32768), (0, 32767), (1, -1)]])
    want = np.array([orc.fast_atan2_i16(a, b) for a, b in ab.tolist()])
    assert np.array_equal(A.fast_atan2(ab[:, 0], ab[:, 1]), want)


def _rows(seed, n):
    rng = np.random.default_rng(seed)
    q = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    q[3], q[4], q[5], q[n - 1] = (0, 0), (-32768, -32768), (32767, -32768), (-32768, 32767)
    return q


def test_am_and_usb_against_the_oracle(orc):
    q = _rows(11, 5000)
    assert np.array_equal(A.am(q), orc.am_i16(q)) and np.array_equal(A.usb(q), orc.usb_i16(q))
    r = A.Rows([A.AM, A.USB])
    y = np.stack([q, q]).astype(np.float32)            # gain 1 on integers: the conversion is the identity
    assert np.array_equal(r.process(y), np.stack([orc.am_i16(q), orc.usb_i16(q)])) and r.last == [0, 0]


def test_fm_per_call_convention_against_the_oracle(orc):
    q = _rows(12, 4000)
    lens = [0, 1, 2, 1, 1, 0, 2, 3, 500, 1, 2, 7]
    lens.append(len(q) - sum(lens))
    r, ref, off = A.Rows([A.FM]), orc.FMDemodI16(), 0
    for n in lens:
        part = q[off:off + n]
        before = r.last[0]
        got = r.process(part[None].astype(np.float32))
        assert got.shape == (1, n) and np.array_equal(got[0], ref.process(part, inplace=True)), (off, n)
        assert r.last[0] == int(ref.last[0])
        if n <= 1:
            assert r.last[0] == before                 # a call's sample 0 never touches last
        if n == 1:
            assert got[0, 0] == part[0, 0]
        if n >= 2:
            assert r.last[0] == int(A.phi(part[-1])) and got[0, 0] == part[0, 0]
            assert got[0, 1] == np.int16(before - int(A.phi(part[1])))
        off += n
    # set_mode restarts the row, reset all rows; a gain keeps last
    r.set_gain(0, 0.5)
    assert r.last[0] != 0
    r.set_mode(0, A.FM)
    assert r.last == [0]
    r.process(q[None, :9].astype(np.float32))
    r.reset()
    assert r.last == [0]


def test_rows_select_state_by_row():
    q = _rows(13, 40).astype(np.float32)
    a, b = A.Rows([A.FM, A.AM, A.FM]), A.Rows([A.FM, A.AM, A.FM])
    full = a.process(np.stack([q, q, q[::-1]]))
    part = b.process(np.stack([q[::-1], q]), rows=[2, 0])
    assert np.array_equal(part, full[[2, 0]]) and b.last == [a.last[0], 0, a.last[2]]


def test_conversion_edges():
    y = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, 32766.5, 32767.5, -32767.5, -32768.5, 32767.0, -32768.0, 1e9, -1e9,
                  INF, -INF, NAN, -NAN], np.float32)
    want = [0, 0, 2, -2, 2, -2, 0, 32766, 32767, -32768, -32768, 32767, -32768, 32767, -32768, 32767, -32768, 0, 0]
    got = A.convert(y, 1.0)
    assert got.dtype == np.int16 and got.tolist() == want
    # the gain is ONE float32 multiply before the rounding: 3 * 0.5 = 1.5 -> 2, 0.1f * 5 = 0.5 (rounded product) -> 0
    assert A.convert(np.array([0.5, 2.5, 10922.5], np.float32), 3.0).tolist() == [2, 8, 32767]
    assert A.convert(np.array([5.0], np.float32), 0.1).tolist() == [int(np.rint(np.float32(0.1) * np.float32(5.0)))]
    assert A.convert(np.array([INF, -INF, NAN, 1.0], np.float32), 0.0).tolist() == [0, 0, 0, 0]      # inf * 0 = NaN -> 0
    assert A.convert(np.array([INF, 3.0], np.float32), -1.0).tolist() == [-32768, -3]
    assert A.convert(np.array([3e38], np.float32), 10.0).tolist() == [32767]                          # overflow to +inf
