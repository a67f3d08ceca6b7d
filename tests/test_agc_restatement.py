"""tests/agc_restatement.py against the g20_agc_* fixtures (tools/golden_agc: cut from the unmodified reference AGC<int16_t> and
AGC<float>): every output sample of every stream in its recorded call split, the setter calls between buffers included, and
the node's gain, sd and enabled flag after every buffer. Bit for bit; float rows except where both sides are NaN, and only the
silence streams may hold a NaN at all. The designers give the recorded lambda and target bits."""
import numpy as np
import pytest

import agc_restatement as R

MAN = R.manifest()
NAMES = sorted(MAN)


def test_the_fixture_set_is_what_the_issue_lists():
    assert len(NAMES) == 8 and all(n.startswith("g20_agc_") for n in NAMES)
    for t in ("i16", "f32"):
        for k in ("default", "target", "ops", "silence"):
            assert "g20_agc_%s_%s" % (t, k) in MAN
    assert {MAN[n]["Fs"] for n in NAMES} >= {22050.0, 48000.0, 8000.0}
    for n in NAMES:
        m, x, y = R.load(n, MAN)
        assert x.nbytes <= 96 * 1024 and sum(m["lens"]) == x.size
    # the silence streams: tau 0.001 at 8000 Hz, at least 1200 zeros in a row with a non-zero sample inside the silence
    for t in ("i16", "f32"):
        m, x, _ = R.load("g20_agc_%s_silence" % t, MAN)
        assert m["tau"] == 0.001 and m["Fs"] == 8000.0
        z = np.flatnonzero(x[300:1700])
        assert z.size == 1 and (1400 - 1 - z[0]) >= 1200


@pytest.mark.parametrize("name", NAMES)
def test_designers_give_the_recorded_bits(name):
    m = MAN[name]
    dt = np.int16 if m["dtype"] == "i16" else np.float32
    assert R.design_lambda(m["tau"], m["Fs"]).view(np.uint32) == m["lambda_bits"]
    want = np.float32(m["target"]) if m["target"] else R.design_target(dt)
    assert want.view(np.uint32) == m["target_bits"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    m, x, y = R.load(name, MAN)
    node = R.Bank(x.dtype, R.design_lambda(m["tau"], m["Fs"]), m["target"])
    got = np.empty_like(y)
    for b, (off, n) in enumerate(R.buffers(m)):
        R.apply_ops(node, 0, m, b)
        got[off:off + n] = node.process(x[off:off + n])[0]
        g, s, e = m["state_bits"][b]
        assert (node.gain.view(np.uint32)[0], node.sd.view(np.uint32)[0], int(node.enabled[0])) == (g, s, e), (name, b)
    assert R.same(got, y), (name, int(np.flatnonzero(got.view(np.uint8) != y.view(np.uint8))[0]))
    if x.dtype == np.float32:
        nan = int(np.isnan(got).sum())
        assert (nan > 0) == name.endswith("silence"), (name, nan)   # the NaN rule can hide nothing outside the silence case
        assert np.array_equal(np.isnan(got), np.isnan(y))


def test_the_fixtures_hold_the_traps():
    """int16 wraps after a quiet stretch, pass-through and held-gain buffers, +inf gain behind a denormal sd."""
    m, x, y = R.load("g20_agc_i16_default", MAN)
    node = R.Bank(np.int16, R.design_lambda(m["tau"], m["Fs"]))
    products = []   # gain * x sample by sample: a wrap is a product outside int16's range
    for v in x[:4400]:
        node.process(np.array([v], np.int16))
        products.append(float(node.gain[0]) * float(v))
    assert sum(abs(p) >= 32768 for p in products) > 50
    m, x, y = R.load("g20_agc_f32_silence", MAN)
    g, s, e = m["state_bits"][1]
    assert R.bits_f32(g) == np.inf and 0 < R.bits_f32(s) < np.finfo(np.float32).tiny
    m, x, y = R.load("g20_agc_i16_silence", MAN)
    assert np.all(y[1000:1500] == 0)
    m, x, y = R.load("g20_agc_i16_ops", MAN)
    (o3, n3), (o7, n7) = R.buffers(m)[3], R.buffers(m)[7]
    assert np.array_equal(y[o3:o3 + n3], x[o3:o3 + n3]) and np.array_equal(y[o7:o7 + n7], x[o7:o7 + n7])
