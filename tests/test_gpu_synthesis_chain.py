"""Synthesis -> analysis on the device: three channel rows (tests/synthesis_restatement.py's chain_case: M = 16, D = 8, a
128-tap prototype h, the synthesis bank's taps D h) go through Synthesis.process_dev onto one wideband row and from there through
Channelizer.process_dev (cf32, the same M, D and h) back to 16 channel rows, nothing leaving the device in between. Behind column
40 the analysis rows of the three channels equal the inputs delayed by 15 columns, within 1e-2 of each row's amplitude, and every
other channel's mean power is at least 60 dB under the strongest channel's. The restatements alone hold both conditions
(tests/test_synthesis_restatement.py: 5.3e-3 and -65.4 dB)."""
import numpy as np
import pytest

import synthesis_restatement as R

pytestmark = pytest.mark.gpu


def test_synthesis_into_a_channelizer_returns_the_rows():
    import libsdr_amd as sa
    k = R.chain_case()
    M, D, x = k["M"], k["D"], k["x"]
    rows, n = x.shape[0], x.shape[1]
    ctx = sa.Context(0)
    syn = sa.Synthesis(ctx, M, D, D * k["h"], channels=k["channels"], max_in=n)
    ana = sa.Channelizer(ctx, np.float32, M, D, k["h"], max_in=n * D)
    y = np.zeros((M, n, 2), np.float32)
    d_in, d_wide, d_out = ctx.malloc(x.nbytes), ctx.malloc(n * D * 8), ctx.malloc(y.nbytes)
    try:
        ctx.h2d(d_in, x)
        assert syn.process_dev(d_in, n, 0, d_wide) == n * D
        assert ana.process_dev(d_wide, n * D, d_out, n) == n
        ctx.synchronize()
        ctx.d2h(y, d_out)
    finally:
        for p in (d_in, d_wide, d_out):
            ctx.free(p)
    err, db = R.chain_margins(k, R.rows_of(y))
    print("chain on the device: row error %.3g of the amplitude, strongest other channel %.1f dB" % (err, db))
    assert err <= 1e-2 and db <= -60.0, (err, db)
    assert rows == 3 and syn.get_state()["consumed"] == n and ana.get_state()["consumed"] == n * D
    for o in (syn, ana, ctx):
        o.close()
