"""GPU parity of every compiled instance of the time-domain FIR kernels (tests/fir_classes.py: fir_cs16_exact_kernel<WRAP,R2>,
fir_cf32_rt_kernel<R,DC>, fir_cf32_pipe_kernel<R,8>, tile_phasor_kernel, hist_roll_cf32), reached through sa.FIR and
sa.FloatBaseBand. Per case, over three calls of ragged lengths with the history carried: after every call last_kernels() must
be exactly what the case names — a case that lands on another instance FAILS. The float kinds: every channel is held to a
float64 restatement of the chain (shift, FIR, D-sample mean, demodulator), on white noise and on an impulse train that puts
a single folded tap on every output around a tile seam, within the project's contract (RTOL of tests/test_gpu_parity.py, of
each channel's largest reference magnitude). The exact kind: bit for bit against the oracle's FIRFilter<complex<int16>>
(+ FMDemod) with its state carried, on full-scale noise and on the rows that drive every partial sum of the per-tap loop to
its bound. Where the code promises identical bits (the pipelined form and the one-tile-per-workgroup kernel) they are
compared too. The module runs inside the red-zoned device arena (tests/redzone.py), rows on every alignment. Run with
`pytest -m gpu` on an MI355X; `-s` prints the kernels the device reported and every error figure."""
import numpy as np
import pytest

import libsdr_amd as sa

try:   # torch brings its own HIP runtime: it only finds the GPU when it initialises before libsdrhip.so does
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()
except Exception:   # pragma: no cover
    torch = None

import fir_classes as fc
from redzone import RedZone
from test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in fc.ENV_HOOKS:
        monkeypatch.delenv(k, raising=False)


def set_hooks(monkeypatch, env):
    """The library reads its hooks when a plan is made and again at every launch: exactly `env` is set."""
    for k in fc.ENV_HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in fc.ENV_HOOKS, k
        monkeypatch.setenv(k, v)


def make_node(ctx, case, alpha):
    assert (sa.EPI_NONE, sa.EPI_FM, sa.EPI_AM, sa.EPI_USB) == (fc.EPI_NONE, fc.EPI_FM, fc.EPI_AM, fc.EPI_USB)
    if case.kind == "fbb":
        return sa.FloatBaseBand(ctx, case.fc, fc.FS, alpha, case.decim, channels=case.C, max_in=case.max_in)
    kind = sa.FIR_CS16_EXACT if case.kind == "exact" else sa.FIR_CF32
    return sa.FIR(ctx, kind, alpha, decim=case.decim, channels=case.C, max_in=case.max_in, epilogue=case.epi)


def run(node, chunk, n_out):
    """One call: through the arena whenever it has output (a call that completes none has no output rows to guard and goes
    through the host-pointer entry point) -> [C, n_out(, 2)]."""
    before = RedZone.calls
    y = node.process(chunk)
    assert RedZone.active and RedZone.calls == before + (1 if n_out else 0)
    assert y.shape[:2] == (chunk.shape[0], n_out)
    return y


def run_case(ctx, case, monkeypatch, judge):
    """The three calls of `case` on both inputs, the kernel record of every call (and of the twin's) held to the table; judge(what,
    x, k, off, chunk, y) sees every call's output; -> {input: [C, sum n_out(, 2)]}."""
    monkeypatch.setattr(RedZone, "band", case.band)
    alpha = fc.case_taps(case)
    assert alpha.shape == (case.order,)
    set_hooks(monkeypatch, case.env)
    node = make_node(ctx, case, alpha)
    assert node.last_kernels() == []                                   # nothing launched yet
    twin = None
    if case.twin_expect is not None:
        set_hooks(monkeypatch, case.twin_env)
        twin = make_node(ctx, case, alpha)
    n_outs = fc.out_lens(case)
    got = {}
    for what, x in fc.case_inputs(case):
        for nd in (node, twin):
            if nd is not None:
                nd.reset()
                if case.retune:
                    nd.set_shift(case.fc)                              # (the frequency the case starts on, phasor restarted at sample 0)
        outs, off = [], 0
        for k, n in enumerate(case.lens):
            chunk = np.ascontiguousarray(x[:, off:off + n])
            if case.retune and case.retune[0] == k:
                node.set_shift(case.retune[1])
                if twin is not None:
                    twin.set_shift(case.retune[1])
            set_hooks(monkeypatch, case.env)
            y = run(node, chunk, n_outs[k])
            ran = node.last_kernels()
            print("FIR_CLASS case=%s input=%s call=%d n_in=%d kernels=%s" % (case.id, what, k, n, ran))
            assert ran == case.expect[k], (case.id, what, "call", k, ran, case.expect[k])
            if twin is not None:
                set_hooks(monkeypatch, case.twin_env)
                yt = run(twin, chunk, n_outs[k])
                assert twin.last_kernels() == case.twin_expect[k], (case.id, what, "call", k, twin.last_kernels(), case.twin_expect[k])
                assert np.array_equal(y, yt), (case.id, what, "call", k, "differs from the same plan under", case.twin_env)
            judge(what, x, k, off, chunk, y)
            outs.append(y)
            off += n
        got[what] = np.concatenate(outs, axis=1)
    # a call of 0 samples launches nothing, and says so
    set_hooks(monkeypatch, case.env)
    node.process(x[:, :0])
    assert node.last_kernels() == []
    return got


@pytest.mark.parametrize("case", [c for c in fc.cases() if c.kind != "exact"], ids=lambda c: c.id)
def test_fir_class_float_case(ctx, case, monkeypatch):
    tol = case.rtol if case.rtol is not None else RTOL
    alpha = fc.case_taps(case)
    inputs = dict(fc.case_inputs(case))
    got = run_case(ctx, case, monkeypatch, lambda *a: None)
    rows = list(range(case.C)) if case.rows is None else case.rows
    worst = {}
    for what, y in got.items():
        for c in rows:
            ref = fc.reference(case, inputs[what][c], alpha)
            out = fc.as_float64(case, y[c])
            assert out.shape == ref.shape
            scale = np.abs(ref).max()
            assert scale > 0
            worst[(what, c)] = np.abs(out - ref).max() / scale
        print("FIR_CLASS case=%s input=%s worst_rel_err=%.3e tol=%.1e" % (case.id, what, max(v for k, v in worst.items() if k[0] == what), tol))
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, (case.id, "relative error above %g (input, channel)" % tol, bad)
    assert len(worst) == 2 * len(rows)


@pytest.mark.parametrize("case", [c for c in fc.cases() if c.kind == "exact"], ids=lambda c: c.id)
def test_fir_class_exact_case(ctx, orc, case, monkeypatch):
    alpha = fc.case_taps(case)
    rows = list(range(case.C)) if case.rows is None else case.rows
    refs, differ = {}, []

    def judge(what, x, k, off, chunk, y):
        if k == 0:                                                     # a new input: the oracle starts afresh, as reset() does
            for c in rows:
                refs[c] = (orc.FIR(alpha), orc.FMDemodI16())
        for c in rows:
            f, fm = refs[c]
            ref = f.process_cs16(chunk[c])
            if case.epi == fc.EPI_FM:
                ref = fm.process(ref)
            if not np.array_equal(y[c], ref):
                differ.append((what, "call", k, "channel", c, int(np.count_nonzero(np.any((y[c] != ref).reshape(len(ref), -1), axis=1)))))

    run_case(ctx, case, monkeypatch, judge)
    print("FIR_CLASS case=%s rows=%s differing (input, call, channel, outputs): %s" % (case.id, rows, differ or "none"))
    assert not differ, (case.id, differ)


@pytest.mark.parametrize("r2", [4, 8])
def test_wrap_decision_follows_set_taps(ctx, orc, r2):
    """The wrap decision is taken again whenever the taps change: a plan made on the threshold filter (no partial sum can
    leave int16: the instance without the per-tap wrap) must run the wrapping instance after set_taps to the filter just above
    the threshold, and the other one again after going back — on the same handle, the history carried, bit for bit against
    the oracle on the adversarial rows."""
    case = next(c for c in fc.cases() if c.taps == "lowpass@threshold" and c.epi == fc.EPI_NONE and (c.C == 64) == (r2 == 8))
    C, max_in = case.C, case.max_in                                    # (64 channels of 65536 samples: the plan that takes R2 = 8)
    below, above = fc.threshold_taps(case.order, 32767.5), fc.threshold_taps(case.order, 32768.5)
    x = dict(fc.case_inputs(case))["adversarial"]
    n = case.lens[0]
    node = sa.FIR(ctx, sa.FIR_CS16_EXACT, below, channels=C, max_in=max_in)
    rows = sorted({0, 1, C - 1})
    oracles = {c: (orc.FIR(below), orc.FIR(above)) for c in rows}       # both rings see every sample; the taps in force judge
    for k, (taps, wrap) in enumerate([(below, 0), (above, 1), (below, 0)]):
        if k:
            node.set_taps(taps)
        chunk = np.ascontiguousarray(x[:, :n] if k != 1 else fc.mirrored(x[:, :n]))      # (the middle call on the mirrored rows)
        y = node.process(chunk)
        assert node.last_kernels() == [fc.exact(wrap, r2)], (k, node.last_kernels())
        for c in rows:
            both = [o.process_cs16(chunk[c]) for o in oracles[c]]
            assert np.array_equal(y[c], both[wrap]), (k, c)
