"""GPU parity of the tuner bank's matrix kernel (tuner_i16_mfma_kernel) in every plan class of tests/tuner_classes.py: the
channel tiles a workgroup walks (1, 2, 4, 8; a ragged last workgroup; a partial last tile behind other tiles), the tile
geometries of the decimations over calls of >= 100 time tiles, the K-step counts, the LDS maximum, and all eight (epilogue,
input kind) instances. Per case: plan_info of every call equals the model field for field, the rows tuner_classes.oracle_rows
names are held to the compiled CPU oracle, every other row is compared with the same bank under SDRHIP_TUNER_PATH=valu (which
only localises a fault: the oracle is the reference). Everything is np.array_equal; the module runs inside the red-zoned
device arena (tests/redzone.py). Run with `pytest -m gpu` on an MI355X; `-s` prints the plan_info the device reported."""
import numpy as np
import pytest

import libsdr_amd as sa

try:   # torch brings its own HIP runtime: it only finds the GPU when it initialises before libsdrhip.so does
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()
except Exception:   # pragma: no cover
    torch = None

import tuner_classes as tc
from hot_classes import BOUNDARY, PLANE_LIMIT
from redzone import RedZone
from test_gpu_parity_tuner import EPIS, FS, HOT, VALU, Ref, bank_tunes, make_bank, split, tune

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("SDRHIP_TUNER_PATH", raising=False)
    monkeypatch.delenv("SDRHIP_TUNER_CTW", raising=False)


def case_seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id))


def case_input(orc, case, n):
    """(what the bank is fed, the same as cs16 for the oracle)."""
    rng = np.random.default_rng(case_seed(case))
    if case.data == "full":
        x = rng.integers(0, 256, (n, 2)).astype(np.uint8) if case.cu8 else rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    else:
        x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3), (210e3, 9000, 1.0), (700e3, 5000, 2.0)]).next_cs16(n)
        x = (x.astype(np.int32) + rng.integers(-3000, 3000, x.shape)).astype(np.int16)
        if case.cu8:
            x = ((x >> 8) + 128).astype(np.uint8)
    return x, (orc.autocast_cu8_cs16(x) if case.cu8 else x)


def case_tunes(case):
    if case.taps == "design":
        return bank_tunes(case.C, case.order, seed=case_seed(case))
    rng = np.random.default_rng(case_seed(case))
    taps = np.asarray(BOUNDARY, np.int32)[rng.integers(0, len(BOUNDARY), (case.C, case.order, 2))]
    taps[2, :, 0] = PLANE_LIMIT; taps[2, :, 1] = -PLANE_LIMIT          # the planes' limit on every tap: the int32 sums wrap
    incs = rng.integers(0, 8192, case.C)
    incs[1] = 0
    return [(taps[c], int(incs[c]), bool(c & 1)) for c in range(case.C)]


def make_pair(ctx, monkeypatch, tunes, D, epi, max_in, cu8, force_ctw=None):
    """(the bank as the case asks for it, the same bank on the plain kernel, the LUT)."""
    if force_ctw is not None:
        monkeypatch.setenv("SDRHIP_TUNER_CTW", str(force_ctw))
    bank, lut = make_bank(ctx, tunes, D, epi, max_in, cu8=cu8)
    monkeypatch.setenv("SDRHIP_TUNER_PATH", "valu")
    plain, _ = make_bank(ctx, tunes, D, epi, max_in, cu8=cu8)
    monkeypatch.delenv("SDRHIP_TUNER_PATH")
    monkeypatch.delenv("SDRHIP_TUNER_CTW", raising=False)
    return bank, plain, lut


def assert_rows_equal(y, yp, rows, what):
    """Rows `rows` of y and yp bit for bit; the message names the first row that differs."""
    if not np.array_equal(y[rows], yp[rows]):
        bad = [int(c) for c in rows if not np.array_equal(y[c], yp[c])]
        raise AssertionError("%s: %d rows differ from the plain kernel's, first %s" % (what, len(bad), bad[:8]))


@pytest.mark.parametrize("case", tc.cases(), ids=lambda c: c.id)
def test_tuner_class_case(ctx, orc, case, monkeypatch):
    lens = tc.call_lengths(case)
    x, xo = case_input(orc, case, sum(lens))
    tunes = case_tunes(case)
    epi = EPIS[case.epi]
    bank, plain, lut = make_pair(ctx, monkeypatch, tunes, case.D, epi, case.N, case.cu8, case.force_ctw)
    rows = tc.oracle_rows(case)
    others = np.setdiff1d(np.arange(case.C), rows)
    refs = {c: Ref(orc, tunes[c][0], lut, tunes[c][1], tunes[c][2], case.D, epi) for c in rows}
    models = tc.case_models(case)
    assert bank.kernel_names == [HOT] and plain.kernel_names == [VALU]
    before = RedZone.calls
    for k, (chunk, chunk_o) in enumerate(zip(split(x, lens), split(xo, lens))):
        info = bank.plan_info(len(chunk))
        print("TUNER_CLASS case=%s call=%d n_in=%d plan_info=%s" % (case.id, k, len(chunk), info))
        assert info == models[k], (case.id, k, info, models[k])
        assert plain.plan_info(len(chunk))["hot"] == 0
        y, yp = bank.process(chunk), plain.process(chunk)
        assert bank.kernel_names == ([HOT] if models[k]["hot"] else [VALU]) and plain.kernel_names == [VALU]
        assert y.shape[0] == case.C and y.shape == yp.shape
        for c in rows:
            assert np.array_equal(y[c], refs[c].process(chunk_o)), (case.id, "call", k, "row", c)
        assert_rows_equal(y, yp, others, "%s call %d" % (case.id, k))
    assert len(rows) + len(others) == case.C                       # no row goes uncompared
    assert RedZone.active and RedZone.calls >= before + 2 * (len(lens) - 1)   # (a short call without outputs moves nothing)
    print("TUNER_CLASS case=%s classes=%s" % (case.id, sorted(tc.classes_of(case), key=repr)))


# ---- a forced ctw changes the grid and nothing else -----------------------------------------------------------------------------

FORCED_FROM = ["d64_o127_fm", "ctw2_partial_c250", "ctw4_raggedwg_c530", "ctw8_ragged_c1000"]   # natural ctw 1, 2, 4, 8


@pytest.mark.parametrize("cid", FORCED_FROM)
def test_forced_ctw_does_not_change_results(ctx, orc, cid, monkeypatch):
    case = {c.id: c for c in tc.cases()}[cid]
    lens = tc.call_lengths(case)
    x, _ = case_input(orc, case, sum(lens))
    tunes = case_tunes(case)
    natural = tc.case_models(case)[1]["ctw"]
    assert natural == tc.CTWS[FORCED_FROM.index(cid)]
    outs = {}
    for ctw in (None,) + tuple(v for v in tc.CTWS if v != natural):
        if ctw is not None:
            monkeypatch.setenv("SDRHIP_TUNER_CTW", str(ctw))
        bank, _ = make_bank(ctx, tunes, case.D, EPIS[case.epi], case.N, cu8=case.cu8)
        monkeypatch.delenv("SDRHIP_TUNER_CTW", raising=False)
        got, n0 = [], 0
        for n, chunk in zip(lens, split(x, lens)):
            want = tc.model(case.C, case.order, case.D, case.epi == "fm", n0, n, force_ctw=ctw)
            info = bank.plan_info(n)
            assert info == want and (ctw is None or not info["hot"] or info["ctw"] == ctw), (cid, ctw, info, want)
            got.append(bank.process(chunk))
            n0 += n
        assert bank.kernel_names == [HOT]
        outs[ctw or natural] = got
    assert sorted(outs) == list(tc.CTWS)
    for ctw in tc.CTWS:
        for k in range(len(lens)):
            assert np.array_equal(outs[ctw][k], outs[natural][k]), (cid, "ctw", ctw, "call", k)
    # values outside 1 | 2 | 4 | 8 are ignored
    for junk in ("3", "16", "", "2x", "08"):
        monkeypatch.setenv("SDRHIP_TUNER_CTW", junk)
        bank, _ = make_bank(ctx, tunes, case.D, EPIS[case.epi], case.N, cu8=case.cu8)
        monkeypatch.delenv("SDRHIP_TUNER_CTW")
        assert bank.plan_info(case.N) == tc.model(case.C, case.order, case.D, case.epi == "fm", 0, case.N), junk


# ---- retune mid-stream where workgroups walk two channel tiles ---------------------------------------------------------------------

def test_retune_midstream_ctw2(ctx, orc, monkeypatch):
    C, order, D, N = 250, 64, 8, 65536
    tunes = bank_tunes(C, order, seed=77)
    x = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3), (210e3, 9000, 1.0)]).next_cs16(333 + 5 * N)
    x = (x.astype(np.int32) + np.random.default_rng(78).integers(-3000, 3000, x.shape)).astype(np.int16)
    bank, plain, lut = make_pair(ctx, monkeypatch, tunes, D, sa.EPI_FM, N, False)
    # channel 37: tile 2, the first of workgroup 1; 60: tile 3, its last; 245: the partial tile 15 (10 channels) behind tile 14
    first, last, partial = 37, 60, 245
    rows = sorted({0} | {c + d for c in (first, last, partial) for d in (-1, 0, 1)} | {32, 47, 48, 63, 240, 249})
    refs = {c: Ref(orc, tunes[c][0], lut, tunes[c][1], tunes[c][2], D, sa.EPI_FM) for c in rows}
    others = np.setdiff1d(np.arange(C), rows)
    big = np.asarray(tunes[last][0], np.int32).reshape(-1, 2).copy()
    big[5, 0] = 32700                                          # a high byte plane of 128: no int8

    def both(f):
        f(bank); f(plain)

    n0 = 0
    for k, chunk in enumerate(split(x, [333, N, N, N, N, N])):
        hot_plan = True
        if k == 2:
            t = tune(-150e3, -150e3, 50e3, order)
            both(lambda b: b.set_shift(first, t[1], t[2])); refs[first].bb.set_shift(t[1], t[2])
            t = tune(0.0, 333e3, 30e3, order)
            both(lambda b: b.set_taps(partial, t[0])); refs[partial].bb.set_taps(t[0])
        if k == 3:
            t = tune(333e3, 333e3, 30e3, order)
            both(lambda b: (b.set_shift(last, t[1], t[2]), b.set_taps(last, t[0])))
            refs[last].bb.set_shift(t[1], t[2]); refs[last].bb.set_taps(t[0])
            both(lambda b: b.set_shift(partial, 0, False)); refs[partial].bb.set_shift(0, False)
            t2 = tune(0.0, -100e3, 20e3, order)
            both(lambda b: b.set_taps(first, t2[0])); refs[first].bb.set_taps(t2[0])
        if k == 4:   # one channel's taps misfit the planes: the whole bank runs the plain kernel and says so
            both(lambda b: b.set_taps(last, big)); refs[last].bb.set_taps(big)
            hot_plan = False
        if k == 5:
            t = tune(333e3, 333e3, 30e3, order)
            both(lambda b: b.set_taps(last, t[0])); refs[last].bb.set_taps(t[0])
        want = tc.model(C, order, D, True, n0, len(chunk), hot_plan=hot_plan)
        info = bank.plan_info(len(chunk))
        assert info == want, (k, info, want)
        if k >= 1:
            assert info["hot"] == int(hot_plan) and (not hot_plan or info["ctw"] == 2)
        y, yp = bank.process(chunk), plain.process(chunk)
        assert bank.kernel_names == ([HOT] if want["hot"] else [VALU])
        for c in rows:
            assert np.array_equal(y[c], refs[c].process(chunk)), ("call", k, "row", c)
        assert_rows_equal(y, yp, others, "call %d" % k)
        n0 += len(chunk)
