"""Random plans and call sequences of the tuner bank (sdrhip_tuner_i16_*) against the compiled CPU oracle, bit for bit, inside the
red-zoned device arena. Half the plans can run the matrix kernel (tuner_i16_mfma_kernel), a random one of them with a forced
SDRHIP_TUNER_CTW; between calls channels are retuned and the bank is reset with every flag combination. Every call's
plan_info is held to the model of tests/tuner_classes.py. Run with `pytest -m gpu` on an MI355X."""
import os

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
from redzone import RedZone
from test_gpu_parity_tuner import EPIS, FS, HOT, VALU, Ref, make_bank, tune

pytestmark = pytest.mark.gpu
EXTRA = int(os.environ.get("SDRHIP_FUZZ_EXTRA", "0"))


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def draw_plan(rng, hot):
    plan = dict(C=int(rng.integers(1, 301)), order=int(rng.choice([1, 2, 15, 16, 17, 33, 127, 128, 129, 513, int(rng.integers(1, 514))])),
                epi=str(rng.choice(tc.EPI_NAMES)), cu8=bool(rng.integers(0, 2)), max_in=int(rng.integers(2000, 20001)),
                ctw=[None, None, 1, 2, 4, 8][int(rng.integers(0, 6))], misfit=False)
    if hot:
        plan["D"] = int(rng.choice([4, 5, 7, 8, 12, 20, 64, 125, 256, 257, 300, 512, int(rng.integers(4, 513))]))
    else:   # the plain kernel: a small decimation, one channel's taps beyond the byte planes, or calls too short
        why = int(rng.integers(0, 4))
        plan["D"] = int(rng.integers(1, 4)) if why < 2 else int(rng.integers(4, 513))
        plan["misfit"] = why == 2
        if why == 3:
            plan["max_in"] = int(rng.integers(100, 512))
    return plan


def draw_tune(rng, order):
    Fc = float(rng.integers(-1100, 1100)) * 1e3 + 500.0
    return tune(Fc, Fc, float(rng.integers(8, 200)) * 1e3, order)


def draw_length(rng, plan):
    m, kind = plan["max_in"], int(rng.integers(0, 9))
    n = [0, 1, int(rng.integers(1, plan["order"] + 1)), int(rng.integers(1, plan["D"] + 1)), int(rng.integers(500, 512)),
         int(rng.integers(512, 530)), m, m, int(rng.integers(0, m + 1))][kind]
    return min(n, m)


@pytest.mark.parametrize("seed", range(12 + EXTRA))
def test_tuner_random_plans(ctx, orc, seed, monkeypatch):
    rng = np.random.default_rng(7100 + seed)
    plan = draw_plan(rng, hot=seed % 2 == 0)   # half the plans can run the matrix kernel
    C, order, D, epi, cu8 = plan["C"], plan["order"], plan["D"], EPIS[plan["epi"]], plan["cu8"]
    fm = plan["epi"] == "fm"
    tunes = [draw_tune(rng, order) for _ in range(C)]
    bad = int(rng.integers(0, C))
    if plan["misfit"]:
        k = np.asarray(tunes[bad][0], np.int32).reshape(-1, 2).copy()
        k[int(rng.integers(0, order)), int(rng.integers(0, 2))] = 32700
        tunes[bad] = (k,) + tuple(tunes[bad][1:])
    monkeypatch.delenv("SDRHIP_TUNER_PATH", raising=False)
    monkeypatch.delenv("SDRHIP_TUNER_CTW", raising=False)
    if plan["ctw"] is not None:
        monkeypatch.setenv("SDRHIP_TUNER_CTW", str(plan["ctw"]))
    bank, lut = make_bank(ctx, tunes, D, epi, plan["max_in"], cu8=cu8)
    monkeypatch.delenv("SDRHIP_TUNER_CTW", raising=False)
    if C <= 48:
        rows = list(range(C))
    else:
        rows = sorted(set(int(r) for r in rng.choice(C, 24, replace=False)) | {e for ct in range(tc.ceil_div(C, tc.CT)) for e in tc.tile_edges(C, ct)})
    new_ref = lambda c: Ref(orc, tunes[c][0], lut, tunes[c][1], tunes[c][2], D, epi)
    refs = {c: new_ref(c) for c in rows}
    sig = orc.IQSigGen(FS, [(100e3, 8000, 0.0), (-300e3, 6000, 0.3), (210e3, 9000, 1.0)])
    full_scale = bool(rng.integers(0, 2))
    n0, hot_plan = 0, D >= tc.HOT_MIN_D and not plan["misfit"]
    before, guarded = RedZone.calls, 0
    for call in range(int(rng.integers(8, 13))):
        where = "seed %d plan %s call %d" % (seed, plan, call)
        act = int(rng.integers(0, 8)) if call else 7
        c = int(rng.integers(0, C))
        if act == 0:
            t = draw_tune(rng, order)
            bank.set_shift(c, t[1], t[2])
            tunes[c] = (tunes[c][0], t[1], t[2])
            if c in refs:
                refs[c].bb.set_shift(t[1], t[2])
        elif act == 1 and not (plan["misfit"] and c == bad):
            t = draw_tune(rng, order)
            bank.set_taps(c, t[0])
            tunes[c] = (t[0],) + tuple(tunes[c][1:])
            if c in refs:
                refs[c].bb.set_taps(t[0])
        elif act == 2:
            flags = int(rng.integers(0, 4))
            bank.reset(keep_history=bool(flags & 1), keep_fm=bool(flags & 2))
            for r, ref in refs.items():
                old_fm = ref.fm
                if flags & 1:
                    ref.bb.reset()
                else:
                    refs[r] = ref = new_ref(r)       # a freshly constructed node with the channel's current tune
                ref.fm = old_fm if flags & 2 else orc.FMDemodI16()
            n0 = 0
        n = draw_length(rng, plan)
        if cu8:
            x = rng.integers(0, 256, (n, 2)).astype(np.uint8) if full_scale else ((sig.next_cs16(n) >> 8) + 128 + rng.integers(-9, 9, (n, 2))).astype(np.uint8)
            xo = orc.autocast_cu8_cs16(x)
        else:
            x = rng.integers(-32768, 32768, (n, 2)).astype(np.int16) if full_scale else (sig.next_cs16(n).astype(np.int32) + rng.integers(-3000, 3000, (n, 2))).astype(np.int16)
            xo = x
        if n:
            want = tc.model(C, order, D, fm, n0, n, hot_plan=hot_plan, force_ctw=plan["ctw"])
            info = bank.plan_info(n)
            assert info == want, (where, n, info, want)
        y = bank.process(x)
        guarded += 1 if n and y.shape[1] else 0
        if n:
            assert bank.kernel_names == ([HOT] if want["hot"] else [VALU]), where
        assert y.shape[0] == C, where
        for r in rows:
            if not np.array_equal(y[r], refs[r].process(xo)):
                raise AssertionError("%s: row %d of a call of %d samples from index %d differs from the oracle" % (where, r, n, n0))
        n0 += n
    assert RedZone.active and RedZone.calls == before + guarded
