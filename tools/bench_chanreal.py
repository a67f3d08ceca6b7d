"""Device-resident timing of the channelizer family on a REAL row (include/sdrhip_chanreal.h) beside what a user could run
before it: the complex cs16 node on the same samples widened to (x, 0) on the device (not timed), rows 0 ... M / 2 selected.
s16 input, n = 2^21 real samples per call — the bytes of the family's 2^20 cs16. Shapes M = 1024 with 8192 taps at D = 1024 and
D = 512, and M = 128 with 512 taps at D = 128, for Channelizer; AudioChannelizer (all FM) and ChannelPower at M = 1024, D = 1024.
Candidates are INTERLEAVED round by round: every round times each once, HIP events over `reps` calls after a warm-up; the median
and the range of the rounds are reported, and (a) real over (b) widened. Before the timing, parity_max_rel_err is measured: the
real Channelizer's one call on every shape and input of tests/test_gpu_parity_chanreal.py against the float64 restatement
(tests/chanreal_restatement.py), max |y - folded_real| / max |folded_real| per case and the maximum over them. Writes
profiles/chanreal_bench.json; the key family_parent_vs_this is kept from the file that is there (tools/bench_chanreal_family.py
writes it).
usage: python tools/bench_chanreal.py [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchkit import timed_interleaved  # noqa: E402

import libsdr_amd as sa

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "chanreal_bench.json")
N, FS = 1 << 21, 2.048e6
# name -> (M, D, n_taps)
SHAPES = {"m1024_d1024": (1024, 1024, 8192), "m1024_d512": (1024, 512, 8192), "m128_d128": (128, 128, 512)}
NODES_AT = "m1024_d1024"   # the shape of the audio and power candidates
KEPT = ("family_parent_vs_this",)


def parity(ctx):
    """{case: error} over the parity test's shapes and input types, on its inputs; one call each"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import chanreal_restatement as RR
    import test_gpu_parity_chanreal as T
    errs = {}
    for shape in RR.SHAPES:
        for dtype in T.DTYPES:
            taps, x, _, ref = T._case(shape, dtype)
            node = sa.Channelizer(ctx, T.NP[dtype], shape[0], shape[1], taps, max_in=len(x), real=True)
            errs["%d-%d-%d-%s" % (shape + (dtype,))] = float("%.3g" % T._err(node.process(x), ref))
            node.close()
    return errs


def main():
    ctx = sa.Context(0)
    errs = parity(ctx)
    rng = np.random.default_rng(2048)
    x = rng.integers(-12000, 12000, N).astype(np.int16)
    wide = np.stack([x, np.zeros_like(x)], axis=1)
    nodes, cand, plans, kernels = [], {}, {}, {}
    din, dwide, dsum = ctx.malloc(x.nbytes), ctx.malloc(wide.nbytes), ctx.malloc(4096 * 8)
    dout = ctx.malloc(max((M // 2 + 1) * (N // D) for M, D, _ in SHAPES.values()) * 8)
    try:
        ctx.h2d(din, x)
        ctx.h2d(dwide, wide)
        for name, (M, D, n_taps) in SHAPES.items():
            taps = sa.design_fir_lowpass(n_taps, FS / (2 * M), FS)
            half = list(range(M // 2 + 1))
            real = sa.Channelizer(ctx, np.int16, M, D, taps, max_in=N, real=True)
            widened = sa.Channelizer(ctx, np.int16, M, D, taps, channels=half, max_in=N)
            nodes += [real, widened]
            plans[name] = {"real": real.plan_info(), "widened": widened.plan_info()}
            kernels[name] = real.kernel_names
            cand[name + "_channelizer_real"] = lambda v=real, s=N // D: v.process_dev(din, N, dout, s)
            cand[name + "_channelizer_widened"] = lambda v=widened, s=N // D: v.process_dev(dwide, N, dout, s)
        M, D, n_taps = SHAPES[NODES_AT]
        taps = sa.design_fir_lowpass(n_taps, FS / (2 * M), FS)
        half = list(range(M // 2 + 1))
        a_real = sa.AudioChannelizer(ctx, np.int16, M, D, taps, max_in=N, real=True)
        a_wide = sa.AudioChannelizer(ctx, np.int16, M, D, taps, channels=half, max_in=N)
        p_real = sa.ChannelPower(ctx, np.int16, M, D, taps, alpha=0.25, max_in=N, real=True)
        p_wide = sa.ChannelPower(ctx, np.int16, M, D, taps, alpha=0.25, max_in=N)    # (the monitor has no selection: all M sums)
        nodes += [a_real, a_wide, p_real, p_wide]
        kernels["audio"], kernels["power"] = a_real.kernel_names, p_real.kernel_names
        plans["audio"], plans["power"] = {"real": a_real.plan_info(), "widened": a_wide.plan_info()}, {"real": p_real.plan_info(), "widened": p_wide.plan_info()}
        cand[NODES_AT + "_audio_real"] = lambda: a_real.process_dev(din, N, dout, N // D)
        cand[NODES_AT + "_audio_widened"] = lambda: a_wide.process_dev(dwide, N, dout, N // D)
        cand[NODES_AT + "_power_real"] = lambda: p_real.process_dev(din, N, dsum)
        cand[NODES_AT + "_power_widened"] = lambda: p_wide.process_dev(dwide, N, dsum)
        stages = timed_interleaved(ctx, cand, REPS, ROUNDS)
        ctx.synchronize()
        ratios = {}
        for k in stages:
            if k.endswith("_real"):
                a, b = stages[k], stages[k[:-5] + "_widened"]
                ratios[k[:-5]] = {"real_over_widened": round(a["ms"] / b["ms"], 3), "real_below_widened_range": a["max_ms"] < b["min_ms"]}
        result = {"device": ctx.device_name(), "real_samples_per_call": N, "reps": REPS, "rounds": ROUNDS,
                  "shapes": {k: dict(zip(("M", "D", "n_taps"), v)) for k, v in SHAPES.items()}, "plans": plans, "stages": stages,
                  "ratios": ratios, "kernels": kernels, "parity_max_rel_err": max(errs.values()), "parity_rel_err": errs,
                  "parity_bound": 1e-5}
    finally:
        for p in (din, dwide, dsum, dout):
            ctx.free(p)
    for v in nodes:
        v.close()
    ctx.close()
    if os.path.exists(OUT):
        with open(OUT) as f:
            old = json.load(f)
        result.update({k: old[k] for k in KEPT if k in old})
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
