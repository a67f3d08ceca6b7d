"""Device-resident timing of the channel power monitor beside the plain channelizer on the SAME input in the SAME run.
cs16 input, n = 2^20 samples per call; shapes M = 1024 with 8192 taps at D = 1024 and D = 512, and M = 128 with 512 taps at
D = 128. Candidates per shape: the monitor (sums written), the monitor with no sums asked for (the state alone), the plain
channelizer writing all rows and the plain channelizer writing 64 rows. They are INTERLEAVED round by round: every round times each
once, HIP events over `reps` calls after a warm-up; the median and the range of the rounds are reported, and the monitor's ratio
to the two channelizers. Writes profiles/chanpower_bench.json.
usage: python tools/bench_chanpower.py [reps] [rounds] [out.json]"""
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
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "chanpower_bench.json")
N, FS, SEL = 1 << 20, 2.048e6, 64
# name -> (M, D, n_taps)
SHAPES = {"m1024_d1024": (1024, 1024, 8192), "m1024_d512": (1024, 512, 8192), "m128_d128": (128, 128, 512)}


def main():
    ctx = sa.Context(0)
    rng = np.random.default_rng(1024)
    x = rng.integers(-12000, 12000, (N, 2)).astype(np.int16)
    nodes, cand = {}, {}
    din, dsum = ctx.malloc(x.nbytes), ctx.malloc(4096 * 8)
    dout = ctx.malloc(max(M * (N // D) for M, D, _ in SHAPES.values()) * 8)
    try:
        ctx.h2d(din, x)
        for name, (M, D, n_taps) in SHAPES.items():
            taps = sa.design_fir_lowpass(n_taps, FS / (2 * M), FS)
            sel = [int(k) for k in rng.choice(M, SEL, replace=False)]
            mon = sa.ChannelPower(ctx, np.int16, M, D, taps, alpha=0.25, max_in=N)
            every = sa.Channelizer(ctx, np.int16, M, D, taps, max_in=N)
            some = sa.Channelizer(ctx, np.int16, M, D, taps, channels=sel, max_in=N)
            nodes[name] = (mon, every, some)
            cand[name + "_monitor"] = lambda mon=mon: mon.process_dev(din, N, dsum)
            cand[name + "_monitor_state_only"] = lambda mon=mon: mon.process_dev(din, N)
            cand[name + "_channelizer_all"] = lambda v=every, s=N // D: v.process_dev(din, N, dout, s)
            cand[name + "_channelizer_sel64"] = lambda v=some, s=N // D: v.process_dev(din, N, dout, s)
        stages = timed_interleaved(ctx, cand, REPS, ROUNDS)
        ctx.synchronize()
        ratios = {}
        for name in SHAPES:
            m = stages[name + "_monitor"]["ms"]
            ratios[name] = {"monitor_over_channelizer_all": round(m / stages[name + "_channelizer_all"]["ms"], 3),
                            "monitor_over_channelizer_sel64": round(m / stages[name + "_channelizer_sel64"]["ms"], 3)}
        result = {"device": ctx.device_name(), "samples_per_call": N, "reps": REPS, "rounds": ROUNDS,
                  "shapes": {k: dict(zip(("M", "D", "n_taps"), v)) for k, v in SHAPES.items()},
                  "plans": {k: v[0].plan_info() for k, v in nodes.items()}, "stages": stages, "ratios": ratios,
                  "kernels": {k: v[0].kernel_names for k, v in nodes.items()}}
    finally:
        for p in (din, dsum, dout):
            ctx.free(p)
    for group in nodes.values():
        for v in group:
            v.close()
    ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
