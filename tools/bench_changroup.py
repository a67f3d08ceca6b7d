"""Device-resident timing of the channel group (sdrhip_changroup.h) beside the SAME handles called one after another, in the SAME
run. Inputs: cs16 rows of 2^20 samples per member and real s16 rows of 2^21; shapes M = 1024 with 8192 taps at D = 1024, and
M = 128 with 512 taps at D = 128; every member has its own input row and its own output rows. Per input and shape:
  channelizer_a<A>, A = 1, 2, 4, 8   (a) one group call over A Channelizer members   (b) the A handles' own calls in turn
  audio_a4 (all FM), power_a4        the same pair for AudioChannelizer and ChannelPower
The A = 1 pair is the price of the member pick: one handle through the group against its own call.
The candidates of an input and shape are INTERLEAVED round by round: every round times each once, HIP events over `reps` calls
after a warm-up; the median and the range of the rounds are reported, and for each pair whether the group's median lies below
the members' range (or, for A = 1, outside it). Writes profiles/changroup_bench.json.
usage: python tools/bench_changroup.py [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchkit import timed_interleaved  # noqa: E402

import libsdr_amd as sa

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "changroup_bench.json")
FS, AMAX, SIZES = 2.048e6, 8, (1, 2, 4, 8)
INPUTS = {"cs16": (False, 1 << 20), "real_s16": (True, 1 << 21)}                # name -> (real, samples per member)
SHAPES = {"m1024_d1024": (1024, 1024, 8192), "m128_d128": (128, 128, 512)}       # name -> (M, D, n_taps)


def bench(ctx, real, N, M, D, n_taps, rng):
    """-> (stages, plans, kernels) of one input and shape"""
    taps = sa.design_fir_lowpass(n_taps, FS / (2 * M), FS)
    K, no = (M // 2 + 1 if real else M), N // D
    x = rng.integers(-12000, 12000, (AMAX, N) if real else (AMAX, N, 2)).astype(np.int16)
    din = ctx.malloc(x.nbytes)
    dout = ctx.malloc(AMAX * K * no * 8)
    dsum = ctx.malloc(AMAX * K * 8)
    ins = [din + a * (x.nbytes // AMAX) for a in range(AMAX)]
    outs = [dout + a * K * no * 8 for a in range(AMAX)]
    sums = [dsum + a * K * 8 for a in range(AMAX)]
    chan = [sa.Channelizer(ctx, np.int16, M, D, taps, max_in=N, real=real) for _ in range(AMAX)]
    audio = [sa.AudioChannelizer(ctx, np.int16, M, D, taps, max_in=N, real=real) for _ in range(4)]     # (the default: all FM)
    power = [sa.ChannelPower(ctx, np.int16, M, D, taps, alpha=0.25, max_in=N, real=real) for _ in range(4)]
    groups = {"channelizer_a%d" % A: sa.ChannelGroup(chan[:A]) for A in SIZES}
    groups["audio_a4"], groups["power_a4"] = sa.ChannelGroup(audio), sa.ChannelGroup(power)
    cand = {}
    try:
        ctx.h2d(din, x)
        for A in SIZES:
            g = groups["channelizer_a%d" % A]
            cand["channelizer_a%d_group" % A] = lambda g=g, A=A: g.process_dev(ins[:A], [N] * A, outs[:A], [no] * A)
            cand["channelizer_a%d_members" % A] = lambda A=A: [v.process_dev(i, N, o, no) for v, i, o in zip(chan[:A], ins, outs)]
        cand["audio_a4_group"] = lambda: groups["audio_a4"].process_dev(ins[:4], [N] * 4, outs[:4], [no] * 4)
        cand["audio_a4_members"] = lambda: [v.process_dev(i, N, o, no) for v, i, o in zip(audio, ins, outs)]
        cand["power_a4_group"] = lambda: groups["power_a4"].process_dev(ins[:4], [N] * 4, sums[:4])
        cand["power_a4_members"] = lambda: [v.process_dev(i, N, s) for v, i, s in zip(power, ins, sums)]
        stages = timed_interleaved(ctx, cand, REPS, ROUNDS)
        ctx.synchronize()
        plans = {k: g.plan_info() for k, g in groups.items()}
        kernels = {k: g.kernel_names for k, g in groups.items()}
    finally:
        for g in groups.values():
            g.close()
        for v in chan + audio + power:
            v.close()
        for p in (din, dout, dsum):
            ctx.free(p)
    return stages, plans, kernels


def compare(stages):
    """per pair: the two candidates, and where the group's median lies against the members' range"""
    pairs = {}
    for name in sorted({k.rsplit("_", 1)[0] for k in stages}):
        g, m = stages[name + "_group"], stages[name + "_members"]
        pairs[name] = {"group": g, "members": m, "group_below_members_range": g["ms"] < m["min_ms"],
                       "group_above_members_range": g["ms"] > m["max_ms"], "members_ms_minus_group_ms": round(m["ms"] - g["ms"], 5)}
    one = pairs["channelizer_a1"]
    outside = one["group_below_members_range"] or one["group_above_members_range"]
    pairs["channelizer_a1"]["cost_of_the_member_pick_ms"] = round(-one["members_ms_minus_group_ms"], 5) if outside else None
    return pairs


def main():
    ctx = sa.Context(0)
    rng = np.random.default_rng(2048)
    result = {"device": ctx.device_name(), "reps": REPS, "rounds": ROUNDS, "inputs": {k: v[1] for k, v in INPUTS.items()},
              "shapes": {k: dict(zip(("M", "D", "n_taps"), v)) for k, v in SHAPES.items()}, "pairs": {}, "plans": {}, "kernels": {}}
    for iname, (real, N) in INPUTS.items():
        for sname, (M, D, n_taps) in SHAPES.items():
            stages, plans, kernels = bench(ctx, real, N, M, D, n_taps, rng)
            key = iname + "_" + sname
            result["pairs"][key], result["plans"][key], result["kernels"][key] = compare(stages), plans, kernels
    ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
