"""Device-resident timing of the polyphase synthesis bank, and its measured error against the numpy restatement.
Timing, complex float rows: M = 1024 with 8192 taps at D = 1024 and D = 512, 1024 columns per call (2^20 and 2^19 output samples),
all rows and 64 selected ones; and M = 128 with 512 taps at D = 128, 8192 columns per call. The yardstick is the cf32 `Channelizer`
on the mirrored shape — the same M, D, taps and rows, the synthesis call's output length as its input — in the SAME run: it moves
the same bytes the other way. The candidates are INTERLEAVED round by round: every round times each once, HIP events over `reps`
calls after a warm-up; the median and the range of the rounds are reported, with the algorithmic bytes of a call (8 rows n in,
8 n D out). Error: max |z - folded| / max |folded| per shape of tests/test_gpu_parity_synthesis.py, on that test's inputs.
Writes profiles/synthesis_bench.json.
usage: python tools/bench_synthesis.py [reps] [rounds] [out.json]
       python tools/bench_synthesis.py trace <workload> [calls]      that workload's calls alone, nothing written: the program of a
                                                                     `rocprofv3 --kernel-trace --stats --` run of its own
       python tools/bench_synthesis.py merge <workload> <kernel_stats.csv> [out.json]   that run's per-kernel averages into the
                                                                     JSON's "launch_split" (host only)"""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEFAULT_OUT = os.path.join(ROOT, "profiles", "synthesis_bench.json")
FS = 2.048e6
# name -> (M, D, n_taps, selected rows (None: all), columns per call)
WORKLOADS = {"m1024_d1024_all": (1024, 1024, 8192, None, 1024), "m1024_d1024_sel64": (1024, 1024, 8192, 64, 1024),
             "m1024_d512_all": (1024, 512, 8192, None, 1024), "m1024_d512_sel64": (1024, 512, 8192, 64, 1024),
             "m128_d128_all": (128, 128, 512, None, 8192)}
KERNELS = ("synthesis_transform_kernel", "synthesis_overlap_kernel")


def make(ctx, name, rng, yardstick):
    """(the workload's Synthesis, its Channelizer twin or None)"""
    import libsdr_amd as sa
    M, D, n_taps, n_sel, n = WORKLOADS[name]
    h = sa.design_fir_lowpass(n_taps, FS / (2 * M), FS)
    sel = None if n_sel is None else [int(k) for k in rng.choice(M, n_sel, replace=False)]
    syn = sa.Synthesis(ctx, M, D, D * np.asarray(h), channels=sel, max_in=n)
    return syn, (sa.Channelizer(ctx, np.float32, M, D, h, channels=sel, max_in=n * D) if yardstick else None)


def parity(ctx):
    """{shape: max |z - folded| / max |folded|} on the parity test's own cases, one call each"""
    import test_gpu_parity_synthesis as P
    out = {}
    for name in sorted(P.SHAPES):
        _, x, ref = P._case(name)
        node = P._node(ctx, name, x.shape[1])
        out[name] = float("%.3g" % P._err(node.process(x), ref))
        node.close()
    return out


def bench(reps, rounds, out_path):
    import libsdr_amd as sa
    from benchkit import timed_interleaved
    ctx = sa.Context(0)
    rng = np.random.default_rng(1024)
    pairs = {name: make(ctx, name, rng, True) for name in WORKLOADS}
    rows_elems = max(pairs[k][0].channels * WORKLOADS[k][4] for k in WORKLOADS)
    wide_elems = max(w[4] * w[1] for w in WORKLOADS.values())
    x = (0.25 * rng.standard_normal((rows_elems, 2))).astype(np.float32)
    z = (0.25 * rng.standard_normal((wide_elems, 2))).astype(np.float32)
    d_rows, d_wide, d_rows_out, d_wide_out = (ctx.malloc(8 * k) for k in (rows_elems, wide_elems, rows_elems, wide_elems))
    try:
        ctx.h2d(d_rows, x)
        ctx.h2d(d_wide, z)
        cand = {}
        for name, (syn, chan) in pairs.items():
            n, D = WORKLOADS[name][4], WORKLOADS[name][1]
            cand["synthesis_" + name] = lambda syn=syn, n=n: syn.process_dev(d_rows, n, 0, d_wide_out)
            cand["channelizer_" + name] = lambda chan=chan, n=n, D=D: chan.process_dev(d_wide, n * D, d_rows_out, n)
        stages = timed_interleaved(ctx, cand, reps, rounds)
        ctx.synchronize()
        ratio = {}
        for name, (syn, chan) in pairs.items():
            n, D = WORKLOADS[name][4], WORKLOADS[name][1]
            b = 8 * syn.channels * n + 8 * n * D
            for side in ("synthesis_", "channelizer_"):
                stages[side + name].update(rows=syn.channels, algorithmic_bytes=b, gb_per_s=round(b / stages[side + name]["ms"] / 1e6, 1))
            ratio[name] = round(stages["synthesis_" + name]["ms"] / stages["channelizer_" + name]["ms"], 3)
        result = {"device": ctx.device_name(), "reps": reps, "rounds": rounds,
                  "workloads": {k: dict(zip(("M", "D", "n_taps", "rows", "columns_per_call"), (v[0], v[1], v[2], pairs[k][0].channels, v[4])))
                                for k, v in WORKLOADS.items()},
                  "plans": {k: v[0].plan_info() for k, v in pairs.items()}, "stages": stages,
                  "synthesis_over_channelizer": ratio, "kernels": {k: v[0].kernel_names for k, v in pairs.items()}}
    finally:
        for p in (d_rows, d_wide, d_rows_out, d_wide_out):
            ctx.free(p)
    for syn, chan in pairs.values():
        syn.close()
        chan.close()
    result["parity_max_rel_err"] = parity(ctx)
    ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def trace(name, calls):
    import libsdr_amd as sa
    ctx = sa.Context(0)
    rng = np.random.default_rng(1024)
    syn, _ = make(ctx, name, rng, False)
    n, D = WORKLOADS[name][4], WORKLOADS[name][1]
    x = (0.25 * rng.standard_normal((syn.channels * n, 2))).astype(np.float32)
    d_rows, d_wide = ctx.malloc(x.nbytes), ctx.malloc(8 * n * D)
    try:
        ctx.h2d(d_rows, x)
        for _ in range(calls):
            syn.process_dev(d_rows, n, 0, d_wide)
        ctx.synchronize()
    finally:
        ctx.free(d_rows)
        ctx.free(d_wide)
    syn.close()
    ctx.close()
    print("traced %d calls of %s" % (calls, name))


def merge(name, stats_csv, out_path):
    with open(stats_csv) as f:
        table = list(csv.DictReader(f))
    split = {}
    for row in table:
        for k in KERNELS:
            if k in row["Name"]:
                split[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                            "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    assert sorted(split) == sorted(KERNELS), sorted(split)
    total = sum(v["average_us"] for v in split.values())
    for v in split.values():
        v["share"] = round(v["average_us"] / total, 3)
    with open(out_path) as f:
        result = json.load(f)
    result.setdefault("launch_split", {})[name] = split
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({name: split}))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "trace":
        trace(a[1], int(a[2]) if len(a) > 2 else 50)
    elif a and a[0] == "merge":
        merge(a[1], a[2], a[3] if len(a) > 3 else DEFAULT_OUT)
    else:
        bench(int(a[0]) if a else 20, int(a[1]) if len(a) > 1 else 7, a[2] if len(a) > 2 else DEFAULT_OUT)
