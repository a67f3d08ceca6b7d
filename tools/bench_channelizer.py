"""Device-resident timing of the polyphase channelizer, and its measured error against the numpy restatement.
Timing, cs16 input, n = 2^20 samples per call: M = 1024 with 8192 taps at D = 1024 and D = 512, all channels and 64 selected ones;
and M = 128 with 512 taps at D = 128 beside a tuner bank of 128 SDRHIP_EPI_NONE channels on the same grid (its longest order, 513,
and /128) on the SAME input in the SAME run. The candidates are INTERLEAVED round by round: every round times each once, HIP
events over `reps` calls after a warm-up; the median and the range of the rounds are reported, with the algorithmic bytes of a
call (4 n in, 8 rows n / D out). Error: max |y - folded| / max |folded| per shape and input type of
tests/test_gpu_parity_channelizer.py, on that test's inputs. Writes profiles/channelizer_bench.json.
usage: python tools/bench_channelizer.py [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from benchkit import timed_interleaved  # noqa: E402

import libsdr_amd as sa

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "channelizer_bench.json")
N, FS = 1 << 20, 2.048e6
# name -> (M, D, n_taps, selected rows (None: all))
WORKLOADS = {"m1024_d1024_all": (1024, 1024, 8192, None), "m1024_d1024_sel64": (1024, 1024, 8192, 64),
             "m1024_d512_all": (1024, 512, 8192, None), "m1024_d512_sel64": (1024, 512, 8192, 64),
             "m128_d128_all": (128, 128, 512, None)}
TUNER_C, TUNER_ORDER, TUNER_D = 128, 513, 128


def parity(ctx):
    """{shape-dtype: max |y - folded| / max |folded|} on the parity test's own cases, one call each"""
    import test_gpu_parity_channelizer as P
    out = {}
    for shape in P.SHAPES:
        for dtype in P.DTYPES:
            taps, x, _, ref = P._case(shape, dtype)
            node = sa.Channelizer(ctx, np.int16 if dtype == "cs16" else np.float32, shape[0], shape[1], taps, max_in=len(x))
            out["%d-%d-%d-%s" % (shape + (dtype,))] = float("%.3g" % P._err(node.process(x), ref))
            node.close()
    return out


def main():
    ctx = sa.Context(0)
    rng = np.random.default_rng(1024)
    x = rng.integers(-12000, 12000, (N, 2)).astype(np.int16)
    nodes, rows = {}, {}
    for name, (M, D, n_taps, n_sel) in WORKLOADS.items():
        taps = sa.design_fir_lowpass(n_taps, FS / (2 * M), FS)
        sel = None if n_sel is None else [int(k) for k in rng.choice(M, n_sel, replace=False)]
        nodes[name] = sa.Channelizer(ctx, np.int16, M, D, taps, channels=sel, max_in=N)
        rows[name] = nodes[name].channels
    # the tuner bank on the M = 128 grid: channel k at k fs / 128 (above fs / 2: the negative frequency), a low-pass of the
    # channel's width, its longest order
    centres = [(k if k < TUNER_C // 2 else k - TUNER_C) * FS / TUNER_C for k in range(TUNER_C)]
    ttaps = np.stack([sa.design_iqbb_taps(f, FS / TUNER_C, FS, TUNER_ORDER) for f in centres])
    tuner = sa.TunerBankI16(ctx, ttaps, sa.design_freqshift_lut_i16(), [sa.design_freqshift_inc(f, FS) for f in centres],
                            [f < 0 for f in centres], TUNER_D, max_in=N, epilogue=sa.EPI_NONE)
    out_elems = max(max(rows[k] * (N // WORKLOADS[k][1]) for k in WORKLOADS), TUNER_C * (N // TUNER_D + 1))
    din, dout = ctx.malloc(x.nbytes), ctx.malloc(out_elems * 8)
    try:
        ctx.h2d(din, x)
        cand = {name: (lambda node=node, s=N // WORKLOADS[name][1]: node.process_dev(din, N, dout, s)) for name, node in nodes.items()}
        cand["tuner_128_order513_d128"] = lambda: tuner.process_dev(din, N, dout, N // TUNER_D + 1)
        stages = timed_interleaved(ctx, cand, REPS, ROUNDS)
        ctx.synchronize()
        for name in WORKLOADS:
            D = WORKLOADS[name][1]
            b = 4 * N + 8 * rows[name] * (N // D)
            stages[name].update(rows=rows[name], algorithmic_bytes=b, gb_per_s=round(b / stages[name]["ms"] / 1e6, 1))
        result = {"device": ctx.device_name(), "samples_per_call": N, "reps": REPS, "rounds": ROUNDS,
                  "workloads": {k: dict(zip(("M", "D", "n_taps"), v[:3])) for k, v in WORKLOADS.items()},
                  "plans": {k: v.plan_info() for k, v in nodes.items()}, "stages": stages,
                  "tuner": {"channels": TUNER_C, "order": TUNER_ORDER, "decim": TUNER_D, "kernels": tuner.kernel_names},
                  "kernels": {k: v.kernel_names for k, v in nodes.items()}}
    finally:
        ctx.free(din)
        ctx.free(dout)
    for v in list(nodes.values()) + [tuner]:
        v.close()
    result["parity_max_rel_err"] = parity(ctx)
    ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
