"""Device-resident timing of the AGC bank on 1024 channels x 8192 samples per call, int16 and float rows, beside two stages
of the same size timed in the SAME run: the de-emphasis (sdrhip_deemph_i16, alpha of 22 050 Hz) and the BitStream stage
(1200 baud at 22 050 Hz). The candidates are INTERLEAVED round by round: every round times each once, HIP events over `reps`
calls after a warm-up; the median and the range of the rounds are reported. Writes profiles/agc_bench.json and keeps the
two entries of the file it finds there that it does not measure itself: "cpu_reference", merged in from
`make -C tools/golden_agc bench` (the reference's node on one core), and "earlier_geometry", the timings of the same kernel
with 16 rows per workgroup on which the 4 rows per workgroup were chosen.
usage: python tools/bench_agc.py [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchkit import timed_interleaved  # noqa: E402

import libsdr_amd as sa

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "agc_bench.json")
C, N, FS = 1024, 8192, 22050.0


def main():
    ctx = sa.Context(0)
    r = np.random.default_rng(20)
    # 16 different rows of tones plus noise at different levels, tiled; the symbol rows are random runs
    t = np.arange(N) / FS
    rows = np.stack([(0.05 + 0.05 * i) * np.sin(2 * np.pi * (300.0 + 90.0 * i) * t) + 0.02 * r.normal(size=N) for i in range(16)])
    x16 = np.tile(np.clip(np.rint(rows * 32767), -32768, 32767).astype(np.int16), (C // 16, 1))
    xf = np.tile(rows.astype(np.float32), (C // 16, 1))
    sym = np.tile(np.repeat(r.integers(0, 2, (16, N // 18 + 1)), 18, axis=1)[:, :N].astype(np.uint8), (C // 16, 1))
    lam = sa.design_agc_lambda(0.1, FS)
    agc16 = sa.AGC(ctx, np.int16, FS, channels=C, max_in=N)
    agcf = sa.AGC(ctx, np.float32, FS, channels=C, max_in=N)
    de = sa.FMDeemphI16(ctx, sa.design_fmdeemph_alpha(FS), channels=C, max_in=N)
    bits = sa.BitStream(ctx, FS, 1200.0, sa.BITS_TRANSITION, channels=C, max_in=N)
    cap = bits.out_capacity(N)
    d16, o16, df, of, dsym, dbits, dcnt = (ctx.malloc(b) for b in (C * N * 2, C * N * 2, C * N * 4, C * N * 4, C * N, C * cap, 4 * C))
    try:
        ctx.h2d(d16, x16)
        ctx.h2d(df, xf)
        ctx.h2d(dsym, sym)
        cand = {
            "agc_i16": lambda: agc16.process_dev(d16, N, N, o16, N),
            "agc_f32": lambda: agcf.process_dev(df, N, N, of, N),
            "deemph_i16": lambda: de.process_dev(d16, N, N, o16, N),
            "bitstream": lambda: bits.process_dev(dsym, N, N, dbits, cap, dcnt),
        }
        result = {"device": ctx.device_name(), "channels": C, "samples_per_channel": N, "reps": REPS, "rounds": ROUNDS, "lambda": lam,
                  "plan": agc16.plan_info(N), "stages": timed_interleaved(ctx, cand, REPS, ROUNDS, warmup=5),
                  "kernels": {"agc_i16": agc16.kernel_names, "agc_f32": agcf.kernel_names, "deemph_i16": de.kernel_names(N),
                              "bitstream": bits.kernel_names}}
        ctx.synchronize()
    finally:
        for p in (d16, o16, df, of, dsym, dbits, dcnt):
            ctx.free(p)
    for v in (agc16, agcf, de, bits):
        v.close()
    ctx.close()
    if os.path.exists(OUT):
        with open(OUT) as f:
            old = json.load(f)
        for key in ("cpu_reference", "earlier_geometry"):   # what this tool does not measure: the reference on one core, and
            if old.get(key):                                 # the 16-rows-per-group timings the geometry was chosen on
                result[key] = old[key]
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
