"""Device-resident timing of the interpolating resampler bank on 1024 channels x 8192 samples per call: the four element types
at frac 0.5, 1.378125 and 7.9 (every row of a bank the same frac), beside two stages of the same size timed in the SAME run as
yardsticks: the AGC bank (int16 and float rows) and the BitStream stage (1200 baud at 22 050 Hz). The candidates are INTERLEAVED
round by round: every round times each once, HIP events over `reps` calls after a warm-up; the median and the range of the
rounds are reported. Writes profiles/resample_bench.json and keeps the one entry of the file it finds there that it does not
measure itself: "cpu_reference", merged in from `make -C tools/golden_resample bench` (the reference's node on one core).
usage: python tools/bench_resample.py [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchkit import timed_interleaved  # noqa: E402

import libsdr_amd as sa
from libsdr_amd.resample import RESAMPLE_F32, RESAMPLE_CF32, RESAMPLE_I16, RESAMPLE_CS16_CF32

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "resample_bench.json")
C, N, FS = 1024, 8192, 22050.0
FRACS = {"0p5": 0.5, "1p378125": 1.378125, "7p9": 7.9}
# name -> (code, bytes per input element, bytes per output element)
TYPES = {"f32": (RESAMPLE_F32, 4, 4), "cf32": (RESAMPLE_CF32, 8, 8), "i16": (RESAMPLE_I16, 2, 2), "cs16_cf32": (RESAMPLE_CS16_CF32, 4, 8)}


def main():
    ctx = sa.Context(0)
    r = np.random.default_rng(22)
    # 16 different rows of tones plus noise at different levels, tiled; the symbol rows are random runs
    t = np.arange(N) / FS
    rows = np.stack([(0.05 + 0.05 * i) * np.sin(2 * np.pi * (300.0 + 90.0 * i) * t) + 0.02 * r.normal(size=N) for i in range(16)])
    quad = np.stack([(0.05 + 0.05 * i) * np.cos(2 * np.pi * (300.0 + 90.0 * i) * t) + 0.02 * r.normal(size=N) for i in range(16)])
    iq = np.stack([rows, quad], axis=2)
    i16 = lambda a: np.clip(np.rint(a * 32767), -32768, 32767).astype(np.int16)
    x = {"f32": np.tile(rows.astype(np.float32), (C // 16, 1)), "cf32": np.tile(iq.astype(np.float32), (C // 16, 1, 1)),
         "i16": np.tile(i16(rows), (C // 16, 1)), "cs16_cf32": np.tile(i16(iq), (C // 16, 1, 1))}
    sym = np.tile(np.repeat(r.integers(0, 2, (16, N // 18 + 1)), 18, axis=1)[:, :N].astype(np.uint8), (C // 16, 1))
    agc16 = sa.AGC(ctx, np.int16, FS, channels=C, max_in=N)
    agcf = sa.AGC(ctx, np.float32, FS, channels=C, max_in=N)
    bits = sa.BitStream(ctx, FS, 1200.0, sa.BITS_TRANSITION, channels=C, max_in=N)
    bcap = bits.out_capacity(N)
    nodes = {"%s_%s" % (d, tag): sa.InpolSubSampler(ctx, TYPES[d][0], frac, channels=C, max_in=N) for d in TYPES for tag, frac in FRACS.items()}
    cap = max(n.out_capacity(N) for n in nodes.values())
    din = {d: ctx.malloc(x[d].nbytes) for d in TYPES}
    dout, dcnt, dsym, dbits, o16, of = (ctx.malloc(b) for b in (C * cap * 8, 4 * C, C * N, C * bcap, C * N * 2, C * N * 4))
    try:
        for d in TYPES:
            ctx.h2d(din[d], x[d])
        ctx.h2d(dsym, sym)
        cand = {}
        for name, node in nodes.items():
            d = name.rsplit("_", 1)[0]
            cand[name] = (lambda node=node, p=din[d], c=node.out_capacity(N): node.process_dev(p, N, N, dout, c, dcnt))
        cand["agc_i16"] = lambda: agc16.process_dev(din["i16"], N, N, o16, N)
        cand["agc_f32"] = lambda: agcf.process_dev(din["f32"], N, N, of, N)
        cand["bitstream"] = lambda: bits.process_dev(dsym, N, N, dbits, bcap, dcnt)
        stages = timed_interleaved(ctx, cand, REPS, ROUNDS, warmup=5)
        ctx.synchronize()
        outputs = {}
        counts = np.zeros(C, np.uint32)
        for name, node in nodes.items():   # one more call each for the counts it writes
            cand[name]()
            ctx.synchronize()
            ctx.d2h(counts, dcnt)
            outputs[name] = int(counts[0])
        result = {"device": ctx.device_name(), "channels": C, "samples_per_channel": N, "reps": REPS, "rounds": ROUNDS,
                  "fracs": {k: float(np.float32(v)) for k, v in FRACS.items()}, "plan": nodes["f32_0p5"].plan_info(N), "stages": stages,
                  "outputs_per_row": outputs,
                  "kernels": dict({name: node.kernel_names for name, node in nodes.items()},
                                  agc_i16=agc16.kernel_names, agc_f32=agcf.kernel_names, bitstream=bits.kernel_names)}
    finally:
        for p in list(din.values()) + [dout, dcnt, dsym, dbits, o16, of]:
            ctx.free(p)
    for v in list(nodes.values()) + [agc16, agcf, bits]:
        v.close()
    ctx.close()
    if os.path.exists(OUT):
        with open(OUT) as f:
            old = json.load(f)
        if old.get("cpu_reference"):   # what this tool does not measure: the reference on one core
            result["cpu_reference"] = old["cpu_reference"]
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
