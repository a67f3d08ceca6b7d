"""Device-resident timing of the symbol path on 1024 channels x 8192 audio samples per step, AX.25 (L = 18) and RTTY
(L = 242) at 22 050 Hz: the detector kernel, the BitStream kernels, and the chain from cs16 input to bits
(IQBaseBand(127, /8, FM) -> FMDeemph -> FSKDetector -> BitStream, 65536 input samples per channel), beside the headline
chain alone (IQBaseBand(127, /8) -> FM on 1024 x 65536) timed in the SAME run. HIP events over `reps` steps after warm-up,
repeated `rounds` times: median and spread. Merges its result into profiles/symbols_bench.json next to `cpu_reference_ms`
(tools/golden_fsk: `make bench`, the reference's nodes on one core). Run under `rocprofv3 --kernel-trace --stats --` for the
per-kernel split. usage: python tools/bench_symbols.py [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libsdr_amd as sa

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "symbols_bench.json")
C, N_IN, D = 1024, 65536, 8
M = N_IN // D
FS_IN, FS = 22050.0 * D, 22050.0
WORKLOADS = {"ax25_L18": (1200.0, 1200.0, 2200.0), "rtty_L242": (90.90, 930.0, 1100.0)}


def timed(ctx, fn):
    for _ in range(5):
        fn()
    ms = []
    for _ in range(ROUNDS):
        t = sa.Timer(ctx)
        t.start()
        for _ in range(REPS):
            fn()
        t.stop()
        ms.append(t.elapsed_ms() / REPS)
    ms.sort()
    return {"ms": round(ms[len(ms) // 2], 5), "min_ms": round(ms[0], 5), "max_ms": round(ms[-1], 5)}


def main():
    ctx = sa.Context(0)
    r = np.random.default_rng(1)
    result = {"device": ctx.device_name(), "channels": C, "audio_samples_per_channel": M, "input_samples_per_channel": N_IN,
              "reps": REPS, "rounds": ROUNDS, "workloads": {}}
    taps, lut, inc = sa.design_iqbb_taps(10e3, 12e3, FS_IN, 127), sa.design_freqshift_lut_i16(), sa.design_freqshift_inc(10e3, FS_IN)
    din, dfm, dau, dsym = ctx.malloc(C * N_IN * 4), ctx.malloc(C * M * 2), ctx.malloc(C * M * 2), ctx.malloc(C * M)
    try:
        for name, (baud, f0, f1) in WORKLOADS.items():
            L = int(FS / np.float32(baud))
            n = N_IN
            key = np.repeat(r.integers(0, 2, (16, n // (L * D) + 2)), L * D, axis=1)[:, :n]   # 16 different rows, tiled
            audio = np.sin(2 * np.pi * np.cumsum(np.where(key, f1, f0) / FS_IN, axis=1))
            phase = 2 * np.pi * np.cumsum(3000.0 * audio / FS_IN, axis=1) + 2 * np.pi * 10e3 * np.arange(n) / FS_IN
            x = np.tile(np.stack([np.rint(9000 * np.cos(phase)), np.rint(9000 * np.sin(phase))], axis=2).astype(np.int16), (C // 16, 1, 1))
            ctx.h2d(din, x)
            del key, audio, phase, x
            bb = sa.IQBaseBandI16(ctx, taps, lut, inc, False, D, channels=C, max_in=N_IN, epilogue=sa.EPI_FM)
            de = sa.FMDeemphI16(ctx, sa.design_fmdeemph_alpha(FS), channels=C, max_in=M)
            det = sa.FSKDetector(ctx, FS, baud, f0, f1, channels=C, max_in=M)
            bits = sa.BitStream(ctx, FS, baud, sa.BITS_TRANSITION, channels=C, max_in=M)
            cap = bits.out_capacity(M)
            dbits, dcnt = ctx.malloc(C * cap), ctx.malloc(4 * C)
            try:
                def front():
                    no = bb.process_dev(din, N_IN, N_IN, dfm, M)
                    de.process_dev(dfm, no, M, dau, M)
                    return no

                def chain():
                    no = front()
                    det.process_dev(dau, no, M, dsym, M)
                    bits.process_dev(dsym, no, M, dbits, cap, dcnt)

                chain()
                ctx.synchronize()
                cnt = np.zeros(C, np.uint32)
                ctx.d2h(cnt, dcnt)
                w = {"corr_len": L, "bits_per_channel_and_step": float(cnt.mean()),
                     "headline_chain": timed(ctx, lambda: bb.process_dev(din, N_IN, N_IN, dfm, M)),
                     "front_end_with_deemph": timed(ctx, front),
                     "detector": timed(ctx, lambda: det.process_dev(dau, M, M, dsym, M)),
                     "bitstream": timed(ctx, lambda: bits.process_dev(dsym, M, M, dbits, cap, dcnt)),
                     "chain_to_bits": timed(ctx, chain),
                     "kernels": bb.kernel_names + de.kernel_names(M) + det.kernel_names + bits.kernel_names}
                w["chain_to_bits_over_headline"] = round(w["chain_to_bits"]["ms"] / w["headline_chain"]["ms"], 2)
                result["workloads"][name] = w
                print(json.dumps({name: w}), flush=True)
            finally:
                ctx.free(dbits)
                ctx.free(dcnt)
    finally:
        for p in (din, dfm, dau, dsym):
            ctx.free(p)
    ctx.close()
    old = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            old = json.load(f)
    for name, w in result["workloads"].items():   # keep what `make -C tools/golden_fsk bench` recorded
        cpu = old.get("workloads", {}).get(name, {}).get("cpu_reference")
        if cpu:
            w["cpu_reference"] = cpu
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
