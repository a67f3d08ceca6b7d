"""Device-resident timing of the symbol path on 1024 channels x 8192 audio samples per step, AX.25 (L = 18) and RTTY
(L = 242) at 22 050 Hz: the detector kernel, the BitStream kernels, and the chain from cs16 input to bits
(IQBaseBand(127, /8, FM) -> FMDeemph -> FSKDetector -> BitStream, 65536 input samples per channel), beside the headline
chain alone (IQBaseBand(127, /8) -> FM on 1024 x 65536) timed in the SAME run. HIP events over `reps` steps after warm-up,
repeated `rounds` times: median and spread. Merges its result into profiles/symbols_bench.json next to `cpu_reference_ms`
(tools/golden_fsk: `make bench`, the reference's nodes on one core). Run under `rocprofv3 --kernel-trace --stats --` for the
per-kernel split. usage: python tools/bench_symbols.py [reps] [rounds] [out.json]

--per-channel: the detector and BitStream stages alone on 1024 channels x 8192 audio samples, candidates INTERLEAVED round by
round in one process: (a) the one-parameter handles at L = 18 and L = 242, (b) the per-channel handles (SymbolDetectorBank /
BitStreamBank) with every channel set to the same parameters, (c) a bank whose channels alternate between the two, and (d) the
regrouped alternative to (c): the audio rows gathered by protocol into two blocks (one row-gather launch on the context's
stream, inside the timed region; also timed alone) and two one-parameter handles of 512 channels each; its BitStream halves read
the symbols the detector halves left sorted. "detector_then_bitstream" times both stages of one step together. Device buffers,
the stream and the gather are torch's (plumbing); every timed kernel but the gather is the library's. Medians and ranges go to
profiles/symbols_per_channel_bench.json.
usage: python tools/bench_symbols.py --per-channel [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchkit import timed_interleaved  # noqa: E402

import libsdr_amd as sa

PER_CHANNEL = "--per-channel" in sys.argv
ARGS = [a for a in sys.argv[1:] if a != "--per-channel"]
REPS = int(ARGS[0]) if len(ARGS) > 0 else 50
ROUNDS = int(ARGS[1]) if len(ARGS) > 1 else 5
OUT = ARGS[2] if len(ARGS) > 2 else os.path.join(ROOT, "profiles", "symbols_per_channel_bench.json" if PER_CHANNEL else "symbols_bench.json")
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


def main_per_channel():
    import torch   # plumbing only: device buffers, the stream the context borrows, and the regrouped variant's row gather

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx = sa.Context(0, stream=stream.cuda_stream)
    r = np.random.default_rng(1)
    H = C // 2
    fsk = {name: (sa.design_fsk_lut(FS, b, f0), sa.design_fsk_lut(FS, b, f1)) for name, (b, f0, f1) in WORKLOADS.items()}
    baud = {name: w[0] for name, w in WORKLOADS.items()}
    a, b = list(WORKLOADS)
    # 16 different rows of keyed tones plus noise, tiled; even rows keyed at the first workload's rate, odd rows at the second's
    x = np.zeros((16, M), np.int16)
    for i in range(16):
        bd, f0, f1 = WORKLOADS[(a, b)[i & 1]]
        L = int(FS / np.float32(bd))
        key = np.repeat(r.integers(0, 2, M // L + 2), L)[:M]
        x[i] = np.rint(9000 * np.sin(2 * np.pi * np.cumsum(np.where(key, f1, f0) / FS)) + r.normal(0, 800, M)).astype(np.int16)
    x = np.tile(x, (C // 16, 1))
    T = sa.BITS_TRANSITION
    with torch.cuda.stream(stream):
        au = torch.from_numpy(x).to(dev)                              # the rows as a tuner bank leaves them: protocols interleaved
        au_s, sym, sym_s = torch.empty_like(au), torch.empty((C, M), dtype=torch.uint8, device=dev), torch.empty((C, M), dtype=torch.uint8, device=dev)
        by_protocol = torch.cat([torch.arange(0, C, 2), torch.arange(1, C, 2)]).to(dev)   # (d): even rows, then odd rows
        det = {"a_one_parameter_" + n: sa.SymbolDetector(ctx, sa.DET_FSK, *fsk[n], channels=C, max_in=M) for n in WORKLOADS}
        det.update({"b_per_channel_all_" + n: sa.SymbolDetectorBank(ctx, [("fsk",) + fsk[n]] * C, max_in=M) for n in WORKLOADS})
        det["c_per_channel_alternating"] = sa.SymbolDetectorBank(ctx, [("fsk",) + fsk[(a, b)[c & 1]] for c in range(C)], max_in=M)
        halves = [sa.SymbolDetector(ctx, sa.DET_FSK, *fsk[n], channels=H, max_in=M) for n in (a, b)]
        bits = {"a_one_parameter_" + n: sa.BitStream(ctx, FS, baud[n], T, channels=C, max_in=M) for n in WORKLOADS}
        bits.update({"b_per_channel_all_" + n: sa.BitStreamBank(ctx, FS, [baud[n]] * C, [T] * C, max_in=M) for n in WORKLOADS})
        bits["c_per_channel_alternating"] = sa.BitStreamBank(ctx, FS, [baud[(a, b)[c & 1]] for c in range(C)], [T] * C, max_in=M)
        bhalves = [sa.BitStream(ctx, FS, baud[n], T, channels=H, max_in=M) for n in (a, b)]
        cap = max(v.out_capacity(M) for v in bits.values())
        out = torch.empty((C, cap), dtype=torch.uint8, device=dev)
        cnt = torch.empty(C, dtype=torch.int32, device=dev)
        dau, dau_s, dsym, dsym_s, dbits, dcnt = (t.data_ptr() for t in (au, au_s, sym, sym_s, out, cnt))

        def gather():   # the copy a caller redoes after every tuner call: one launch, 16 MiB read and 16 MiB written
            torch.index_select(au, 0, by_protocol, out=au_s)

        def det_halves():
            halves[0].process_dev(dau_s, M, M, dsym_s, M)
            halves[1].process_dev(dau_s + H * M * 2, M, M, dsym_s + H * M, M)

        def det_regrouped():
            gather()
            det_halves()

        def bits_halves():   # (the symbols are sorted already: the detector halves wrote them so)
            bhalves[0].process_dev(dsym_s, M, M, dbits, cap, dcnt)
            bhalves[1].process_dev(dsym_s + H * M, M, M, dbits + H * cap, cap, dcnt + 4 * H)

        cand = {k: (lambda v=v: v.process_dev(dau, M, M, dsym, M)) for k, v in det.items()}
        cand["d_regrouped_gather_plus_two_halves"] = det_regrouped
        cand["d_regrouped_two_halves_alone"] = det_halves
        cand["d_regrouped_gather_alone"] = gather
        result = {"device": ctx.device_name(), "channels": C, "audio_samples_per_channel": M, "reps": REPS, "rounds": ROUNDS,
                  "corr_len": {n: int(FS / np.float32(baud[n])) for n in WORKLOADS},
                  "detector": timed_interleaved(ctx, cand, REPS, ROUNDS, warmup=5),
                  "detector_kernels": {k: v.kernel_names for k, v in det.items()}}
        print(json.dumps({"detector": result["detector"]}), flush=True)
        for v in [det["c_per_channel_alternating"]] + halves:            # (the timed calls left them at different sample counts)
            v.reset()
        det["c_per_channel_alternating"].process_dev(dau, M, M, dsym, M)   # the symbols the BitStream candidates read
        det_regrouped()
        ctx.synchronize()
        assert torch.equal(au.index_select(0, by_protocol), au_s)
        assert torch.equal(sym.index_select(0, by_protocol), sym_s)       # (d) computes (c)'s rows, regrouped
        cand = {k: (lambda v=v: v.process_dev(dsym, M, M, dbits, cap, dcnt)) for k, v in bits.items()}
        cand["d_regrouped_two_halves"] = bits_halves
        result["bitstream"] = timed_interleaved(ctx, cand, REPS, ROUNDS, warmup=5)
        result["bitstream_kernels"] = {k: v.kernel_names for k, v in bits.items()}
        print(json.dumps({"bitstream": result["bitstream"]}), flush=True)

        # both stages of one step, audio rows to bits
        def both(k):
            return lambda: (det[k].process_dev(dau, M, M, dsym, M), bits[k].process_dev(dsym, M, M, dbits, cap, dcnt))

        cand = {k: both(k) for k in det}
        cand["d_regrouped_gather_plus_two_halves_per_stage"] = lambda: (det_regrouped(), bits_halves())
        result["detector_then_bitstream"] = timed_interleaved(ctx, cand, REPS, ROUNDS, warmup=5)
        print(json.dumps({"detector_then_bitstream": result["detector_then_bitstream"]}), flush=True)
        ctx.synchronize()
        for v in list(det.values()) + list(bits.values()) + halves + bhalves:
            v.close()
    ctx.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main_per_channel() if PER_CHANNEL else main()
