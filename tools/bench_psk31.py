"""Device-resident timing of the BPSK31 bank on 1024 channels x 8192 complex samples per call at 8000 Hz, complex<int16> and
complex<float> rows, beside two stages of the same size timed in the SAME run for scale: the AGC bank (int16 rows) and the
BitStream stage (1200 baud at 22 050 Hz). The candidates are INTERLEAVED round by round: every round times each once, HIP events
over `reps` calls after a warm-up; the median and the range of the rounds are reported. The rows hold 16 different PSK31 signals
(their own bits, carrier offsets and phases, light noise), tiled; the state streams on from call to call, as in a receiver.
Writes profiles/psk31_bench.json and keeps the entry of the file it finds there that it does not measure itself:
"cpu_reference", merged in from `make -C tools/golden_psk31 bench` (the reference's node on one core).
usage: python tools/bench_psk31.py [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from benchkit import timed_interleaved  # noqa: E402

import libsdr_amd as sa
import psk31_restatement as R

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "psk31_bench.json")
C, N, FS = 1024, 8192, 8000.0


def main():
    ctx = sa.Context(0)
    r = np.random.default_rng(21)
    rows = []
    for i in range(16):
        z = R.modulate(FS, r.integers(0, 2, N // 256 + 3), N, offset_hz=r.uniform(-5, 5), phase=r.uniform(0, 6))
        z = z + 0.01 * (r.standard_normal(N) + 1j * r.standard_normal(N))
        rows.append(np.stack([z.real, z.imag], axis=1))
    rows = np.stack(rows)
    x16 = np.tile(np.rint(rows * 32767).astype(np.int16), (C // 16, 1, 1))
    xf = np.tile(rows.astype(np.float32), (C // 16, 1, 1))
    sym = np.tile(np.repeat(r.integers(0, 2, (16, N // 18 + 1)), 18, axis=1)[:, :N].astype(np.uint8), (C // 16, 1))
    p16 = sa.BPSK31(ctx, np.int16, FS, channels=C, max_in=N)
    pf = sa.BPSK31(ctx, np.float32, FS, channels=C, max_in=N)
    agc16 = sa.AGC(ctx, np.int16, 22050.0, channels=C, max_in=N)
    bits = sa.BitStream(ctx, 22050.0, 1200.0, sa.BITS_TRANSITION, channels=C, max_in=N)
    cap, pcap = bits.out_capacity(N), p16.out_capacity(N)
    sizes = (C * N * 4, C * N * 8, C * pcap, 4 * C, C * N * 2, C * N * 2, C * N, C * cap, 4 * C)
    bufs = [ctx.malloc(b) for b in sizes]
    d16, df, pbits, pcnt, a_in, a_out, dsym, dbits, dcnt = bufs
    try:
        ctx.h2d(d16, x16)
        ctx.h2d(df, xf)
        ctx.h2d(a_in, np.ascontiguousarray(x16[:, :, 0]))
        ctx.h2d(dsym, sym)
        cand = {
            "psk31_cs16": lambda: p16.process_dev(d16, N, N, pbits, pcap, pcnt),
            "psk31_cf32": lambda: pf.process_dev(df, N, N, pbits, pcap, pcnt),
            "agc_i16": lambda: agc16.process_dev(a_in, N, N, a_out, N),
            "bitstream": lambda: bits.process_dev(dsym, N, N, dbits, cap, dcnt),
        }
        result = {"device": ctx.device_name(), "channels": C, "samples_per_channel": N, "sample_rate": FS, "reps": REPS, "rounds": ROUNDS,
                  "plan": p16.plan_info(N), "bit_capacity": pcap, "stages": timed_interleaved(ctx, cand, REPS, ROUNDS),
                  "kernels": {"psk31_cs16": p16.kernel_names, "psk31_cf32": pf.kernel_names, "agc_i16": agc16.kernel_names,
                              "bitstream": bits.kernel_names}}
        ctx.synchronize()
        counts = np.zeros(C, np.uint32)
        ctx.d2h(counts, pcnt)
        result["bits_of_the_last_call"] = {"min": int(counts.min()), "max": int(counts.max())}
    finally:
        for p in bufs:
            ctx.free(p)
    for v in (p16, pf, agc16, bits):
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
