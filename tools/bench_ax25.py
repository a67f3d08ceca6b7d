"""Timing of the AX.25 deframer bank on 1024 channels x 446 bits (one receiver call at 1200 baud, the row length of
tools/bench_pocsag.py and tools/bench_baudot.py) for three row kinds — noise, idle (flags back to back: every eighth position a
flag, nothing buffered) and traffic (UI frames back to back behind single shared flags) — and behind the receiver bank of
tools/bench_receiver.py (127 taps) with EVERY row on the AX.25 service (FM, de-emphasised, FSK 1200 / 2200 Hz, 1200 baud,
TRANSITION). Candidates INTERLEAVED round by round in one process, HIP events over `reps` calls after warm-up, `rounds` rounds
(default 7), median [min - max]:
  a_deframer_<kind>          one sdrhip_ax25_process_dev on the synthetic rows (the state carries from call to call)
  b_receiver_bank            one sdrhip_rxbank_process_dev
  c_receiver_then_deframer   (b), then the deframer on the receiver's own device rows
`cpu_reference_ms` is the unmodified reference node on the same rows, one core: `make -C tools/golden_ax25 bench`, which reads the
rows this tool writes with `rows` (the figures below were measured on the build machine). No time is fixed in advance.
Results go to profiles/ax25_bench.json.
usage: python tools/bench_ax25.py [reps] [rounds] [out.json]   |   python tools/bench_ax25.py rows <outdir> <rows> <bits>"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ax25_restatement as R  # noqa: E402  (the encoder)

CH, BITS = 1024, 446
KINDS = ("noise", "idle", "traffic")
# make -C tools/golden_ax25 bench, one core, reference sources at -O3: ms per call of 1024 rows x 446 bits
CPU_REFERENCE_MS = {"noise": 1.222, "idle": 0.703, "traffic": 10.702}


def bench_rows(kind, rows=CH, bits=BITS, seed=0xA825):
    r = np.random.default_rng(seed)
    if kind == "noise":
        return r.integers(0, 2, (rows, bits)).astype(np.uint8)
    if kind == "idle":
        return np.tile(np.array(R.FLAG, np.uint8), (rows, bits // 8 + 1))[:, :bits].copy()
    out = np.zeros((rows, bits), np.uint8)
    for c in range(rows):
        frames = [R.ui_frame(("APRS", 0), ("N%dCALL" % (c % 10), c % 16), text=bytes(r.integers(32, 127, int(r.integers(1, 12)), dtype=np.uint8)))
                  for _ in range(4)]
        out[c] = R.encode(frames, shared_flags=True, tail=bits)[:bits]
    return out


def write_rows(outdir, rows, bits):
    os.makedirs(outdir, exist_ok=True)
    for kind in KINDS:
        bench_rows(kind, rows, bits).tofile(os.path.join(outdir, "bench_%s.bin" % kind))


def main():
    import libsdr_amd as sa
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ax25_bench.json")
    N_IN, D, FS_IN, FS, ORDER = 65536, 8, 176400.0, 22050.0, 127
    M = N_IN // D
    ctx = sa.Context(0)
    result = {"device": ctx.device_name(), "channels": CH, "bits_per_row": BITS, "reps": reps, "rounds": rounds,
              "cpu_reference_ms": CPU_REFERENCE_MS}

    def timed_interleaved(candidates):
        for fn in candidates.values():
            for _ in range(3):
                fn()
        ms = {k: [] for k in candidates}
        for _ in range(rounds):
            for k, fn in candidates.items():
                t = sa.Timer(ctx)
                t.start()
                for _ in range(reps):
                    fn()
                t.stop()
                ms[k].append(t.elapsed_ms() / reps)
        out = {}
        for k, v in ms.items():
            v.sort()
            out[k] = {"ms": round(v[len(v) // 2], 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5)}
        return out

    # the receiver of tools/bench_receiver.py with every one of its 1024 rows an AX.25 channel: FM, 12.5 kHz wide, 127 taps
    r = np.random.default_rng(1)
    t = np.arange(N_IN)
    x = np.zeros(N_IN, np.complex128)
    for fc in (-60e3, -25e3, 10e3, 40e3, 70e3):
        key = np.repeat(r.integers(0, 2, N_IN // 147 + 2), 147)[:N_IN]   # 1200 baud at 176 400 Hz
        audio = np.sin(2 * np.pi * np.cumsum(np.where(key, 2200.0, 1200.0) / FS_IN))
        x += 4000 * np.exp(2j * np.pi * (fc * t / FS_IN + 3000.0 / FS_IN * np.cumsum(audio)))
    x = np.stack([x.real, x.imag], axis=1) + r.normal(0, 300, (N_IN, 2))
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    fcs = np.linspace(-80e3, 80e3, CH)
    taps = np.stack([np.asarray(sa.design_iqbb_taps(f, 12.5e3, FS_IN, ORDER), np.int32).reshape(-1, 2) for f in fcs])
    tuner = sa.TunerBankI16(ctx, taps, sa.design_freqshift_lut_i16(), [sa.design_freqshift_inc(f, FS_IN) for f in fcs], [f < 0 for f in fcs], D,
                            max_in=N_IN, modes=[sa.EPI_FM] * CH)
    aprs = ("fsk", sa.design_fsk_lut(FS, 1200.0, 1200.0), sa.design_fsk_lut(FS, 1200.0, 2200.0))
    deemph = sa.FMDeemphBankI16(ctx, sa.design_fmdeemph_alpha(FS), [True] * CH, max_in=M)
    det = sa.SymbolDetectorBank(ctx, [aprs] * CH, max_in=M)
    bits = sa.BitStreamBank(ctx, FS, [1200.0] * CH, [sa.BITS_TRANSITION] * CH, max_in=M)
    rx = sa.ReceiverBank(ctx, tuner, det, bits, deemph=deemph)
    cap = bits.out_capacity(M)
    bank = sa.AX25(ctx, CH, max(cap, BITS))
    bcap, fcap = bank.bytes_capacity(), bank.frames_capacity()
    sizes = {"in": N_IN * 4, "bits": CH * cap, "cnt": 4 * CH, "bytes": CH * bcap, "ev": 8 * CH * fcap, "fc": 4 * CH, "scnt": 4 * CH}
    sizes.update({"rows_" + k: CH * BITS for k in KINDS})
    d = {k: ctx.malloc(b) for k, b in sizes.items()}
    try:
        ctx.h2d(d["in"], x)
        ctx.h2d(d["scnt"], np.full(CH, BITS, np.uint32))

        def deframe(rows, stride, counts):
            bank.process_dev(rows, stride, counts, d["bytes"], bcap, d["ev"], fcap, d["fc"])

        frames = {}
        for k in KINDS:
            ctx.h2d(d["rows_" + k], bench_rows(k))
            bank.reset()
            deframe(d["rows_" + k], BITS, d["scnt"])
            ctx.synchronize()
            fc = np.zeros(CH, np.uint32)
            ctx.d2h(fc, d["fc"])
            frames[k] = float(fc.mean())
        bank.reset()
        cand = {"a_deframer_" + k: (lambda k=k: deframe(d["rows_" + k], BITS, d["scnt"])) for k in KINDS}
        cand["b_receiver_bank"] = lambda: rx.process_dev(d["in"], N_IN, d["bits"], cap, d["cnt"])

        def c():
            rx.process_dev(d["in"], N_IN, d["bits"], cap, d["cnt"])
            deframe(d["bits"], cap, d["cnt"])

        cand["c_receiver_then_deframer"] = c
        w = timed_interleaved(cand)
        ctx.synchronize()
        cnt = np.zeros(CH, np.uint32)
        ctx.d2h(cnt, d["cnt"])
        result.update(w)
        result["frames_per_row"] = frames
        result["receiver_bits_per_row"] = float(cnt.mean())
        result["kernels"] = bank.kernel_names
        b = w["b_receiver_bank"]
        result["a_over_b_percent"] = {k: round(100.0 * w["a_deframer_" + k]["ms"] / b["ms"], 2) for k in KINDS}
        result["c_minus_b_ms"] = round(w["c_receiver_then_deframer"]["ms"] - b["ms"], 5)
        result["c_inside_b_range"] = bool(b["min_ms"] <= w["c_receiver_then_deframer"]["ms"] <= b["max_ms"])
        result["cpu_reference_over_a"] = {k: (round(CPU_REFERENCE_MS[k] / w["a_deframer_" + k]["ms"], 1) if CPU_REFERENCE_MS[k] else None)
                                          for k in KINDS}
        print(json.dumps(result), flush=True)
    finally:
        ctx.synchronize()
        for p in d.values():
            ctx.free(p)
        bank.close()
        rx.close()
        for v in (tuner, deemph, det, bits):
            v.close()
        ctx.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rows":
        write_rows(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
