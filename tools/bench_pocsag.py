"""Timing of the POCSAG decoder bank on 1024 channels x the bit rows of one receiver call of the README plan (8192 audio samples
at 22 050 Hz, 1200 baud: 446 bits per row), for three row kinds — noise (every channel waits for a sync word: the reference's
worst case), idle (a sync word, then idle codewords) and traffic (a sync word, then address and text codewords) — and behind the
receiver bank of tools/bench_receiver.py (127 taps). Candidates INTERLEAVED round by round in one process, HIP events over `reps`
calls after warm-up, `rounds` rounds (default 7), median [min - max]:
  a_decoder_<kind>          one sdrhip_pocsag_process_dev on the synthetic rows (idle, traffic: behind a reset, so that every
                            call decodes the rows from a fresh node, as the reference figure does)
  b_receiver_bank           one sdrhip_rxbank_process_dev
  c_receiver_then_decoder   (b), then the decoder on the receiver's own device rows
  d_bitstream_stage         the receiver's BitStream stage alone, on the symbol rows a receiver call left
`cpu_reference_ms` is the unmodified reference node on the same rows, one core: `make -C tools/golden_pocsag bench`, which
reads the rows this tool writes with `rows` (the figures below were measured on the build machine). No time is fixed in advance.
Results go to profiles/pocsag_bench.json.
usage: python tools/bench_pocsag.py [reps] [rounds] [out.json]   |   python tools/bench_pocsag.py rows <outdir> <rows> <bits>"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pocsag_restatement as P  # noqa: E402  (the encoder)

CH, BITS = 1024, 446
KINDS = ("noise", "idle", "traffic")
# make -C tools/golden_pocsag bench, one core, reference sources at -O3: ms per call of 1024 rows x 446 bits
CPU_REFERENCE_MS = {"noise": 1137.569, "idle": 105.841, "traffic": 114.631}


def bench_rows(kind, rows=CH, bits=BITS, seed=0x90C5A6):
    """[rows, bits] uint8. idle / traffic: 30 preamble bits, the sync word, then codewords to the row's end."""
    r = np.random.default_rng(seed)
    if kind == "noise":
        return r.integers(0, 2, (rows, bits)).astype(np.uint8)
    out = np.zeros((rows, bits), np.uint8)
    for c in range(rows):
        words = [P.SYNC_WORD]
        while 30 + 32 * len(words) < bits:
            k = len(words) - 1
            if kind == "idle":
                words.append(P.IDLE_WORD)
            elif k % 6 == 0:
                words.append(P.address_word((int(r.integers(0, 1 << 18)) << 3) | ((k // 2) % 8), int(r.integers(0, 4))))
            else:
                words.append(P.codeword((1 << 20) | int(r.integers(0, 1 << 20))))
        b = P.preamble(30) + [v for w in words for v in P.word_bits(w)]
        out[c] = b[:bits]
    return out


def write_rows(outdir, rows, bits):
    os.makedirs(outdir, exist_ok=True)
    for kind in KINDS:
        bench_rows(kind, rows, bits).tofile(os.path.join(outdir, "bench_%s.bin" % kind))


def main():
    import libsdr_amd as sa
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pocsag_bench.json")
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

    # the receiver of tools/bench_receiver.py: 1024 channels, AX.25 on FM / RTTY on USB / ASK on AM in turn, 127 taps
    r = np.random.default_rng(1)
    t = np.arange(N_IN)
    x = np.zeros(N_IN, np.complex128)
    for fc in (-60e3, -25e3, 10e3, 40e3, 70e3):
        key = np.repeat(r.integers(0, 2, N_IN // 147 + 2), 147)[:N_IN]
        tone = np.sin(2 * np.pi * np.cumsum(np.where(key, 2200.0, 1200.0) / FS_IN))
        x += 4000 * (0.4 + 0.6 * key) * np.exp(2j * np.pi * (fc * t / FS_IN + np.cumsum(3000.0 * tone / FS_IN)))
    x = np.stack([x.real, x.imag], axis=1) + r.normal(0, 300, (N_IN, 2))
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    fcs = np.linspace(-80e3, 80e3, CH)
    kind = [c % 3 for c in range(CH)]
    taps = np.stack([np.asarray(sa.design_iqbb_taps(f, (12.5e3, 2.5e3, 9e3)[k], FS_IN, ORDER), np.int32).reshape(-1, 2) for f, k in zip(fcs, kind)])
    tuner = sa.TunerBankI16(ctx, taps, sa.design_freqshift_lut_i16(), [sa.design_freqshift_inc(f, FS_IN) for f in fcs], [f < 0 for f in fcs], D,
                            max_in=N_IN, modes=[(sa.EPI_FM, sa.EPI_USB, sa.EPI_AM)[k] for k in kind])
    fsk = {0: ("fsk", sa.design_fsk_lut(FS, 1200.0, 1200.0), sa.design_fsk_lut(FS, 1200.0, 2200.0)),
           1: ("fsk", sa.design_fsk_lut(FS, 90.90, 930.0), sa.design_fsk_lut(FS, 90.90, 1100.0)), 2: ("ask", False)}
    deemph = sa.FMDeemphBankI16(ctx, sa.design_fmdeemph_alpha(FS), [k == 0 for k in kind], max_in=M)
    det = sa.SymbolDetectorBank(ctx, [fsk[k] for k in kind], max_in=M)
    bits = sa.BitStreamBank(ctx, FS, [(1200.0, 90.90, 1200.0)[k] for k in kind],
                            [(sa.BITS_TRANSITION, sa.BITS_NORMAL, sa.BITS_NORMAL)[k] for k in kind], max_in=M)
    rx = sa.ReceiverBank(ctx, tuner, det, bits, deemph=deemph)
    cap = bits.out_capacity(M)
    bank = sa.POCSAGBank(ctx, CH, max(cap, BITS))
    ecap = bank.out_capacity()
    sizes = {"in": N_IN * 4, "a0": CH * M * 2, "a1": CH * M * 2, "sym": CH * M, "bits": CH * cap, "cnt": 4 * CH, "ev": 8 * CH * ecap, "evc": 4 * CH,
             "scnt": 4 * CH}
    sizes.update({"rows_" + k: CH * BITS for k in KINDS})
    d = {k: ctx.malloc(b) for k, b in sizes.items()}
    try:
        ctx.h2d(d["in"], x)
        ctx.h2d(d["scnt"], np.full(CH, BITS, np.uint32))
        events = {}
        for k in KINDS:
            ctx.h2d(d["rows_" + k], bench_rows(k))
            bank.reset()
            bank.process_dev(d["rows_" + k], BITS, d["scnt"], d["ev"], ecap, d["evc"])
            ctx.synchronize()
            evc = np.zeros(CH, np.uint32)
            ctx.d2h(evc, d["evc"])
            events[k] = float(evc.mean())
        # the symbol rows of one receiver call, for the BitStream stage alone
        no = tuner.process_dev(d["in"], N_IN, d["a0"], M)
        deemph.process_dev(d["a0"], no, M, d["a1"], M)
        det.process_dev(d["a1"], no, M, d["sym"], M)
        ctx.synchronize()
        bank.reset()

        def decoder(k):
            if k != "noise":     # the same rows again: every call starts from a fresh node (one memset of the states, timed with it)
                bank.reset()
            bank.process_dev(d["rows_" + k], BITS, d["scnt"], d["ev"], ecap, d["evc"])

        cand = {"a_decoder_" + k: (lambda k=k: decoder(k)) for k in KINDS}
        cand["b_receiver_bank"] = lambda: rx.process_dev(d["in"], N_IN, d["bits"], cap, d["cnt"])

        def c():
            rx.process_dev(d["in"], N_IN, d["bits"], cap, d["cnt"])
            bank.process_dev(d["bits"], cap, d["cnt"], d["ev"], ecap, d["evc"])

        cand["c_receiver_then_decoder"] = c
        cand["d_bitstream_stage"] = lambda: bits.process_dev(d["sym"], no, M, d["bits"], cap, d["cnt"])
        w = timed_interleaved(cand)
        ctx.synchronize()
        cnt = np.zeros(CH, np.uint32)
        ctx.d2h(cnt, d["cnt"])
        result.update(w)
        result["events_per_row"] = events
        result["receiver_bits_per_row"] = float(cnt.mean())
        result["kernels"] = bank.kernel_names
        b = w["b_receiver_bank"]["ms"]
        result["a_over_b_percent"] = {k: round(100.0 * w["a_decoder_" + k]["ms"] / b, 2) for k in KINDS}
        result["c_minus_b_ms"] = round(w["c_receiver_then_decoder"]["ms"] - b, 5)
        result["c_over_b"] = round(w["c_receiver_then_decoder"]["ms"] / b, 4)
        result["a_over_bitstream_stage"] = {k: round(w["a_decoder_" + k]["ms"] / w["d_bitstream_stage"]["ms"], 3) for k in KINDS}
        result["cpu_reference_over_a"] = {k: (round(CPU_REFERENCE_MS[k] / w["a_decoder_" + k]["ms"], 1) if CPU_REFERENCE_MS[k] else None)
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
