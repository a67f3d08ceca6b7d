"""Timing of the receiver bank on 1024 channels x 65536 cs16 antenna samples per step at 176 400 Hz, /8 (audio 22 050 Hz,
FMDeemph alpha = 2), for two tuners: 127 taps and the reference's 21 taps. The channels' services alternate AX.25 (FM,
de-emphasised) / RTTY (USB) / ASK (AM). Candidates INTERLEAVED round by round in one process, HIP events over `reps` steps after
warm-up, `rounds` rounds (default 7), median [min - max]:
  a_receiver_bank        one sdrhip_rxbank_process_dev per step
  b_chained_on_device    the same component handles chained by hand: four *_process_dev calls on device rows
  c_through_pinned_host  the same, with every stage's rows taken through pinned host buffers between the stages — what a graph of
                         today's nodes does
and, separately, the de-emphasis stage alone on 1024 x 8192 audio rows: the one-parameter handle, a bank with every row enabled,
a bank with every second row enabled. No time is fixed in advance; (a) is expected inside (b)'s own range, since it enqueues the
same launches, and the all-enabled bank is read against the one-parameter handle's range: what lies outside is the flag's cost.
Results go to profiles/receiver_bench.json. usage: python tools/bench_receiver.py [reps] [rounds] [out.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchkit import timed_interleaved  # noqa: E402

import libsdr_amd as sa
from libsdr_amd import abi

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "receiver_bench.json")
CH, N_IN, D = 1024, 65536, 8
M = N_IN // D
FS_IN, FS = 176400.0, 22050.0
AX25, RTTY = (1200.0, 1200.0, 2200.0), (90.90, 930.0, 1100.0)


def inside(x, ref):
    return ref["min_ms"] <= x["ms"] <= ref["max_ms"]


def antenna(r):
    t = np.arange(N_IN)
    x = np.zeros(N_IN, np.complex128)
    for fc in (-60e3, -25e3, 10e3, 40e3, 70e3):
        key = np.repeat(r.integers(0, 2, N_IN // 147 + 2), 147)[:N_IN]
        tone = np.sin(2 * np.pi * np.cumsum(np.where(key, 2200.0, 1200.0) / FS_IN))
        x += 4000 * (0.4 + 0.6 * key) * np.exp(2j * np.pi * (fc * t / FS_IN + np.cumsum(3000.0 * tone / FS_IN)))
    x = np.stack([x.real, x.imag], axis=1) + r.normal(0, 300, (N_IN, 2))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def receiver(ctx, order, x, result):
    L = abi.lib()
    fcs = np.linspace(-80e3, 80e3, CH)
    kind = [c % 3 for c in range(CH)]                                     # 0 AX.25 on FM, 1 RTTY on USB, 2 ASK on AM
    taps = np.stack([np.asarray(sa.design_iqbb_taps(f, (12.5e3, 2.5e3, 9e3)[k], FS_IN, order), np.int32).reshape(-1, 2) for f, k in zip(fcs, kind)])
    tuner = sa.TunerBankI16(ctx, taps, sa.design_freqshift_lut_i16(), [sa.design_freqshift_inc(f, FS_IN) for f in fcs], [f < 0 for f in fcs], D,
                            max_in=N_IN, modes=[(sa.EPI_FM, sa.EPI_USB, sa.EPI_AM)[k] for k in kind])
    fsk = {0: ("fsk", sa.design_fsk_lut(FS, *AX25[:2]), sa.design_fsk_lut(FS, AX25[0], AX25[2])),
           1: ("fsk", sa.design_fsk_lut(FS, *RTTY[:2]), sa.design_fsk_lut(FS, RTTY[0], RTTY[2])), 2: ("ask", False)}
    deemph = sa.FMDeemphBankI16(ctx, sa.design_fmdeemph_alpha(FS), [k == 0 for k in kind], max_in=M)
    det = sa.SymbolDetectorBank(ctx, [fsk[k] for k in kind], max_in=M)
    bits = sa.BitStreamBank(ctx, FS, [(1200.0, 90.90, 1200.0)[k] for k in kind],
                            [(sa.BITS_TRANSITION, sa.BITS_NORMAL, sa.BITS_NORMAL)[k] for k in kind], max_in=M)
    rx = sa.ReceiverBank(ctx, tuner, det, bits, deemph=deemph)
    cap = bits.out_capacity(M)
    sizes = {"in": N_IN * 4, "a0": CH * M * 2, "a1": CH * M * 2, "sym": CH * M, "bits": CH * cap, "cnt": 4 * CH}
    d = {k: ctx.malloc(b) for k, b in sizes.items()}
    host = {}
    for k in ("a0", "a1", "sym", "bits"):
        p = C.c_void_p()
        abi.check(L.sdrhip_host_alloc(sizes[k], C.byref(p)))
        host[k] = p
    ctx.h2d(d["in"], x)

    def a():
        rx.process_dev(d["in"], N_IN, d["bits"], cap, d["cnt"])

    def b():
        no = tuner.process_dev(d["in"], N_IN, d["a0"], M)
        deemph.process_dev(d["a0"], no, M, d["a1"], M)
        det.process_dev(d["a1"], no, M, d["sym"], M)
        bits.process_dev(d["sym"], no, M, d["bits"], cap, d["cnt"])

    def bounce(k):   # the stage's rows to the host and back: what the next node of a graph receives and uploads
        abi.check(L.sdrhip_memcpy_d2h_async(ctx.handle, host[k], C.c_void_p(d[k]), sizes[k]))
        abi.check(L.sdrhip_ctx_synchronize(ctx.handle))
        abi.check(L.sdrhip_memcpy_h2d_async(ctx.handle, C.c_void_p(d[k]), host[k], sizes[k]))

    def c():
        no = tuner.process_dev(d["in"], N_IN, d["a0"], M)
        bounce("a0")
        deemph.process_dev(d["a0"], no, M, d["a1"], M)
        bounce("a1")
        det.process_dev(d["a1"], no, M, d["sym"], M)
        bounce("sym")
        bits.process_dev(d["sym"], no, M, d["bits"], cap, d["cnt"])
        abi.check(L.sdrhip_memcpy_d2h_async(ctx.handle, host["bits"], C.c_void_p(d["bits"]), sizes["bits"]))
        abi.check(L.sdrhip_ctx_synchronize(ctx.handle))

    try:
        a()
        ctx.synchronize()
        cnt = np.zeros(CH, np.uint32)
        ctx.d2h(cnt, d["cnt"])
        w = timed_interleaved(ctx, {"a_receiver_bank": a, "b_chained_on_device": b, "c_through_pinned_host": c}, REPS, ROUNDS)
        w["bits_per_channel_and_step"] = float(cnt.mean())
        w["kernels"] = tuner.kernel_names + deemph.kernel_names(M) + det.kernel_names + bits.kernel_names
        w["a_inside_b_range"] = inside(w["a_receiver_bank"], w["b_chained_on_device"])
        w["c_over_a"] = round(w["c_through_pinned_host"]["ms"] / w["a_receiver_bank"]["ms"], 2)
        result["receiver_%d_taps" % order] = w
        print(json.dumps({"receiver_%d_taps" % order: w}), flush=True)
        if "deemph" not in result:       # the de-emphasis stage alone, on the audio rows the tuner left
            tuner.process_dev(d["in"], N_IN, d["a0"], M)
            one = sa.FMDeemphI16(ctx, sa.design_fmdeemph_alpha(FS), channels=CH, max_in=M)
            all_on = sa.FMDeemphBankI16(ctx, sa.design_fmdeemph_alpha(FS), [True] * CH, max_in=M)
            half = sa.FMDeemphBankI16(ctx, sa.design_fmdeemph_alpha(FS), [c % 2 == 0 for c in range(CH)], max_in=M)
            cand = {k: (lambda v=v: v.process_dev(d["a0"], M, M, d["a1"], M))
                    for k, v in (("one_parameter", one), ("bank_all_enabled", all_on), ("bank_half_enabled", half))}
            w = timed_interleaved(ctx, cand, REPS, ROUNDS)
            w["kernels"] = {"one_parameter": one.kernel_names(M), "bank": all_on.kernel_names(M)}
            w["all_enabled_inside_one_parameter_range"] = inside(w["bank_all_enabled"], w["one_parameter"])
            w["cost_of_the_flag_percent"] = round(100.0 * (w["bank_all_enabled"]["ms"] / w["one_parameter"]["ms"] - 1.0), 2)
            result["deemph"] = w
            print(json.dumps({"deemph": w}), flush=True)
            ctx.synchronize()
            for v in (one, all_on, half):
                v.close()
    finally:
        ctx.synchronize()
        for p in d.values():
            ctx.free(p)
        for p in host.values():
            L.sdrhip_host_free(p)
        rx.close()
        for v in (tuner, deemph, det, bits):
            v.close()


def main():
    ctx = sa.Context(0)
    result = {"device": ctx.device_name(), "channels": CH, "input_samples_per_channel": N_IN, "audio_samples_per_channel": M,
              "reps": REPS, "rounds": ROUNDS}
    x = antenna(np.random.default_rng(1))
    for order in (127, 21):
        receiver(ctx, order, x, result)
    ctx.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
