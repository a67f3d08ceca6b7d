"""Device-resident timing of the tuner bank (sdrhip_tuner_i16_*): ONE input row of 65536 samples per step, C channels each with
its own tune, for C in {16, 128, 1024} and two plans — "fm127d8" (cs16, 127 taps, /8, FM) and "sdr_fm" (cu8, 21 taps, /125, FM).
Candidates, all timed in the SAME process, interleaved round by round (HIP events over `reps` steps, `rounds` rounds after
warm-up; median and range):
  a  what the library offered before the bank: C one-channel IQBaseBandI16 plans, each with its own tune, run back to back on
     the same device row
  b  the headline plan at the same C: C separate input rows, ONE tune (the same arithmetic per channel, C times the input)
  c  the bank, matrix form          d  the bank, plain form (SDRHIP_TUNER_PATH=valu)
Before anything is timed one step of c is compared with a's rows bit for bit. Writes profiles/tuner_bench.json, then exits
non-zero when c was not verified or is not faster than a at some C. c against b is reported (c_over_b), not gated.
--modes: the bank with a demodulator per channel (TunerBankI16(modes=...)) instead, at 1024 channels of both plans and in both
kernel forms, interleaved in the same way:
  fm       the bank with ONE demodulator, FM (c / d above)
  all_fm   the per-channel bank, every channel FM: the same geometry and the same work, the mode read per channel
  mixed    the per-channel bank, FM / AM / USB in turn
Before anything is timed, all_fm is compared with fm on every row and every row of mixed with the row of the single-demodulator
bank of its mode, bit for bit. Writes profiles/tuner_modes_bench.json; exits non-zero when a comparison failed. No speed gate.
--real: the bank of real-input channels (TunerBankI16(real=True): BaseBand<int16_t> over ONE row of real int16 samples) instead,
127 taps: 1024 channels at /20 FM, /8 FM and /20 USB, and 16 and 128 channels at /20 FM, interleaved in the same way:
  a        what the library offered before: C one-channel BaseBandI16 plans run back to back on the same device row
  complex  the complex bank at the same order, decimation, demodulator and C on a cs16 row of as many samples (matrix form)
  c        the real bank, matrix form          d  the real bank, plain form (SDRHIP_TUNER_PATH=valu)
Before anything is timed one step of c is compared with a's rows bit for bit. Writes profiles/tuner_real_bench.json with the
ratios a_over_c (and whether a's fastest round is still slower than c's slowest: the bank beats the one-channel plans by more
than the spread of the two measurements), c_over_complex and d_over_c; exits non-zero when c was not verified or that fails.
usage: python tools/bench_tuner.py [--modes | --real] [reps] [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libsdr_amd as sa

MODES = "--modes" in sys.argv[1:]
REAL = "--real" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a not in ("--modes", "--real")]
REPS = int(ARGS[0]) if len(ARGS) > 0 and ARGS[0].isdigit() else 50
ROUNDS = int(ARGS[1]) if len(ARGS) > 1 else 5
OUT = ARGS[2] if len(ARGS) > 2 else os.path.join(ROOT, "profiles", "tuner_modes_bench.json" if MODES else "tuner_real_bench.json" if REAL else "tuner_bench.json")
N = 65536
CHANNELS = (16, 128, 1024)
PLANS = {"fm127d8": dict(order=127, D=8, Fs=2.4e6, cu8=False), "sdr_fm": dict(order=21, D=125, Fs=1e6, cu8=True)}


def tunes(C, order, Fs):
    """C different tunes spread over 80 % of the band, widths 1 ... 4 % of it."""
    out = []
    for c in range(C):
        Fc = float(int((-0.4 + 0.8 * (c + 0.5) / C) * Fs))
        out.append((sa.design_iqbb_taps(Fc, (0.01 + 0.03 * (c % 7) / 7) * Fs, Fs, order), sa.design_freqshift_inc(Fc, Fs), Fc < 0))
    return out


def signal(rng, cu8):
    n = np.arange(N)
    ph = 2 * np.pi * (0.04 * n + 0.3 * np.sin(2 * np.pi * n / 5000.0))
    x = np.stack([np.cos(ph), np.sin(ph)], axis=1) * 9000 + rng.normal(0, 2500, (N, 2))
    if cu8:
        return np.clip(np.rint(x / 256 + 127.5), 0, 255).astype(np.uint8)
    return np.rint(x).astype(np.int16)


def measure(ctx, fns):
    """{name: fn} -> {name: {ms, min_ms, max_ms}}: every round times each candidate once, in turn."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    ctx.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t = sa.Timer(ctx)
            t.start()
            for _ in range(REPS):
                fn()
            t.stop()
            ms[k].append(t.elapsed_ms() / REPS)
    out = {}
    for k, v in ms.items():
        v.sort()
        out[k] = {"ms": round(v[len(v) // 2], 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5)}
    return out


def bank(ctx, tn, lut, D, cu8, valu, epilogue=sa.EPI_FM, modes=None, real=False):
    old = os.environ.pop("SDRHIP_TUNER_PATH", None)
    if valu:
        os.environ["SDRHIP_TUNER_PATH"] = "valu"
    try:
        b = sa.TunerBankI16(ctx, np.stack([np.asarray(t[0], np.int32).reshape(-1, 2) for t in tn]), lut, [t[1] for t in tn],
                            [t[2] for t in tn], D, max_in=N, epilogue=epilogue, modes=modes, real=real)
    finally:
        os.environ.pop("SDRHIP_TUNER_PATH", None)
        if old is not None:
            os.environ["SDRHIP_TUNER_PATH"] = old
    if cu8:
        b.set_input_format(sa.abi.IN_CU8)
    return b


def singles(ctx, tn, lut, D, cu8):
    nodes = []
    for t in tn:
        nd = sa.IQBaseBandI16(ctx, t[0], lut, t[1], t[2], D, channels=1, max_in=N, epilogue=sa.EPI_FM)
        if cu8:
            nd.set_input_format(sa.abi.IN_CU8)
        nodes.append(nd)
    return nodes


def run_case(ctx, rng, name, p, C):
    order, D, Fs, cu8 = p["order"], p["D"], p["Fs"], p["cu8"]
    lut = sa.design_freqshift_lut_i16()
    tn = tunes(C, order, Fs)
    x = signal(rng, cu8)
    eb = 2 if cu8 else 4
    M = N // D + 2
    din, dbig = ctx.malloc(N * eb), ctx.malloc(C * N * eb)
    da, dc = ctx.malloc(C * M * 2), ctx.malloc(C * M * 2)
    try:
        ctx.h2d(din, x)
        ctx.h2d(dbig, np.ascontiguousarray(np.broadcast_to(x, (C,) + x.shape)))
        # ---- c against a, bit for bit, both from a fresh state --------------------------------------------------------
        ya, yc = np.full((C, M), 0x5A5A, np.int16), np.full((C, M), 0x5A5A, np.int16)
        ctx.h2d(da, ya); ctx.h2d(dc, yc)
        a_nodes, c_bank = singles(ctx, tn, lut, D, cu8), bank(ctx, tn, lut, D, cu8, False)
        no = c_bank.process_dev(din, N, dc, M)
        for c, nd in enumerate(a_nodes):
            assert nd.process_dev(din, N, N, da + c * M * 2, M) == no
        ctx.synchronize()
        ctx.d2h(ya, da); ctx.d2h(yc, dc)
        verified = bool(np.array_equal(ya, yc)) and c_bank.kernel_names == ["tuner_i16_mfma_kernel"]
        # ---- timing ---------------------------------------------------------------------------------------------------
        d_bank = bank(ctx, tn, lut, D, cu8, True)
        b_node = sa.IQBaseBandI16(ctx, tn[0][0], lut, tn[0][1], tn[0][2], D, channels=C, max_in=N, epilogue=sa.EPI_FM)
        if cu8:
            b_node.set_input_format(sa.abi.IN_CU8)

        def run_a():
            for c, nd in enumerate(a_nodes):
                nd.process_dev(din, N, N, da + c * M * 2, M)

        r = measure(ctx, {"a_one_channel_plans": run_a,
                          "b_headline_plan": lambda: b_node.process_dev(dbig, N, N, da, M),
                          "c_bank_hot": lambda: c_bank.process_dev(din, N, dc, M),
                          "d_bank_plain": lambda: d_bank.process_dev(din, N, dc, M)})
        r.update({"verified_c_equals_a": verified, "outputs_per_channel": no,
                  "kernels": {"a": a_nodes[0].kernel_names, "b": b_node.kernel_names, "c": c_bank.kernel_names, "d": d_bank.kernel_names},
                  "a_over_c": round(r["a_one_channel_plans"]["ms"] / r["c_bank_hot"]["ms"], 2),
                  "c_over_b": round(r["c_bank_hot"]["ms"] / r["b_headline_plan"]["ms"], 2),
                  "d_over_c": round(r["d_bank_plain"]["ms"] / r["c_bank_hot"]["ms"], 2)})
        r["c_faster_than_a"] = r["c_bank_hot"]["ms"] < r["a_one_channel_plans"]["ms"]
        for nd in a_nodes + [b_node, c_bank, d_bank]:
            nd.close()
        return r
    finally:
        for q in (din, dbig, da, dc):
            ctx.free(q)


def run_modes_case(ctx, rng, p, C):
    order, D, Fs, cu8 = p["order"], p["D"], p["Fs"], p["cu8"]
    lut = sa.design_freqshift_lut_i16()
    tn = tunes(C, order, Fs)
    x = signal(rng, cu8)
    M = N // D + 2
    mixed_modes = [(sa.EPI_FM, sa.EPI_AM, sa.EPI_USB)[c % 3] for c in range(C)]
    din, dout = ctx.malloc(N * (2 if cu8 else 4)), ctx.malloc(C * M * 2)
    made = []

    def rows(b):
        """One step of a fresh bank: its rows."""
        made.append(b)
        y = np.full((C, M), 0x5A5A, np.int16)
        ctx.h2d(dout, y)
        b.process_dev(din, N, dout, M)
        ctx.synchronize()
        ctx.d2h(y, dout)
        return y

    try:
        ctx.h2d(din, x)
        out = {}
        for form, valu in (("matrix", False), ("plain", True)):
            cand = {"fm": bank(ctx, tn, lut, D, cu8, valu), "all_fm": bank(ctx, tn, lut, D, cu8, valu, modes=[sa.EPI_FM] * C),
                    "mixed": bank(ctx, tn, lut, D, cu8, valu, modes=mixed_modes)}
            y = {k: rows(b) for k, b in cand.items()}
            single = {sa.EPI_FM: y["fm"], sa.EPI_AM: rows(bank(ctx, tn, lut, D, cu8, valu, epilogue=sa.EPI_AM)),
                      sa.EPI_USB: rows(bank(ctx, tn, lut, D, cu8, valu, epilogue=sa.EPI_USB))}
            verified = bool(np.array_equal(y["all_fm"], y["fm"])) and all(np.array_equal(y["mixed"][c], single[m][c]) for c, m in enumerate(mixed_modes))
            r = measure(ctx, {k: (lambda b=b: b.process_dev(din, N, dout, M)) for k, b in cand.items()})
            r.update({"verified": verified, "kernels": {k: b.kernel_names for k, b in cand.items()},
                      "all_fm_over_fm": round(r["all_fm"]["ms"] / r["fm"]["ms"], 4), "mixed_over_fm": round(r["mixed"]["ms"] / r["fm"]["ms"], 4),
                      # the run-to-run range of the single-demodulator bank, as a fraction of its median
                      "fm_range": round((r["fm"]["max_ms"] - r["fm"]["min_ms"]) / r["fm"]["ms"], 4)})
            out[form] = r
        for b in made:
            b.close()
        return out
    finally:
        ctx.free(din); ctx.free(dout)


def main_modes():
    ctx = sa.Context(0)
    rng = np.random.default_rng(7)
    C = 1024
    result = {"device": ctx.device_name(), "samples_per_step": N, "channels": C, "reps": REPS, "rounds": ROUNDS,
              "mixed": "FM / AM / USB in turn (channel c: mode c % 3)", "plans": {}}
    for name, p in PLANS.items():
        r = run_modes_case(ctx, rng, p, C)
        result["plans"][name] = dict(p, forms=r)
        print(json.dumps({name: r}), flush=True)
    ctx.close()
    ok = all(f["verified"] for p in result["plans"].values() for f in p["forms"].values())
    result["verified_everywhere"] = ok
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("verified:", ok)
    sys.exit(0 if ok else 1)


REAL_FS = 2.0e6
# (decimation, demodulator, channels)
REAL_CASES = [(20, "fm", 1024), (8, "fm", 1024), (20, "usb", 1024), (20, "fm", 16), (20, "fm", 128)]


def real_tunes(C, order):
    """C different narrow channels spread over the band 0 ... 0.45 Fs of a real stream, widths 3 ... 12 kHz."""
    out = []
    for c in range(C):
        Fc = float(int(0.45 * (c + 0.5) / C * REAL_FS))
        out.append((sa.design_bb_taps(Fc, 3e3 + 9e3 * (c % 7) / 7, REAL_FS, order), sa.design_freqshift_inc(Fc, REAL_FS), False))
    return out


def run_real_case(ctx, rng, order, D, epi_name, C):
    epi = {"fm": sa.EPI_FM, "usb": sa.EPI_USB}[epi_name]
    lut = sa.design_freqshift_lut_i16()
    tn = real_tunes(C, order)
    n = np.arange(N)
    x = np.rint(9000 * np.cos(2 * np.pi * (0.04 * n + 0.3 * np.sin(2 * np.pi * n / 5000.0))) + rng.normal(0, 2500, N)).astype(np.int16)
    xc = signal(rng, False)
    M = N // D + 2
    din, dcx = ctx.malloc(N * 2), ctx.malloc(N * 4)
    da, dc = ctx.malloc(C * M * 2), ctx.malloc(C * M * 2)
    try:
        ctx.h2d(din, x); ctx.h2d(dcx, xc)
        ya, yc = np.full((C, M), 0x5A5A, np.int16), np.full((C, M), 0x5A5A, np.int16)
        ctx.h2d(da, ya); ctx.h2d(dc, yc)
        a_nodes = [sa.BaseBandI16(ctx, t[0], lut, t[1], t[2], D, channels=1, max_in=N, epilogue=epi) for t in tn]
        c_bank = bank(ctx, tn, lut, D, False, False, epilogue=epi, real=True)
        no = c_bank.process_dev(din, N, dc, M)
        for c, nd in enumerate(a_nodes):
            assert nd.process_dev(din, N, N, da + c * M * 2, M) == no
        ctx.synchronize()
        ctx.d2h(ya, da); ctx.d2h(yc, dc)
        verified = bool(np.array_equal(ya, yc)) and c_bank.kernel_names == ["tuner_bb_i16_mfma_kernel"]
        d_bank = bank(ctx, tn, lut, D, False, True, epilogue=epi, real=True)
        x_bank = bank(ctx, tunes(C, order, 2.4e6), lut, D, False, False, epilogue=epi)

        def run_a():
            for c, nd in enumerate(a_nodes):
                nd.process_dev(din, N, N, da + c * M * 2, M)

        r = measure(ctx, {"a_one_channel_plans": run_a,
                          "complex_bank_hot": lambda: x_bank.process_dev(dcx, N, da, M),
                          "c_bank_hot": lambda: c_bank.process_dev(din, N, dc, M),
                          "d_bank_plain": lambda: d_bank.process_dev(din, N, dc, M)})
        r.update({"order": order, "D": D, "epilogue": epi_name, "channels": C, "verified_c_equals_a": verified, "outputs_per_channel": no,
                  "plan_info": c_bank.plan_info(N), "complex_plan_info": x_bank.plan_info(N),
                  "kernels": {"a": a_nodes[0].kernel_names, "complex": x_bank.kernel_names, "c": c_bank.kernel_names, "d": d_bank.kernel_names},
                  "a_over_c": round(r["a_one_channel_plans"]["ms"] / r["c_bank_hot"]["ms"], 2),
                  "c_over_complex": round(r["c_bank_hot"]["ms"] / r["complex_bank_hot"]["ms"], 3),
                  "d_over_c": round(r["d_bank_plain"]["ms"] / r["c_bank_hot"]["ms"], 2),
                  "channel_msamples_per_s": round(C * N / r["c_bank_hot"]["ms"] / 1e3, 1)})
        # beyond the run-to-run spread of both measurements: a's fastest round against c's slowest
        r["c_faster_than_a_beyond_spread"] = r["c_bank_hot"]["max_ms"] < r["a_one_channel_plans"]["min_ms"]
        for nd in a_nodes + [c_bank, d_bank, x_bank]:
            nd.close()
        return r
    finally:
        for q in (din, dcx, da, dc):
            ctx.free(q)


def main_real():
    ctx = sa.Context(0)
    rng = np.random.default_rng(7)
    result = {"device": ctx.device_name(), "samples_per_step": N, "order": 127, "reps": REPS, "rounds": ROUNDS, "cases": []}
    for D, epi, C in REAL_CASES:
        r = run_real_case(ctx, rng, 127, D, epi, C)
        result["cases"].append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    result["conditions"] = {"c_verified_everywhere": all(r["verified_c_equals_a"] for r in result["cases"]),
                            "c_faster_than_a_beyond_spread_everywhere": all(r["c_faster_than_a_beyond_spread"] for r in result["cases"])}
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ok = all(result["conditions"].values())
    print("conditions:", json.dumps(result["conditions"]), "->", "ok" if ok else "FAILED")
    sys.exit(0 if ok else 1)


def main():
    if MODES:
        return main_modes()
    if REAL:
        return main_real()
    ctx = sa.Context(0)
    rng = np.random.default_rng(7)
    result = {"device": ctx.device_name(), "samples_per_step": N, "reps": REPS, "rounds": ROUNDS, "plans": {}}
    for name, p in PLANS.items():
        result["plans"][name] = dict(p, channels={})
        for C in CHANNELS:
            r = run_case(ctx, rng, name, p, C)
            result["plans"][name]["channels"][str(C)] = r
            print(json.dumps({name: {C: r}}), flush=True)
    ctx.close()
    cases = [r for p in result["plans"].values() for r in p["channels"].values()]
    result["conditions"] = {"c_verified_everywhere": all(r["verified_c_equals_a"] for r in cases),
                            "c_faster_than_a_everywhere": all(r["c_faster_than_a"] for r in cases),
                            "c_over_b_at_1024": {n: p["channels"]["1024"]["c_over_b"] for n, p in result["plans"].items()}}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ok = result["conditions"]["c_verified_everywhere"] and result["conditions"]["c_faster_than_a_everywhere"]
    print("conditions:", json.dumps(result["conditions"]), "->", "ok" if ok else "FAILED")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
