"""Device-resident timing of the audio channelizer beside the plain channelizer and the FM tuner bank.
cs16 input, n = 2^20 samples per call. Shapes: M = 1024 with 8192 taps at D = 1024 and D = 512, all rows and 64 selected ones;
M = 128 with 512 taps at D = 128, all rows. Rows: all FM, all AM, and mixed (FM, AM, USB in turn). In the SAME run on the SAME
input: the plain channelizer at each shape and selection, and — on the M = 128 grid — the 128-channel FM tuner bank (513 taps,
/128), which is what a grid FM receiver costs without this node. The candidates of a shape are INTERLEAVED round by round: every
round times each once, HIP events over `reps` calls after a warm-up; the median and the range of the rounds are reported.
Recorded per shape: the audio kernel's time over the plain channelizer's for each kind of rows; FM over AM (the halo image and the
second angle: the halo's share is at most that); on the M = 128 grid the tuner bank's time over the FM audio channelizer's.
Every shape runs in a child process of its own under a time limit; the first one that fails ends the run.
Writes profiles/chanaudio_bench.json.
usage: python tools/bench_chanaudio.py [reps] [rounds] [out.json]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchkit import timed_interleaved  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "chanaudio_bench.json")
N, FS = 1 << 20, 2.048e6
STEP_LIMIT_S = 150
# name -> (M, D, n_taps, selections (None: all rows), with the tuner bank)
SHAPES = {"m1024_d1024": (1024, 1024, 8192, (None, 64), False), "m1024_d512": (1024, 512, 8192, (None, 64), False),
          "m128_d128": (128, 128, 512, (None,), True)}
TUNER_C, TUNER_ORDER, TUNER_D = 128, 513, 128


def run_shape(name):
    """One shape, in this process: -> its part of the result."""
    import libsdr_amd as sa
    M, D, n_taps, selections, with_tuner = SHAPES[name]
    ctx = sa.Context(0)
    rng = np.random.default_rng(1024)
    x = rng.integers(-12000, 12000, (N, 2)).astype(np.int16)
    taps = sa.design_fir_lowpass(n_taps, FS / (2 * M), FS)
    kinds = {"fm": [sa.EPI_FM] * M, "am": [sa.EPI_AM] * M, "mixed": [(sa.EPI_FM, sa.EPI_AM, sa.EPI_USB)[k % 3] for k in range(M)]}
    nodes, cand, s = {}, {}, N // D
    for n_sel in selections:
        tag = "all" if n_sel is None else "sel%d" % n_sel
        sel = None if n_sel is None else [int(k) for k in rng.choice(M, n_sel, replace=False)]
        nodes["plain_" + tag] = sa.Channelizer(ctx, np.int16, M, D, taps, channels=sel, max_in=N)
        for kind, modes in kinds.items():
            nodes["audio_%s_%s" % (kind, tag)] = sa.AudioChannelizer(ctx, np.int16, M, D, taps, modes=modes, channels=sel, max_in=N)
    tuner = None
    if with_tuner:   # channel k at k fs / 128 (above fs / 2: the negative frequency), a low-pass of the channel's width, FM rows
        centres = [(k if k < TUNER_C // 2 else k - TUNER_C) * FS / TUNER_C for k in range(TUNER_C)]
        ttaps = np.stack([sa.design_iqbb_taps(f, FS / TUNER_C, FS, TUNER_ORDER) for f in centres])
        tuner = sa.TunerBankI16(ctx, ttaps, sa.design_freqshift_lut_i16(), [sa.design_freqshift_inc(f, FS) for f in centres],
                                [f < 0 for f in centres], TUNER_D, max_in=N, epilogue=sa.EPI_FM)
    din, dout = ctx.malloc(x.nbytes), ctx.malloc(8 * M * (s + 1))
    try:
        ctx.h2d(din, x)
        for k, node in nodes.items():
            cand[k] = lambda node=node: node.process_dev(din, N, dout, s)
        if tuner is not None:
            cand["tuner_fm_128_order513_d128"] = lambda: tuner.process_dev(din, N, dout, N // TUNER_D + 1)
        stages = timed_interleaved(ctx, cand, REPS, ROUNDS)
        ctx.synchronize()
    finally:
        ctx.free(din)
        ctx.free(dout)
    part = {"device": ctx.device_name(), "M": M, "D": D, "n_taps": n_taps, "stages": stages,
            "plans": {k: v.plan_info() for k, v in nodes.items()}, "kernels": {k: v.kernel_names for k, v in nodes.items()}, "ratios": {}}
    for k in nodes:
        if k.startswith("audio_"):
            tag = k.rsplit("_", 1)[1]
            part["ratios"][k + "_over_plain"] = round(stages[k]["ms"] / stages["plain_" + tag]["ms"], 3)
    for n_sel in selections:
        tag = "all" if n_sel is None else "sel%d" % n_sel
        part["ratios"]["fm_over_am_" + tag] = round(stages["audio_fm_" + tag]["ms"] / stages["audio_am_" + tag]["ms"], 3)
    if tuner is not None:
        part["tuner"] = {"channels": TUNER_C, "order": TUNER_ORDER, "decim": TUNER_D, "kernels": tuner.kernel_names}
        part["ratios"]["tuner_fm_over_audio_fm_all"] = round(stages["tuner_fm_128_order513_d128"]["ms"] / stages["audio_fm_all"]["ms"], 2)
        tuner.close()
    for v in nodes.values():
        v.close()
    ctx.close()
    return part


def main():
    if len(sys.argv) > 4:                      # a child: one shape, its part on the last line
        print(json.dumps(run_shape(sys.argv[4])), flush=True)
        return
    result = {"samples_per_call": N, "reps": REPS, "rounds": ROUNDS, "shapes": {}}
    for name in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(REPS), str(ROUNDS), OUT, name], capture_output=True, text=True,
                           timeout=STEP_LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("bench_chanaudio: shape %s ended with status %d; nothing further is started" % (name, r.returncode))
        part = json.loads(r.stdout.strip().splitlines()[-1])
        result.setdefault("device", part.pop("device"))
        result["shapes"][name] = part
        print(name, json.dumps(part["ratios"]), flush=True)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
