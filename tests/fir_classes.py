"""The time-domain FIR kernels (libsdr_amd/csrc/fir.hip: sdrhip_fir::launch, reached through sdrhip_fir_* and, for the float
baseband, sdrhip_fbb_f32_*) by compiled instance: for every instance libsdrhip.so holds, the cases
tests/test_gpu_parity_fir_classes.py runs to reach it, each with the kernels every one of its calls must report through
last_kernels() (sdrhip_fir_last_kernels, sdrhip_fbb_f32_last_kernels), or the reason it is never launched. Plain Python, no
GPU: tests/test_fir_classes_complete.py holds MATRIX and EXCLUDED to the symbols of the library's gfx950 code objects.

This is NOT a model of the dispatch: a case states what it must run, as data, and the device says what it ran. The
expectations that depend on the CU count (fir_cs16_exact_kernel<*,8> from 8 workgroups per CU on; the float kernel at /8
left at one tile per workgroup on small batches) hold for the MI355X's 256 CUs."""
import os
import re
from collections import namedtuple

import numpy as np

UNALIGNED, ALIGNED = 37, 38      # RedZone.band, in row elements: 37 puts rows on every alignment; 38 keeps 8-byte elements 16-byte aligned
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIR_HIP = os.path.join(ROOT, "libsdr_amd", "csrc", "fir.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ROLL, PHASOR = "hist_roll_cf32", "tile_phasor_kernel"
ENV_HOOKS = ("SDRHIP_FIR_R", "SDRHIP_FIR_RFORCE", "SDRHIP_FIR_PIPE", "SDRHIP_FIR_TPW", "SDRHIP_FIR_TIME_DOMAIN", "SDRHIP_FIR_FFT_ALWAYS")
EPI_NONE, EPI_FM, EPI_AM, EPI_USB = 0, 1, 2, 3       # sdrhip.h: SDRHIP_EPI_*
FS, FC = 2.4e6, 100e3                                  # the float baseband's sample rate and tune


def exact(wrap, r2):
    """The launch record's spelling of fir_cs16_exact_kernel<WRAP, R2>."""
    return "fir_cs16_exact_kernel<%d,%d>" % (wrap, r2)


def rt(r, dc):
    return "fir_cf32_rt_kernel<%d,%d>" % (r, dc)


def pipe(r):
    return "fir_cf32_pipe_kernel<%d,8>" % r


# a kernel this table answers for: what the completeness test looks for among the compiled symbols (any fir_* kernel, so
# that a new one cannot arrive unnoticed)
_TRACKED = re.compile(r"^(fir_\w+(<[\d,]+>)?|tile_phasor_kernel|hist_roll_cf32)$")
_SYMBOL = re.compile(r"\b(fir_\w+|tile_phasor_kernel|hist_roll_cf32)(<[^()]*>)?\(")


def parse_nm(text):
    """The tracked kernels among `nm -C` lines, in the launch record's spelling."""
    got = set()
    for line in text.splitlines():
        m = _SYMBOL.search(line)
        if not m:
            continue
        args = (m.group(2) or "").replace("true", "1").replace("false", "0").replace(" ", "")
        got.add(m.group(1) + args)
    return got


# ---- cases ----------------------------------------------------------------------------------------------------------------
# kind "exact": sa.FIR(FIR_CS16_EXACT, taps, decim 1, C, max_in, epilogue) — bit for bit against the oracle; "float":
# sa.FIR(FIR_CF32, ...); "fbb": sa.FloatBaseBand(fc, FS, taps, decim, C, max_in) — both against the float64 reference below.
# taps: how case_taps makes the `order` coefficients. tile: input samples per tile of the instance the case must run
# (256 R D; exact kernel: 256 R2 - ovl). lens: the three calls. expect: per call, the kernels last_kernels() must report, in
# order. twin_env / twin_expect: the same plan under other hooks, whose outputs must equal the case's bit for bit. retune:
# (k, fc) — set_shift(fc) before call k. rows: the channels held to the reference (None: all). rtol: None = the contract (RTOL
# of tests/test_gpu_parity.py); a case that needs more says so here, with the figure measured on the CPU and the reason.
Case = namedtuple("Case", "id kind taps order decim epi C max_in env band tile lens expect twin_env twin_expect fc retune rows rtol")


def ragged(tile, k=1):
    """k tile + 3 (ends just behind a tile seam), 1 (shorter than any history), (k + 1) tile - 1 (ends one short of a seam). k > 1
    where the run must be longer than the filter, so that the impulse train meets every tap."""
    return [k * tile + 3, 1, (k + 1) * tile - 1]


def _case(id, kind, order, decim, tile, expect, taps="random", epi=EPI_NONE, C=3, max_in=None, env=None, band=UNALIGNED, lens=None,
          twin_env=None, twin_expect=None, fc=FC, retune=None, rows=None, rtol=None):
    lens = list(lens or ragged(tile))
    expect = [list(e) for e in expect]
    assert len(expect) == len(lens) == 3
    if twin_expect is not None:
        twin_expect = [list(e) for e in twin_expect]
    return Case(id, kind, taps, order, decim, epi, C, max_in or max(lens), dict(env or {}), band, tile, lens, expect,
                dict(twin_env or {}), twin_expect, fc if kind == "fbb" else None, retune, rows, rtol)


def calls(kernel, decim, first=None):
    """The three calls of a float plan on `kernel`: at a decimation above 1 the one-sample call completes no output and only
    rolls the history; `first`: what the first call reports where that differs."""
    return [first or [kernel], [kernel] if decim == 1 else [ROLL], [kernel]]


R4 = {"SDRHIP_FIR_R": "4", "SDRHIP_FIR_RFORCE": "1"}
NOPIPE = {"SDRHIP_FIR_PIPE": "0"}
TD = {"SDRHIP_FIR_TIME_DOMAIN": "1"}


def cases():
    c = []
    f = lambda id, order, D, R, kernel, **kw: c.append(_case(id, kw.pop("kind", "float"), order, D, 256 * R * D,
                                                             kw.pop("expect", None) or calls(kernel, D), **kw))
    # ---- fir_cf32_rt_kernel<4,0>: the generic-decimation instance, 4 outputs per lane ------------------------------------------
    f("f_127_d3", 127, 3, 4, rt(4, 0))
    f("f_21_d1_small_plan", 21, 1, 4, rt(4, 0))                        # (up to 32 taps on a small plan: no FFT convolution)
    f("f_127_d1_usb", 127, 1, 4, rt(4, 0), epi=EPI_USB)                # (a fused demodulator keeps the time-domain kernel)
    f("f_1_d1", 1, 1, 4, rt(4, 0))                                     # M = 1: no history, nothing to roll
    f("f_3_d3", 3, 3, 4, rt(4, 0))
    # ---- fir_cf32_rt_kernel<2,0> ----------------------------------------------------------------------------------------------
    f("f_127_d5", 127, 5, 2, rt(2, 0))
    # the long filters run k tiles per call so that the run is longer than the filter (the impulse train meets every tap); at /1
    # the one-sample call runs the FIR kernel, whose roll then copies old history forward (qq < HH)
    f("f_4097_d1_am", 4097, 1, 2, rt(2, 0), epi=EPI_AM, lens=ragged(512, 9))
    f("f_8192_d1_time_domain_lds104656", 8192, 1, 2, rt(2, 0), env=TD, lens=ragged(512, 17))
    # ---- fir_cf32_rt_kernel<1,0> ----------------------------------------------------------------------------------------------
    f("f_127_d16", 127, 16, 1, rt(1, 0))
    f("f_1025_d8_generic", 1025, 8, 1, rt(1, 0))                       # D = 8 but R = 1: not the compile-time-D instance
    f("f_127_d64_lds134288", 127, 64, 1, rt(1, 0))
    f("f_8192_d8_lds102568", 8192, 8, 1, rt(1, 0), lens=ragged(2048, 5))
    f("f_3_d16_order_below_d", 3, 16, 1, rt(1, 0))
    # ---- the compile-time /8 instances ------------------------------------------------------------------------------------------
    f("f_127_d8", 127, 8, 2, rt(2, 8))                                 # 3 channels: the device leaves one tile per workgroup
    f("f_127_d8_nopipe", 127, 8, 2, rt(2, 8), env=NOPIPE)
    # 3 tiles per workgroup: call 0 has 7 tiles (two whole runs of 3 and one of 1), call 2 has 2 (one partial run)
    f("f_127_d8_pipe_tpw3", 127, 8, 2, pipe(2), env={"SDRHIP_FIR_TPW": "3"}, lens=[4096 * 7 + 3, 1, 4096 * 2 - 1],
      twin_env=NOPIPE, twin_expect=calls(rt(2, 8), 8))
    f("f_127_d8_r4_lds71072", 127, 8, 4, rt(4, 8), env=R4)
    f("f_127_d8_r4_pipe_tpw2", 127, 8, 4, pipe(4), env=dict(R4, SDRHIP_FIR_TPW="2"), band=ALIGNED, lens=[8192 * 3 + 3, 1, 8192 * 2 - 1],
      twin_env=R4, twin_expect=calls(rt(4, 8), 8))
    # ---- the float baseband: the frequency shift fused into the staging of every float family -----------------------------------
    f("fbb_127_d3", 127, 3, 4, rt(4, 0), kind="fbb")
    f("fbb_127_d5_retune", 127, 5, 2, rt(2, 0), kind="fbb", retune=(2, -250e3))
    f("fbb_127_d16", 127, 16, 1, rt(1, 0), kind="fbb")
    f("fbb_127_d8_pipe_tpw3_retune", 127, 8, 2, pipe(2), kind="fbb", env={"SDRHIP_FIR_TPW": "3"}, lens=[4096 * 7 + 3, 1, 4096 * 2 - 1],
      retune=(2, 37e3), twin_env=NOPIPE, twin_expect=calls(rt(2, 8), 8))
    # more than 32 tiles in a call: the tile phasors come from tile_phasor_kernel's table (ptab), not from the arguments. Call 0
    # has 35 tiles of 4096 samples, call 2 has 3. The one large case.
    f("fbb_127_d8_tile_phasor", 127, 8, 2, rt(2, 8), kind="fbb", C=2, max_in=140000, lens=[140000, 1, 9000],
      expect=calls(rt(2, 8), 8, first=[PHASOR, rt(2, 8)]),
      twin_env={"SDRHIP_FIR_TPW": "16"}, twin_expect=calls(pipe(2), 8, first=[PHASOR, pipe(2)]))
    # ---- fir_cs16_exact_kernel<WRAP,R2>: bit for bit -----------------------------------------------------------------------------
    # The golden low-pass filters are normalised to sum |alpha| = 1: 32767 P + 32768 Q = 32767 + Q stays below 32768, no partial
    # sum can leave int16 and the plan takes the instance WITHOUT the per-tap wrap. At gain 1.25 the adversarial rows do wrap.
    e = lambda id, taps, order, epi, wrap, r2, **kw: c.append(_case(
        id, "exact", order, 1, 256 * r2 - (epi == EPI_FM), [[exact(wrap, r2)]] * 3, taps=taps, epi=epi, **kw))
    for r2, kw in ((4, {}), (8, dict(C=64, max_in=65536, rows=[0, 31, 63]))):     # 64 channels x 32 tiles of 2048: 8 workgroups per CU
        s = "" if r2 == 4 else "_c64"
        for epi, tag in ((EPI_NONE, "none"), (EPI_FM, "fm")):
            for order in (127, 255):
                e("x_lp%d_gain125_%s%s" % (order, tag, s), "lowpass*1.25", order, epi, 1, r2, **kw)
            e("x_lp127_above_threshold_%s%s" % (tag, s), "lowpass>threshold", 127, epi, 1, r2, **kw)
            e("x_lp127_threshold_%s%s" % (tag, s), "lowpass@threshold", 127, epi, 0, r2, **kw)
            e("x_lp127_%s%s" % (tag, s), "lowpass", 127, epi, 0, r2, **kw)
        e("x_1tap%s" % s, "0.999", 1, EPI_NONE, 0, r2, **kw)
    assert len({k.id for k in c}) == len(c)
    return c


def _matrix():
    m = {}
    for case in cases():
        for call in case.expect + (case.twin_expect or []):
            for k in call:
                assert _TRACKED.match(k), k
                if case.id not in m.setdefault(k, []):
                    m[k].append(case.id)
    return m


# instance -> the ids of the cases with a call that must run it
MATRIX = _matrix()

# compiled, never launched: instance -> (line of fir.hip that shuts it out, text that line holds, why). Empty: fir_cf32_kernel,
# the one-output-per-lane kernel that no launch site had named since the register-tiled form, is gone from fir.hip.
EXCLUDED = {}


def mismatches(matrix, excluded, compiled):
    """What keeps the tables from describing the build; [] when they do."""
    out = []
    want = set(matrix) | set(excluded)
    if compiled - want:
        out.append(("compiled, in no GPU case and not excluded", sorted(compiled - want)))
    if set(matrix) - compiled:
        out.append(("in the matrix, not compiled", sorted(set(matrix) - compiled)))
    if set(excluded) - compiled:
        out.append(("excluded, but not compiled", sorted(set(excluded) - compiled)))
    if set(matrix) & set(excluded):
        out.append(("both in the matrix and excluded", sorted(set(matrix) & set(excluded))))
    return out


# ---- taps ---------------------------------------------------------------------------------------------------------------------

def case_seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id.split("_c64")[0]))


def _lowpass(order):
    """FIRLowPass(order, 100 kHz at 2.4 MS/s) as the reference designed it: tests/golden (g2), sum |alpha| = 1."""
    return np.fromfile(os.path.join(GOLDEN, "g2_firlp_alpha%d.bin" % order), np.float64)


def wrap_sums(alpha):
    """(32767 P + 32768 Q, 32768 P + 32767 Q), P / Q the sums of the positive / |negative| taps: the largest positive and
    |negative| value a partial sum of the reference's per-tap loop can reach. Below 32768 / 32769 no per-tap int16 wrap can
    trigger (fir_load_taps)."""
    P, Q = alpha[alpha >= 0].sum(), -alpha[alpha < 0].sum()
    return 32767.0 * P + 32768.0 * Q, 32768.0 * P + 32767.0 * Q


def threshold_taps(order, level):
    """The low-pass scaled so that 32767 P + 32768 Q = level: 32767.5 is the last half step below the wrap decision's
    threshold, 32768.5 the first above."""
    a = _lowpass(order)
    return a * (level / wrap_sums(a)[0])


def case_taps(case):
    """The `order` float64 coefficients create takes; alpha[order - 1] meets the newest sample.
    random: magnitudes uniform in [0.5, 1.5] / sqrt(order) with random signs — no tap so small that its loss would hide below
    the tolerance (a windowed low-pass ends in zeros)."""
    if case.taps == "random":
        rng = np.random.default_rng(case_seed(case))
        return rng.choice([-1.0, 1.0], case.order) * rng.uniform(0.5, 1.5, case.order) / np.sqrt(case.order)
    if case.taps == "lowpass":
        return _lowpass(case.order)
    if case.taps == "lowpass*1.25":
        return _lowpass(case.order) * 1.25
    if case.taps == "lowpass@threshold":
        return threshold_taps(case.order, 32767.5)
    if case.taps == "lowpass>threshold":
        return threshold_taps(case.order, 32768.5)
    return np.array([float(case.taps)])


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def boundaries(case):
    """The absolute sample indices at which a call or a tile of a call starts (tiles counted from the call's first sample)."""
    out, start = [], 0
    for n in case.lens:
        out += list(range(start, start + n, case.tile))
        start += n
    return out + [start]


def impulse_positions(case):
    """An impulse on the last sample before every call and tile boundary and on sample 0, then one every order + D samples
    in between, never closer than that: at most one impulse lies in any output's window of order + D - 1 samples, the output
    right behind a seam carries the last taps, the outputs before it the first ones of the impulse before."""
    n, P = sum(case.lens), case.order + case.decim
    anchors = [0]
    for b in boundaries(case):
        if 0 < b - 1 < n and b - 1 - anchors[-1] >= P:
            anchors.append(b - 1)
    pos = []
    for a, nxt in zip(anchors, anchors[1:] + [n + P]):
        pos += list(range(a, nxt - P + 1, P))
    return pos


def adversarial_targets(case):
    """Output indices for the exact kernel's adversarial rows: the first output of every tile of every call (the seam) and one in
    every tile's interior, kept only where its window of `order` samples is clear of the one before."""
    want, start = [], 0
    for n in case.lens:
        for t0 in range(0, n, case.tile):
            want += [start + t0] + ([start + t0 + case.tile // 2] if t0 + case.tile // 2 < n else [])
        start += n
    out = []
    for t in sorted(want):
        if t >= case.order - 1 and (not out or t - case.order >= out[-1]):
            out.append(t)
    return out


def adversarial_row(case, alpha):
    """x[t - (order - 1) + j] = +32767 where alpha[j] >= 0, -32768 where alpha[j] < 0, for every target t (alpha[j] meets the
    j-th oldest sample of the window): every partial sum of the reference's per-tap loop is as large as the taps allow. Zero
    elsewhere."""
    x = np.zeros(sum(case.lens), np.int16)
    pat = np.where(alpha >= 0, 32767, -32768).astype(np.int16)
    for t in adversarial_targets(case):
        x[t - case.order + 1:t + 1] = pat
    return x


def mirrored(x):
    """+32767 <-> -32768 (zeros stay): every partial sum as negative as the taps allow."""
    return np.where(x == 0, 0, -1 - x.astype(np.int32)).astype(np.int16)


def case_inputs(case):
    """[(name, x)], x [C, sum(lens), 2].
    float kinds: white noise 0.3 N(0,1); the impulse train, channel c's turned by i^c (exact in any precision) so that no two
    neighbouring channels carry the same samples.
    exact kind: full-scale uniform int16; the adversarial rows — even channels carry the pattern in the real part and its
    mirror in the imaginary part, odd channels the other way round."""
    rng = np.random.default_rng(case_seed(case) + 1)
    n = sum(case.lens)
    if case.kind == "exact":
        uni = rng.integers(-32768, 32768, size=(case.C, n, 2)).astype(np.int16)
        a = adversarial_row(case, case_taps(case))
        adv = np.zeros((case.C, n, 2), np.int16)
        adv[0::2, :, 0], adv[0::2, :, 1] = a, mirrored(a)
        adv[1::2, :, 0], adv[1::2, :, 1] = mirrored(a), a
        return [("uniform", uni), ("adversarial", adv)]
    noise = rng.standard_normal((case.C, n, 2), dtype=np.float32) * np.float32(0.3)
    imp = np.zeros((case.C, n, 2), np.float32)
    pos = impulse_positions(case)
    for c in range(case.C):
        r = 1j ** c
        imp[c, pos, 0], imp[c, pos, 1] = r.real, r.imag
    return [("noise", noise), ("impulses", imp)]


# ---- the float64 reference -----------------------------------------------------------------------------------------------------

def shift_segments(case):
    """[(fc, k_sw, j_from)]: from output j_from on, the shift is exp(-2 pi i frac(fc (k - k_sw) / FS)) on EVERY sample k an
    output's window holds — set_shift restarts the phasor at the retuned call's first sample k_sw, the FIR history keeps
    the raw samples, and those before k_sw then meet the new phasor at negative k - k_sw (the float baseband is
    build-defined: tests/test_gpu_parity.py, test_float_baseband_setters_keep_the_stream)."""
    segs = [(case.fc, 0, 0)]
    if case.retune:
        k_sw = sum(case.lens[:case.retune[0]])
        segs.append((case.retune[1], k_sw, k_sw // case.decim))
    return segs


def reference(case, x, alpha):
    """x [n, 2], one channel's samples of all calls from the last reset -> what the plan owes for them in float64: the FIR
    (alpha[order - 1] on the newest sample, zeros before the first) of the shifted samples (shift_segments) as an FFT
    product on a transform that holds the whole linear convolution (its own error: some 1e-15 of the largest output), output
    j the mean of the FIR outputs jD ... jD + D - 1, then |y| (AM) or (re + im) / 2 (USB)."""
    xc = x[:, 0].astype(np.float64) + 1j * x[:, 1]
    n, D = len(xc), case.decim
    h = np.asarray(alpha, np.float64)[::-1]
    size = 1 << int(np.ceil(np.log2(n + len(h))))
    H = np.fft.fft(h, size)
    y = np.zeros(n // D, complex)
    for fc_, k_sw, j_from in (shift_segments(case) if case.kind == "fbb" else [(0.0, 0, 0)]):
        sh = xc * np.exp(-2j * np.pi * np.mod(fc_ * (np.arange(n, dtype=np.float64) - k_sw) / FS, 1.0))
        f = np.fft.ifft(np.fft.fft(sh, size) * H)[:n // D * D]
        y[j_from:] = f.reshape(-1, D).mean(axis=1)[j_from:]
    if case.epi == EPI_AM:
        return np.abs(y)
    if case.epi == EPI_USB:
        return (y.real + y.imag) / 2
    return y


def as_float64(case, y):
    """A plan's output rows [n_out, 2] or (demodulated) [n_out] as the reference's type."""
    y = np.asarray(y, np.float64)
    return y if case.epi != EPI_NONE else y[:, 0] + 1j * y[:, 1]


def out_lens(case):
    """Outputs per call: SubSample emits after every D-th input counted from the last reset."""
    ends = np.cumsum(case.lens)
    return [int(e // case.decim - (e - n) // case.decim) for e, n in zip(ends, case.lens)]
