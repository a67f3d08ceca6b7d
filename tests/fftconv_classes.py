"""The FFT convolution's kernels (libsdr_amd/csrc/fftconv.hip: sdrhip_fftconv::launch, GenConv::launch, BigConv::launch) by
compiled instance: for every instance libsdrhip.so holds, the cases tests/test_gpu_parity_fftconv_classes.py runs to reach
it, each with the kernels every one of its calls must report through last_kernels() (sdrhip_fftconv_last_kernels,
sdrhip_fir_last_kernels), or the reason it is never launched. Plain Python, no GPU: tests/test_fftconv_classes_complete.py
holds MATRIX and EXCLUDED to the symbols of the library's gfx950 code objects.

This is NOT a model of the dispatch: a case states what it must run, as data, and the device says what it ran. Where a
case's calls differ (a one-sample call has no second block for the pipelined form to walk) the case says so per call. The
expectations of the cases that leave the workgroup count of the pipelined form to the device (no SDRHIP_K7_PIPE_GRID) hold
for the MI355X's 256 CUs."""
import os
import re
from collections import namedtuple

import numpy as np

OLA, OLS = 0, 1                  # sdrhip.h: SDRHIP_FFTCONV_OLA (kernel = a 2N-point spectrum), _OLS (kernel = n_taps taps)
UNALIGNED, ALIGNED = 37, 38      # RedZone.band: 37 x 8 bytes puts rows on every alignment; 38 x 8 = 304 = 19 x 16 keeps them
                                 # 16-byte aligned and, for an even call length, the row strides even
FFTCONV_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libsdr_amd", "csrc", "fftconv.hip")
ROLL = "hist_roll_kernel"
ENV_HOOKS = ("SDRHIP_K7_PIPE_GRID", "SDRHIP_K7_NT", "SDRHIP_K7_RUNTIME_PLAN", "SDRHIP_K7_PIPE_X2", "SDRHIP_FFTCONV_ODD_HOP",
             "SDRHIP_FFTCONV_LITERAL", "SDRHIP_FFTCONV_NO_PARTS", "SDRHIP_FIR_TIME_DOMAIN", "SDRHIP_FIR_FFT_ALWAYS")


def fused(lg, bank, nt, acc=0, pipe=0, skip=0):
    """The launch record's spelling of fftconv_fused_kernel<LG, BANK, NT, ACC, PIPE, SKIP>."""
    return "fftconv_fused_kernel<%d,%d,%d,%d,%d,%d>" % (lg, bank, nt, acc, pipe, skip)


def typed(kernel, f64):
    return "%s<%s>" % (kernel, "double2" if f64 else "float2")


# a kernel this table answers for: what the completeness test looks for among the compiled symbols
_TRACKED = re.compile(r"^(fftconv_fused_kernel<[\d,]+>|fftconv_kernel|conv_kernel<\w+>|big_\w+_kernel<\w+>)$")
_SYMBOL = re.compile(r"\b(fftconv_fused_kernel|fftconv_kernel|conv_kernel|big_[a-z]+_kernel)(<[^()]*>)?\(")


def parse_nm(text):
    """The tracked kernels among `nm -C` lines, in the launch record's spelling."""
    got = set()
    for line in text.splitlines():
        m = _SYMBOL.search(line)
        if not m:
            continue
        name, args = m.group(1), m.group(2) or ""
        args = args.replace("HIP_vector_type<float, 2u>", "float2").replace("HIP_vector_type<double, 2u>", "double2")
        args = args.replace("true", "1").replace("false", "0").replace(" ", "")
        got.add(name + args)
    return got


# ---- cases ----------------------------------------------------------------------------------------------------------------
# kind "fftconv": sdrhip_fftconv(_f64)_create_bank(mode, fft_size, n_taps taps | a 2 n_taps-point spectrum, bands, C, max_in);
# kind "fir": sdrhip_fir_create(FIR_CF32, n_taps coefficients, decim 1, C, max_in) — the route into the same kernels.
# hop: the samples a block keeps (the impulse train sits on the block seams). lens: the three calls. expect: per call, the
# kernels last_kernels() must report, in order. twin_env / twin_expect: the same plan under other hooks, whose outputs must
# equal the case's bit for bit. rows: the channels held to the float64 reference (None: all). rtol: None = the contract
# (RTOL of tests/test_gpu_parity.py for complex<float>, 1e-12 for complex<double>); a case that needs more says so here,
# with the value measured against the float64 reference and the reason.
Case = namedtuple("Case", "id kind mode fft_size n_taps bands C max_in f64 env band hop lens expect twin_env twin_expect rows rtol")


def ragged(hop, cap=50000):
    """hop + 3 (ends just behind a block seam), 1 (shorter than any history), 2 hop - 1 (ends one short of a seam), the last
    cut down so that the three stay within `cap` samples."""
    a = hop + 3
    return [a, 1, max(2, min(2 * hop - 1, cap - a - 1))]


def even_lens(hop, cap=50000):
    """The same with every length even: the 16-byte form of the pipelined kernel needs an even call length."""
    a = hop + 4
    return [a, 2, max(2, min(2 * hop - 2, (cap - a - 2) & ~1))]


def _case(id, fft_size, n_taps, expect, kind="fftconv", mode=OLS, bands=1, C=3, max_in=None, f64=False, env=None, band=UNALIGNED,
          lens=None, hop=None, twin_env=None, twin_expect=None, rows=None, rtol=None):
    if hop is None:
        hop = fft_size - n_taps + 1
        if hop > 1 and hop % 2 and not f64 and _is_pow2(fft_size) and 4 <= fft_size <= 16384 and not (env or {}).get("SDRHIP_FFTCONV_ODD_HOP"):
            hop -= 1      # (the tuned plans round an odd hop down: one more sample of history)
    lens = lens or ragged(hop)
    if expect and isinstance(expect[0], str):
        expect = [list(expect)] * len(lens)
    if twin_expect and isinstance(twin_expect[0], str):
        twin_expect = [list(twin_expect)] * len(lens)
    assert len(expect) == len(lens)
    return Case(id, kind, mode, fft_size, n_taps, bands, C, max_in or max(lens), f64, dict(env or {}), band, hop, list(lens),
                [list(e) for e in expect], dict(twin_env or {}), twin_expect, rows, rtol)


def _is_pow2(n):
    return n >= 1 and n & (n - 1) == 0


PLAIN14 = fused(14, 0, 1024)
GRID0 = {"SDRHIP_K7_PIPE_GRID": "0"}
RUNTIME = {"SDRHIP_K7_RUNTIME_PLAN": "1"}
NT_OF = {2048: 128, 4096: 256, 8192: 512}
LG_OF = {2048: 11, 4096: 12, 8192: 13}


def _pipelined():
    """The six pipelined forms of the 16384-point plan, PIPE in {4, 2} x HH in {4096, 8192, other}: 4 channels on 3 persistent
    workgroups (every call, the one- or two-sample call too, has more units than workgroups); the XCD-ordered walk (8 channels
    on 8 workgroups: its short call has 8 units for 8 workgroups and runs the one-block kernel); the odd-hop route into the
    8-byte form on aligned rows. Each against the one-block-per-workgroup kernel on the same plan, bit for bit."""
    out = []
    g3 = {"SDRHIP_K7_PIPE_GRID": "3"}
    for taps, hh, tag in ((4097, 4096, "hh4096"), (8192, 8192, "hh8192"), (1000, 1000, "hh1000")):
        hop = 16384 - hh
        s4, s2 = {4096: (2, 4), 8192: (4, 8), 1000: (0, 0)}[hh]
        out.append(_case("pipe4_%s" % tag, 16384, taps, [fused(14, 0, 1024, 0, 4, s4)], C=4, env=g3, band=ALIGNED, hop=hop,
                         lens=even_lens(hop), twin_env=GRID0, twin_expect=[PLAIN14]))
        out.append(_case("pipe2_%s" % tag, 16384, taps, [fused(14, 0, 1024, 0, 2, s2)], C=4, env=g3, band=UNALIGNED, hop=hop,
                         twin_env=GRID0, twin_expect=[PLAIN14]))
    g8 = {"SDRHIP_K7_PIPE_GRID": "8"}
    p4, p2 = fused(14, 0, 1024, 0, 4, 2), fused(14, 0, 1024, 0, 2, 4)
    out.append(_case("pipe4_xcd_c8", 16384, 4097, [[p4], [PLAIN14], [p4]], C=8, env=g8, band=ALIGNED, hop=12288, lens=even_lens(12288, 40000),
                     twin_env=GRID0, twin_expect=[PLAIN14]))
    out.append(_case("pipe2_xcd_c8", 16384, 4097, [[p2], [PLAIN14], [p2]], C=8, env=g8, band=UNALIGNED, hop=12288, lens=ragged(12288, 40000),
                     twin_env=GRID0, twin_expect=[PLAIN14]))
    odd = dict(g3, SDRHIP_FFTCONV_ODD_HOP="1")
    out.append(_case("pipe2_oddhop_aligned_rows", 16384, 1000, [fused(14, 0, 1024, 0, 2, 0)], C=4, env=odd, band=ALIGNED, hop=15385,
                     lens=[15390, 2, 30768], twin_env=dict(GRID0, SDRHIP_FFTCONV_ODD_HOP="1"), twin_expect=[PLAIN14]))
    return out


def cases():
    c = []
    # ---- 16384 points on 1024 lanes --------------------------------------------------------------------------------------
    c.append(_case("plain14_few_blocks", 16384, 4097, [PLAIN14], C=2, hop=12288))       # 4 units at most: fewer than any device's CUs
    # an overlap-add plan of 12290 ... 16384 taps: two tap partitions of 8192 on the 16384-point kernel, the second accumulated
    for N in (12290, 16384):
        c.append(_case("acc14_ola_n%d" % N, 2 * N, N, [PLAIN14, fused(14, 0, 1024, 1)], mode=OLA, C=2, env=GRID0, hop=8192))
    c += _pipelined()
    # ---- compile-time plans 11, 12, 13 (1 band and a bank of 3), each equal to the run-time plan of its size bit for bit -------
    for L in (2048, 4096, 8192):
        for bands in (1, 3):
            bank = int(bands > 1)
            c.append(_case("ct%d_b%d" % (LG_OF[L], bands), L, L // 4 + 1, [fused(LG_OF[L], bank, NT_OF[L])], bands=bands,
                           twin_env=RUNTIME, twin_expect=[fused(0, bank, NT_OF[L])]))
            c.append(_case("rt%d_b%d" % (NT_OF[L], bands), L, L // 4 + 2, [fused(0, bank, NT_OF[L])], bands=bands, env=RUNTIME))
    # ---- the run-time plan on 64 lanes: every fusable size has its own tail of passes (16.2, 16.4, 16.4.2, 16.16, 16.16.2,
    # 16.16.4); a bank shares its forward transform from 1024 points on, below it launches once per band ------------------------
    for L in (32, 64, 128, 256, 512, 1024):
        c.append(_case("rt64_l%d_b1" % L, L, L // 4 + 1, [fused(0, 0, 64)]))
        c.append(_case("rt64_l%d_b3" % L, L, L // 4 + 1, [fused(0, 1, 64)] if L == 1024 else [fused(0, 0, 64)] * 3, bands=3))
    # SDRHIP_K7_NT reaches the 1024-lane run-time instance on a single band (half its lanes idle in every radix-16 pass)
    c.append(_case("rt1024_hook_l8192", 8192, 2049, [fused(0, 0, 1024)], env={"SDRHIP_K7_NT": "1024"}))
    # ---- fftconv_kernel: plans that do not start with two passes of which the first is radix 16 -------------------------------
    for L, taps in ((4, 2), (8, 3), (16, 5)):
        c.append(_case("plain_l%d" % L, L, taps, ["fftconv_kernel", ROLL], lens=[3 * L + 1, 1, 5 * L - 1]))
    c.append(_case("plain_l16_b3", 16, 5, ["fftconv_kernel"] * 3 + [ROLL], bands=3, lens=[49, 1, 79]))
    # ---- GenConv: one transform in one workgroup's LDS, radix passes 2 ... 13 ---------------------------------------------------
    gen = lambda f64: [typed("conv_kernel", f64)]
    c.append(_case("gen_f32_l1000", 1000, 301, gen(False)))
    c.append(_case("gen_f32_l1000_b3", 1000, 301, gen(False), bands=3))                  # (two LDS images: the bank's own path)
    c.append(_case("gen_f32_l12000", 12000, 3001, gen(False), C=2))
    c.append(_case("gen_f32_ola_literal_l2000", 2000, 1000, gen(False), mode=OLA, env={"SDRHIP_FFTCONV_LITERAL": "1"}, hop=1000))
    c.append(_case("gen_f64_l2048", 2048, 513, gen(True), f64=True))
    c.append(_case("gen_f64_l2000_b2", 2000, 301, gen(True), f64=True, bands=2))
    c.append(_case("gen_f64_ola_l1024", 1024, 512, gen(True), f64=True, mode=OLA, hop=512))
    # ---- BigConv: transforms beyond one workgroup's LDS (four-step: gather, product and scatter ride in its passes —
    # AnyFft::fuses()) and sizes with a prime factor above 13 (2018 = 2 x 1009: a chirp transform between the big_* passes) -----
    for f64 in (False, True):
        t = "f64" if f64 else "f32"
        L4 = 16384 if f64 else 32768                                                     # (128 KB of LDS: 8192 double2, 16384 float2)
        t2 = "double2" if f64 else "float2"
        four = ["fourstep_tile_kernel<%s%s>" % (t2, k) for k in (",gather", ",product", "", ",scatter")]
        g, m, s, h, f = (typed(k, f64) for k in ("big_gather_kernel", "big_mul_kernel", "big_scatter_kernel", "big_hist_kernel", "fft passes"))
        for bands in (1, 2):
            c.append(_case("big_%s_fourstep_l%d_b%d" % (t, L4, bands), L4, L4 // 8 + 1, four + [h], f64=f64, bands=bands, C=2,
                           lens=ragged(L4 - L4 // 8, 40000)))
            c.append(_case("big_%s_chirp_l2018_b%d" % (t, bands), 2018, 301, [g, f] + [m, f, s] * bands + [h], f64=f64, bands=bands))
    # ---- routes, not instances: what sdrhip_fir_create(FIR_CF32) and an overlap-add FilterNode plan end up on ----------------
    c.append(_case("route_fir_127_l2048", 2048, 127, [fused(11, 0, 128)], kind="fir", hop=1922))
    c.append(_case("route_fir_1025_l4096", 4096, 1025, [fused(12, 0, 256)], kind="fir", hop=3072))
    # 1025 taps with 1024 channels x 2 blocks >= 4 x 256 CUs: the pipelined 16384-point kernel (the one large case; every channel's
    # guard bands are checked, 8 channels spread over the range against the reference)
    c.append(_case("route_fir_1025_c1024_l16384", 16384, 1025, [fused(14, 0, 1024, 0, 2, 0)], kind="fir", C=1024, max_in=16384, hop=15360,
                   lens=[15363, 1, 16384], rows=[0, 1, 146, 293, 511, 512, 877, 1023]))
    # FilterNode(1000): a 2000-point overlap-add spectrum runs as 1000 taps of overlap-save on 4096 points
    c.append(_case("route_ola_n1000_l4096", 2000, 1000, [fused(12, 0, 256)], mode=OLA, hop=3096))
    c.append(_case("route_ola_n1024_keeps_l2048", 2048, 1024, [fused(11, 0, 128)], mode=OLA, hop=1024))
    c.append(_case("route_ola_bank_n1024_l2048", 2048, 1024, [fused(11, 1, 128)], mode=OLA, bands=3, hop=1024))
    assert len({k.id for k in c}) == len(c)
    return c


def _matrix():
    m = {}
    for case in cases():
        for call in case.expect:
            for k in call:
                if _TRACKED.match(k) and case.id not in m.setdefault(k, []):
                    m[k].append(case.id)
    return m


# instance -> the ids of the cases with a call that must run it
MATRIX = _matrix()

# compiled, never launched: instance -> (line of fftconv.hip that shuts it out, text that line holds, why)
EXCLUDED = {
    fused(0, 1, 1024): (1168, 'getenv("SDRHIP_K7_NT"); if (e && a.nb == 1)',
                        "never launched: fftconv.hip:1168 lets the SDRHIP_K7_NT hook change the lane count of single-band launches only, "
                        "and a bank launch (bands_per_launch, fftconv.hip:1139) has at most 8192 points, i.e. 512 lanes; 16384 points "
                        "never run as a bank"),
}


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


# ---- inputs and the float64 reference ----------------------------------------------------------------------------------------

def case_seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id))


def case_taps(case):
    """(what create takes, the float64 complex taps [bands, n_taps] the plan then convolves with).
    fftconv OLS: n_taps complex taps. OLA: the 2 n_taps-point spectrum of n_taps taps, rounded to the plan's precision — the
    reference takes its taps back from that spectrum in float64, as the library's ola_spectrum_to_taps does. fir: n_taps real
    coefficients; FIRFilter pairs alpha[order - 1] with the newest sample, so h[k] = alpha[order - 1 - k]."""
    rng = np.random.default_rng(case_seed(case))
    dt = np.float64 if case.f64 else np.float32
    M, B = case.n_taps, case.bands
    scale = 1.0 / np.sqrt(M)
    if case.kind == "fir":
        alpha = rng.standard_normal(M) * scale
        return alpha, alpha[::-1].astype(np.float32).astype(np.float64)[None, :] + 0j
    h = (rng.standard_normal((B, M, 2)) * scale).astype(dt)
    hc = h[..., 0].astype(np.float64) + 1j * h[..., 1]
    if case.mode == OLS:
        return [h[b] for b in range(B)], hc
    K = np.fft.fft(hc, 2 * M, axis=1)
    K = np.stack([K.real, K.imag], axis=-1).astype(dt)
    back = np.fft.ifft(K[..., 0].astype(np.float64) + 1j * K[..., 1], axis=1)[:, :M]
    return [K[b] for b in range(B)], back


def impulse_positions(lens, hop):
    """One unit impulse at offsets 0, 1, hop - 1, hop and hop + 1 of every block start of every call (block starts are relative
    to the call): every output position around a block seam then carries a tap value."""
    pos, start = set(), 0
    for n in lens:
        for b0 in range(0, n + hop, hop):
            for o in (-1, 0, 1):
                if start <= start + b0 + o < start + n and b0 + o >= 0:
                    pos.add(start + b0 + o)
        start += n
    return sorted(pos)


def case_inputs(case):
    """[("noise", x), ("impulses", x)], x [C, sum(lens), 2]: white noise of uniform scale; the impulse train, channel c's turned
    by i^c (exact in any precision) so that no two neighbouring channels carry the same samples."""
    rng = np.random.default_rng(case_seed(case) + 1)
    dt = np.float64 if case.f64 else np.float32
    n = sum(case.lens)
    noise = rng.standard_normal((case.C, n, 2), dtype=dt) * dt(0.3)
    imp = np.zeros((case.C, n, 2), dt)
    pos = impulse_positions(case.lens, case.hop)
    for c in range(case.C):
        r = 1j ** c
        imp[c, pos, 0], imp[c, pos, 1] = r.real, r.imag
    return [("noise", noise), ("impulses", imp)]


def reference(x, taps):
    """x [n, 2] -> the first n samples of x * taps in complex128 (an FFT product on a transform that holds the whole linear
    convolution: its own error is some 1e-15 of the largest output)."""
    xc = x[:, 0].astype(np.float64) + 1j * x[:, 1]
    n, m = len(xc), len(taps)
    size = 1 << int(np.ceil(np.log2(n + m - 1)))
    return np.fft.ifft(np.fft.fft(xc, size) * np.fft.fft(taps, size))[:n]
