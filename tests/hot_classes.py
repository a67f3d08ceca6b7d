"""The IQBaseBand hot kernel's instance matrix and a tap builder for it — TEST CODE, a plain helper module (not a test file).

The hot kernel (libsdr_amd/csrc/iqbb_hot.hpp) is compiled as one template instance per (form, S, high-plane K-step range,
low-plane range, rotation, epilogue, input kind); the host picks one at run time from the taps' byte-plane masks. This
module restates that choice in Python:

* `RANGES` / `LO_RANGES`: the tables hot_ranges_* / hot_lo_ranges_* parsed out of iqbb_hot.hpp, so that a new table entry
  shows up here (and in the tests built on it) without an edit;
* `launchable()`: the instances the host can launch — hot_class, hot_has_epi, the `inside` rule of HotClass::launch and
  hot_sd_range_waves restated — keyed `(kernel, S, S0, NH, ROT, EPI, IN, L0, NL)` (the kernels' template arguments without
  NW) with NW as the value; `EXCLUDED`: instances that are compiled but never launched, each with its reason;
* `masks()` / `pick()`: a model of load_taps' ah_mask / al_mask and of pick_hot_ranges (iqbb_i16.hip);
* `taps_for()`: int32 taps whose high- and low-byte masks are exactly the K steps asked for.

tests/test_hot_classes_complete.py checks the matrix against the instances compiled into libsdrhip.so;
tests/test_gpu_parity_hot_classes.py runs every entry against the oracle.
"""
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT_HPP = os.path.join(ROOT, "libsdr_amd", "csrc", "iqbb_hot.hpp")

# input kinds, forms and epilogues (iqbb_hot.hpp, iqbb_common.hpp, include/sdrhip.h)
CS16, CU8, REAL, CS8 = 0, 1, 2, 3
KINDS = {CS16: "cs16", CU8: "cu8", REAL: "real", CS8: "cs8"}
D8, ANYD, SD = 0, 1, 2
FORMS = {D8: "d8", ANYD: "anyd", SD: "sd"}
KERNEL = {D8: "iqbb_hot_kernel", ANYD: "iqbb_hot_anyd_kernel", SD: "iqbb_hot_sd_kernel"}
EPI_NONE, EPI_FM, EPI_AM, EPI_USB, EPI_PARTIAL = 0, 1, 2, 3, 4
EPIS = (EPI_NONE, EPI_FM, EPI_AM, EPI_USB, EPI_PARTIAL)

# values at the byte boundaries of the planes (v = 256 ah + al, al in [-128, 128)): 32639 is the largest magnitude whose
# v and -v both keep ah within int8 (check_taps); 32640 does not
BOUNDARY = (127, -127, 128, -128, -129, 255, -255, 256, -256, 32639, -32639)
PLANE_LIMIT = 32639


def _parse_tables(text):
    steps = [int(v) for v in re.search(r"constexpr int hot_steps\[\]\s*=\s*\{([^}]*)\}", text).group(1).split(",")]
    ranges, lo = {}, {}
    for m in re.finditer(r"constexpr HotRange hot_ranges_(\d+)\[\]\s*=\s*\{(.*?)\};", text, re.S):
        ranges[int(m.group(1))] = [tuple(int(v) for v in e) for e in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", m.group(2))]
    for m in re.finditer(r"constexpr HotLoRange hot_lo_ranges_(\d+)\[\]\s*=\s*\{(.*?)\};", text, re.S):
        lo[int(m.group(1))] = [tuple(int(v) for v in e) for e in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*\}", m.group(2))]
    assert sorted(ranges) == sorted(steps), (steps, sorted(ranges))
    for S in steps:
        assert ranges[S] and ranges[S][-1][:2] == (0, S), "the last high-plane range of %d steps must cover every step" % S
        lo.setdefault(S, [(0, S)])   # hot_lo_full<S>
        assert lo[S][-1] == (0, S), "the last low-plane range of %d steps must cover every step" % S
    return steps, ranges, lo


def load_tables(path=HOT_HPP):
    with open(path) as f:
        return _parse_tables(f.read())


STEPS, RANGES, LO_RANGES = load_tables()


# ---- which classes and instances exist (iqbb_hot.hpp) --------------------------------------------------------------------
def hot_class(form, S, kind):
    if kind == REAL:
        return S in (3, 5, 9)
    if kind == CS8:
        return form != SD and S in (2, 3, 5, 9)
    return S in (2, 3, 5, 9, 17) or (S == 33 and form != SD)


def hot_has_epi(form, kind, epi):
    if epi == EPI_PARTIAL:
        return form == ANYD and kind not in (REAL, CS8)
    return kind != CS8 or epi in (EPI_FM, EPI_NONE)


def _one_plane(kind):
    return kind in (CU8, CS8)


def _halo(S, kind):
    return 32 * S - 16 if kind == REAL else 16 * (S - 1)


def _win(S, kind):
    return 512 + _halo(S, kind) + (16 if kind == REAL else 0)


def _plb(S, kind):
    return _win(S, kind) if kind == REAL else 2 * _win(S, kind) + 32


def _bufb(S, kind):
    return _plb(S, kind) if _one_plane(kind) else 2 * _plb(S, kind)


def _lds_bytes(S, NH, kind, NW, wide):
    return (4096 if wide else 1024) + (S + NH) * 1024 + NW * 2 * _bufb(S, kind)


def _lds_cap(NW, S=0):
    return 163840 if S >= 33 else 40960 if NW == 4 else 81920 if NW == 8 else 163840


def _sd_extra(S, kind, rot, NW):
    return (0 if _bufb(S, kind) >= 2048 else NW * 2048) + (0 if rot else NW * 2048)


def _sd_fits(S, NH, kind, rot, NW):
    return _lds_bytes(S, NH, kind, NW, False) + _sd_extra(S, kind, rot, NW) <= _lds_cap(NW)


def hot_sd_range_waves(S, rng, kind, rot):
    """The small-D form's workgroup for a range (hot_sd_nw from the table's NW; real input: 4 waves only); 0: none fits."""
    _, NH, NW = rng
    nw, found = NW, 0
    while nw <= 16:
        if _sd_fits(S, NH, kind, rot, nw):
            found = nw
            break
        nw *= 2
    return found if kind != REAL or found == 4 else 0


def range_pairs(form, S, kind):
    """(range index, low range index or None, (S0, NH, NW), (L0, NL)) for every pair HotClass::launch can turn into template
    arguments, duplicates (a pair whose high range is not inside the low one runs every step) dropped."""
    out, seen = [], set()
    for ri, R in enumerate(RANGES[S]):
        los = list(enumerate(LO_RANGES[S])) if form == D8 and kind in (CS16, CU8) else [(None, (0, S))]
        for li, L in los:
            inside = R[0] >= L[0] and R[0] + R[1] <= L[0] + L[1]
            LL = L if inside else (0, S)
            if (R, LL) in seen:
                continue
            seen.add((R, LL))
            out.append((ri, li, R, LL))
    return out


def launchable():
    """{(kernel, S, S0, NH, ROT, EPI, IN, L0, NL): NW} — every instance hot_launch can reach."""
    m = {}
    for form in (D8, ANYD, SD):
        for S in STEPS:
            for kind in (CS16, CU8, REAL, CS8):
                if not hot_class(form, S, kind):
                    continue
                for _, _, R, L in range_pairs(form, S, kind):
                    for rot in (False, True):
                        nw = hot_sd_range_waves(S, R, kind, rot) if form == SD else R[2]
                        if nw == 0:
                            continue
                        for epi in EPIS:
                            if hot_has_epi(form, kind, epi):
                                m[(KERNEL[form], S, R[0], R[1], rot, epi, kind) + tuple(L)] = nw
    return m


def _excluded():
    """Instances that are compiled and never launched: {key: (NW, reason)}."""
    ex = {}
    # iqbb_hot.hpp, comment above hot_launch_form: "(The any-D list holds HOT_EPI_PARTIAL for real input too: those kernels
    # are compiled, never launched.)" — hot_launch_form's hipFuncSetAttribute lambda takes every epilogue's kernel address,
    # PARTIAL included, for every input kind but complex<int8>; hot_has_epi keeps real input out of the launch. (The setter
    # runs only for 8- and 16-wave workgroups, never for real input: the host build drops its stubs, the gfx950 code
    # objects keep the kernels.)
    for S in STEPS:
        if not hot_class(ANYD, S, REAL):
            continue
        for R in RANGES[S]:
            for rot in (False, True):
                ex[(KERNEL[ANYD], S, R[0], R[1], rot, EPI_PARTIAL, REAL, 0, S)] = (
                    R[2], "iqbb_hot.hpp hot_launch_form: any-D real-input HOT_EPI_PARTIAL kernels are compiled (attribute setter), never launched")
    return ex


MATRIX = launchable()
EXCLUDED = _excluded()


def key_str(k):
    return "%s<S=%d,S0=%d,NH=%d,ROT=%d,EPI=%d,IN=%s,L0=%d,NL=%d>" % (k[0], k[1], k[2], k[3], int(k[4]), k[5], KINDS[k[6]], k[7], k[8])


# ---- nm: the instances compiled into the library -------------------------------------------------------------------------
_STUB = re.compile(r"\b(?:__device_stub__)?(iqbb_hot(?:_anyd|_sd)?_kernel)<([^<>]*)>")


def parse_nm(text):
    """{(kernel, S, S0, NH, ROT, EPI, IN, L0, NL): set of NW} from `nm -C` output (host stubs and handles alike)."""
    got = {}
    for line in text.splitlines():
        m = _STUB.search(line)
        if not m:
            continue
        args = [a.strip() for a in m.group(2).split(",")]
        v = [a == "true" if a in ("true", "false") else int(a) for a in args]
        if m.group(1) == "iqbb_hot_kernel":
            assert len(v) == 9, line
            S, S0, NH, rot, epi, kind, nw, L0, NL = v
        else:
            assert len(v) == 7, line
            S, S0, NH, rot, epi, kind, nw = v
            L0, NL = 0, S
        got.setdefault((m.group(1), S, S0, NH, bool(rot), epi, kind, L0, NL), set()).add(nw)
    return got


# ---- tap geometry, masks and the range pick (iqbb_i16.hip load_taps / pick_hot_ranges) ----------------------------------
def window(S, kind):
    """Taps in the matrix part's window (OPm): the plan's taps sit at its END, zero-padded at the front."""
    return 32 * S - 15 if kind == REAL else 16 * (S - 1) + 1


def feeds(S, kind, w):
    """K steps that window index w feeds. Complex input: tap w is interleaved element 2w, 2w+1, and byte j of step s, lane
    (t, hh) reads element 32s + 16hh + j - 2t — steps ceil((w-15)/16) ... floor((w+15)/16). Real input (path 4): element
    32s + 16hh + j - t, t in 0 ... 15 — steps with 32s - 15 <= w <= 32s + 31."""
    if kind == REAL:
        return [s for s in range(S) if 32 * s - 15 <= w <= 32 * s + 31]
    return [s for s in range(S) if 16 * s - 15 <= w <= 16 * s + 15]


def anchor(S, kind, s):
    """A window index that feeds step s alone."""
    return 32 * s + 8 if kind == REAL else 16 * s


def _split(v):
    v = np.asarray(v, np.int64)
    al = ((v + 128) & 255) - 128
    return (v - al) >> 8, al


def masks(S, kind, taps):
    """(ah_mask, al_mask) as load_taps computes them: bit s where a high- / low-byte tap fragment of K step s is not zero."""
    taps = np.asarray(taps, np.int64).reshape(-1, 2)
    order, OPm = taps.shape[0], window(S, kind)
    assert order <= OPm
    pad = OPm - order
    ah, al = 0, 0
    for i in range(order):
        kr, ki = int(taps[i, 0]), int(taps[i, 1])
        vals = (kr, ki) if kind == REAL else (kr, -ki, ki)   # (complex: the interleaved vectors hold kr, -ki and ki, kr)
        h, lo = _split(vals)
        hi_any, lo_any = bool(np.any(h != 0)), bool(np.any(lo != 0))
        for s in feeds(S, kind, pad + i):
            if hi_any:
                ah |= 1 << s
            if lo_any:
                al |= 1 << s
    return ah, al


def _covers(mask, first, n):
    return mask & ~(((1 << n) - 1) << first) == 0


def pick(S, ah, al, trim):
    """pick_hot_ranges: (range index, (S0, NH, NW), (L0, NL)); trim: path 1 (the /8 plans of complex input) also picks a
    low-plane range — what plan_info reports, whichever kernel then runs. None where no range covers ah."""
    rg = RANGES[S]
    ri = next((r for r in range(len(rg)) if _covers(ah, rg[r][0], rg[r][1])), None)
    if ri is None:
        return None
    R = rg[ri]
    if not trim:
        return ri, R, (0, S)
    lr = LO_RANGES[S]
    for r in range(len(lr)):
        inside = R[0] >= lr[r][0] and R[0] + R[1] <= lr[r][0] + lr[r][1]
        if (_covers(al, lr[r][0], lr[r][1]) and inside) or r == len(lr) - 1:
            return ri, R, lr[r]


def steps_mask(steps):
    m = 0
    for s in steps:
        m |= 1 << s
    return m


def reachable(S, kind, order):
    """The K steps the taps of a plan of `order` can feed at all (behind the zero front pad)."""
    OPm = window(S, kind)
    return sorted({s for w in range(OPm - order, OPm) for s in feeds(S, kind, w)})


def largest_order(S, kind):
    return window(S, kind)


def smallest_order(S, kind):
    """The smallest order that lands in the class of S K steps (the plan's class rules, iqbb_i16.hip create_baseband)."""
    if kind == REAL:
        return {3: 1, 5: 82, 9: 146}[S]
    prev = [s for s in STEPS if s < S]
    return window(prev[-1], kind) + 1 if prev else 1


def taps_for(S, kind, order, hi_steps, lo_steps, seed=0, anchors=True):
    """int32 taps [order, 2] whose high-byte mask is exactly `hi_steps` and low-byte mask exactly `lo_steps` (hi inside lo).

    Window indices that feed only high-range steps hold general values (random over the whole plane range, the byte
    boundary values among them); those that feed only low-range steps hold low-plane-only values (|v| < 128); the others
    are zero. The first and last step of the high range each get a tap with a multiple of 256 (high plane alone) on the
    index that feeds that step alone; every low-range step outside the high range gets a low-plane-only tap there
    (anchors=False: not — short filters behind a long front pad, whose every tap may be the only one of its step)."""
    hi, lo = sorted(set(hi_steps)), sorted(set(lo_steps))
    assert set(hi) <= set(lo), (hi, lo)
    OPm = window(S, kind)
    pad = OPm - order
    assert 0 <= pad
    rng = np.random.default_rng(seed)
    t = np.zeros((order, 2), np.int64)
    general = []
    for i in range(order):
        f = set(feeds(S, kind, pad + i))
        if f <= set(hi):
            t[i] = rng.integers(-PLANE_LIMIT, PLANE_LIMIT + 1, 2)
            general.append(i)
        elif f <= set(lo):
            t[i] = rng.integers(-127, 128, 2)
    # the first and last step of the high range: high plane alone; the low-range steps outside it: low plane alone
    fixed = set()
    if hi and anchors:
        for s in (hi[0], hi[-1]):
            i = anchor(S, kind, s) - pad
            if 0 <= i < order:
                t[i] = (256 * int(rng.choice([-127, -3, 1, 5, 127])), 256 * int(rng.choice([-126, -1, 2, 126])))
                fixed.add(i)
    for s in lo:
        i = anchor(S, kind, s) - pad
        if anchors and s not in hi and 0 <= i < order:
            t[i] = (int(rng.choice([-127, -1, 3, 127])), int(rng.choice([-126, -2, 1, 127])))
            fixed.add(i)
    # the byte boundaries, on general slots spread over the window (both components)
    free = [i for i in general if i not in fixed]
    if free:
        picks = np.linspace(0, len(free) - 1, num=min(len(free), len(BOUNDARY))).round().astype(int)
        for k, p in enumerate(picks):
            t[free[p]] = (BOUNDARY[k % len(BOUNDARY)], BOUNDARY[(k + 5) % len(BOUNDARY)])
    ah, al = masks(S, kind, t)
    assert (ah, al) == (steps_mask(hi), steps_mask(lo)), ("taps_for", S, KINDS[kind], order, hi, lo, bin(ah), bin(al))
    assert np.abs(t).max() <= PLANE_LIMIT
    return t.astype(np.int32)


# ---- the GPU cases: one per (form, kind, S, high range[, low range]) ----------------------------------------------------
def cases():
    """[(id, form, kind, S, (S0, NH, NW), (L0, NL), {rot: [epilogues]})] covering MATRIX; the PARTIAL instances ride in the
    any-D cases of complex<int16> / complex<uint8>."""
    out = []
    for form in (D8, ANYD, SD):
        for kind in (CS16, CU8, CS8, REAL):
            for S in STEPS:
                if not hot_class(form, S, kind):
                    continue
                for ri, li, R, L in range_pairs(form, S, kind):
                    per_rot = {}
                    for rot in (False, True):
                        e = [epi for epi in EPIS if (KERNEL[form], S, R[0], R[1], rot, epi, kind) + tuple(L) in MATRIX]
                        if e:
                            per_rot[rot] = e
                    if not per_rot:
                        continue
                    cid = "%s-%s-S%d-h%d.%d" % (FORMS[form], KINDS[kind], S, R[0], R[1]) + ("-l%d.%d" % L if li is not None else "")
                    out.append((cid, form, kind, S, R, L, per_rot))
    return out


def classes():
    """[(form, kind, S)] of every compiled class."""
    return [(f, k, S) for f in (D8, ANYD, SD) for k in (CS16, CU8, CS8, REAL) for S in STEPS if hot_class(f, S, k)]


def case_seed(name):
    """A seed of its own for every case id, the same in every run."""
    return zlib.crc32(name.encode()) & 0xffffff
