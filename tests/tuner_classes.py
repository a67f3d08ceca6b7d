"""The tuner bank's matrix kernel (libsdr_amd/csrc/tuner.hip, tuner_i16_mfma_kernel) by plan class: a restatement of the
launcher's geometry (sdrhip_tuner_i16::plan), the classes of calls that geometry makes distinct, and the list of cases
tests/test_gpu_parity_tuner_classes.py runs, each tagged with the classes its calls reach. Plain Python, no GPU: the model
is held to the library on the device (plan_info equals it field for field), the coverage of the list is asserted by
tests/test_tuner_classes_complete.py.

A class is a tuple. ("ctw", n, kind): a call whose workgroups walk n channel tiles, reached WITHOUT SDRHIP_TUNER_CTW; kind =
"even" (ctiles % n == 0, C % 16 == 0), "ragged_wg" (the last workgroup walks fewer tiles), "partial_behind" (a last tile of
fewer than 16 channels behind other tiles of its workgroup); ("ctw", 1) for n = 1. ("geom", g, fm): a call of at least 100
time tiles at a decimation of kind g. ("S", s), ("S_pair", "16S" | "16S+1"), ("lds_max", fm), ("inst", epilogue, cu8): the
(epilogue, input kind) instance at more than one channel tile with ctw > 1, forced or not. ("cross", ...) pairs of the
small forced-ctw cross product."""
from collections import namedtuple

import numpy as np

CT, TR_STRIDE, HOT_COLS, HOT_MIN_D, HOT_MIN_IN, TI, TAPC = 16, 33, 512, 4, 512, 2048, 8
EPI_NAMES = ("none", "fm", "am", "usb")
CTWS = (1, 2, 4, 8)
GEOMS = ("d4", "divides512", "not_dividing512", "above256", "odd", "4mod8")
S_VALUES = (1, 2, 8, 33)
MIN_TILES = 100
ORACLE_ALL_ROWS_UP_TO = 64

FIELDS = ("hot", "S", "CG", "OG", "tiles", "ctiles", "ctw", "grid_y", "PLB", "lds")


def ceil_div(a, b):
    return -(-a // b)


def call_groups(n0, N, D):
    """(n_groups, n_out) of a call of N >= 1 samples from absolute index n0 (IQBaseBand closes its first window after D + 1
    samples)."""
    shift1 = 1 if D > 1 else 0
    group_of = lambda n: 0 if n < shift1 else (n - shift1) // D
    gf, gl = group_of(n0), group_of(n0 + N - 1)
    last_end = (gl + 1) * D - 1 + shift1
    n_groups = gl - gf + 1
    return n_groups, n_groups - (0 if last_end <= n0 + N - 1 else 1)


def model(C, order, D, fm, n0, N, hot_plan=True, force_ctw=None):
    """What sdrhip_tuner_i16_plan_info reports for a call of N >= 1 samples from absolute index n0. hot_plan: no channel's taps
    misfit the byte planes and SDRHIP_TUNER_PATH does not force the plain kernel."""
    S, OP = ceil_div(order, 16), ceil_div(order, TAPC) * TAPC
    ctiles = ceil_div(C, CT)
    ovl = 1 if fm else 0
    hot = bool(hot_plan and D >= HOT_MIN_D and N >= HOT_MIN_IN)
    CG = max(HOT_COLS // D, 4 if ovl else 1) if hot else TI // D
    OG = CG - ovl
    CGr = (CG + 3) & ~3
    tiles = ceil_div(call_groups(n0, N, D)[0], OG)
    if hot:
        ctw = 8
        while ctw > 1 and tiles * ceil_div(ctiles, ctw) < 1024:
            ctw >>= 1
        if force_ctw in CTWS:
            ctw = force_ctw
        cols = (CG * D + 31) & ~31
        PLB = (2 * (cols + 16 * S) + 16 + 15) & ~15
        grid_y = ceil_div(ctiles, ctw)
        lds = 1024 + 2 * PLB + CT * 20 + CT * CG * 8 + CT * 2 * CGr * 4 + 4 * CT * TR_STRIDE * 8
    else:
        ctw, PLB, grid_y = 0, 0, C
        lds = (TI + OP + 8 + 256 + 2 * CGr) * 4 + TI * 8
    return dict(hot=int(hot), S=S, CG=CG, OG=OG, tiles=tiles, ctiles=ctiles, ctw=ctw, grid_y=grid_y, PLB=PLB, lds=lds)


def cols_of(D, fm):
    """Time columns of a matrix-kernel tile, rounded to whole 32-column blocks."""
    return (max(HOT_COLS // D, 4 if fm else 1) * D + 31) & ~31


# ---- cases -----------------------------------------------------------------------------------------------------------------

# data: "tones" IQSigGen tones plus noise, "full" full-scale uniform samples (uniform bytes for cu8)
# taps: "design" bank_tunes' filters, "boundary" taps drawn from hot_classes.BOUNDARY with one channel at +-32639 on every tap
Case = namedtuple("Case", "id C order D epi cu8 N force_ctw data taps")


def _case(id, C, order, D, epi, cu8=False, N=65536, force_ctw=None, data="tones", taps="design"):
    return Case(id, C, order, D, epi, cu8, N, force_ctw, data, taps)


def call_lengths(case):
    """The three calls of a case: a ragged short one (the long calls then start at an odd absolute index and mid-group), N
    and N - 13."""
    return [333, case.N, case.N - 13]


CROSS_RES = (0, 1, 15)      # C mod 16
CROSS_ORDERS = (16, 17, 40, 127, 33, 255, 64, 21)
CROSS_D = (8, 4, 20, 5, 125, 16, 7, 300)


def _cross():
    """The small forced-ctw cross product, pairwise covering as test_gpu_parity_tuner._selection builds its list: every
    (ctw, instance) pair once, the residue of C walking with both indices so that it meets every ctw and every instance.
    C = 16 (ctw + 1) + residue: one full workgroup and a ragged one behind it (ctw + 1 or ctw + 2 channel tiles)."""
    out = []
    for a, ctw in enumerate(CTWS):
        for b in range(8):
            epi, cu8 = EPI_NAMES[b % 4], b >= 4
            res = CROSS_RES[(a + b) % 3]
            out.append(_case("x_ctw%d_%s_%s_r%d" % (ctw, epi, "cu8" if cu8 else "cs16", res), 16 * (ctw + 1) + res,
                             CROSS_ORDERS[(a + 3 * b) % 8], CROSS_D[(2 * a + b) % 8], epi, cu8, N=6000, force_ctw=ctw))
    return out


def cases():
    c = [
        # ---- ctw reached naturally: 65536 samples at /8 are 128 (129 from mid-group) time tiles ----------------------------
        _case("ctw2_even_c256", 256, 33, 8, "none"),
        _case("ctw2_raggedwg_c260", 260, 127, 8, "usb", cu8=True),
        _case("ctw2_partial_c250", 250, 64, 8, "am", cu8=True),
        _case("ctw4_even_c512", 512, 21, 8, "usb"),
        _case("ctw4_raggedwg_c530", 530, 33, 8, "none", cu8=True),
        _case("ctw4_partial_c500", 500, 40, 8, "am"),
        _case("ctw8_even_c1024", 1024, 33, 8, "none"),
        _case("ctw8_ragged_c1000", 1000, 48, 8, "fm", N=73728),   # (FM: 63 new groups per tile, 1024 workgroups need 128 tiles)
        # ---- tile geometry, >= 100 time tiles, with and without the overlap group; K steps 1, 2 (order 16 S, 16 S + 1), 8 ------
        _case("d4_o16_none", 17, 16, 4, "none"),
        _case("d4_o17_fm", 17, 17, 4, "fm", cu8=True),
        _case("d64_o127_am", 20, 127, 64, "am", cu8=True),
        _case("d64_o127_fm", 20, 127, 64, "fm"),
        _case("d20_o65_usb", 17, 65, 20, "usb"),
        _case("d20_o65_fm", 17, 65, 20, "fm"),
        _case("d125_o200_none", 17, 200, 125, "none", cu8=True),
        _case("d125_o200_fm", 17, 200, 125, "fm"),
        _case("d300_o301_am", 17, 301, 300, "am"),
        _case("d300_o301_fm", 17, 301, 300, "fm", N=98304),
        _case("d512_o33_none", 17, 33, 512, "none"),
        _case("d7_o48_usb", 17, 48, 7, "usb", cu8=True),
        _case("d7_o48_fm", 17, 48, 7, "fm"),
        # ---- the LDS maximum (decimation 4, 513 taps: 33 K steps) on full-scale data; 33 K steps on uniform bytes ---------------
        _case("ldsmax_none_boundary", 18, 513, 4, "none", N=20000, data="full", taps="boundary"),
        _case("ldsmax_fm", 18, 513, 4, "fm", N=20000, data="full"),
        _case("s33_d8_cu8_usb", 33, 513, 8, "usb", cu8=True, N=12000, data="full"),
    ]
    return c + _cross()


def case_models(case):
    """The model of each of the case's three calls (None for none: every length is >= 1)."""
    out, n0 = [], 0
    for n in call_lengths(case):
        out.append(model(case.C, case.order, case.D, case.epi == "fm", n0, n, force_ctw=case.force_ctw))
        n0 += n
    return out


def geom_kinds(D):
    k = set()
    if D == 4:
        k.add("d4")
    if 4 < D < 512 and 512 % D == 0:
        k.add("divides512")
    if 512 % D != 0 and 512 // D > 1:
        k.add("not_dividing512")
    if 256 < D <= 512:
        k.add("above256")
    if D % 2 == 1:
        k.add("odd")
    if D % 8 == 4:
        k.add("4mod8")
    return k


def classes_of(case):
    """The classes the case's calls reach."""
    out = set()
    fm = case.epi == "fm"
    for m in case_models(case):
        if not m["hot"]:
            continue
        ctw, ctiles = m["ctw"], m["ctiles"]
        last_wg = ctiles - (m["grid_y"] - 1) * ctw          # channel tiles the last workgroup walks
        if case.force_ctw is None:
            if ctw == 1:
                out.add(("ctw", 1))
            else:
                if ctiles % ctw == 0 and case.C % CT == 0:
                    out.add(("ctw", ctw, "even"))
                if ctiles % ctw != 0:
                    out.add(("ctw", ctw, "ragged_wg"))
                if case.C % CT != 0 and last_wg > 1:
                    out.add(("ctw", ctw, "partial_behind"))
        else:
            res = case.C % CT
            out.add(("cross", "ctw", ctw, "inst", case.epi, case.cu8))
            out.add(("cross", "ctw", ctw, "res", res))
            out.add(("cross", "inst", case.epi, case.cu8, "res", res))
        if ctw > 1 and ctiles > 1:
            out.add(("inst", case.epi, case.cu8))
        if m["tiles"] >= MIN_TILES:
            for g in geom_kinds(case.D):
                out.add(("geom", g, fm))
        out.add(("S", m["S"]))
        if case.order == 16 * m["S"]:
            out.add(("S_pair", "16S"))
        if case.order == 16 * (m["S"] - 1) + 1 and m["S"] > 1:
            out.add(("S_pair", "16S+1"))
        if case.D == HOT_MIN_D and case.order == 513:
            out.add(("lds_max", fm))
    return out


def required_classes():
    req = {("ctw", 1)}
    for n in CTWS[1:]:
        req |= {("ctw", n, k) for k in ("even", "ragged_wg", "partial_behind")}
    req |= {("geom", g, fm) for g in GEOMS for fm in (False, True)}
    req |= {("S", s) for s in S_VALUES}
    req |= {("S_pair", "16S"), ("S_pair", "16S+1"), ("lds_max", False), ("lds_max", True)}
    inst = [(e, cu8) for e in EPI_NAMES for cu8 in (False, True)]
    req |= {("inst",) + i for i in inst}
    req |= {("cross", "ctw", n, "inst") + i for n in CTWS for i in inst}
    req |= {("cross", "ctw", n, "res", r) for n in CTWS for r in CROSS_RES}
    req |= {("cross", "inst") + i + ("res", r) for i in inst for r in CROSS_RES}
    return req


def missing_classes(case_list):
    """Required classes no case of the list reaches; [] when the list is complete."""
    reached = set()
    for c in case_list:
        reached |= classes_of(c)
    return sorted(required_classes() - reached, key=repr)


# ---- the rows held to the oracle ------------------------------------------------------------------------------------------

def tile_edges(C, ct):
    """First and last live channel of channel tile ct."""
    return [CT * ct, min(CT * ct + CT - 1, C - 1)]


def edge_rows(C, m):
    """Of a matrix-kernel call with model m: the first and last live channel of every channel tile the first and the last
    workgroup walk, and of the tile at every position of one interior workgroup."""
    rows = set()
    ctw, gy, ctiles = m["ctw"], m["grid_y"], m["ctiles"]
    for wg in sorted({0, gy - 1, gy // 2}):
        for ci in range(ctw):
            ct = wg * ctw + ci
            if ct < ctiles:
                rows.update(tile_edges(C, ct))
    return rows


def oracle_rows(case, seed=20261017):
    """The rows of a case that are held to the oracle; every other row is compared bit for bit with the plain kernel's."""
    if case.C <= ORACLE_ALL_ROWS_UP_TO:
        return list(range(case.C))
    rows = {0}
    for m in case_models(case):
        if m["hot"]:
            rows |= edge_rows(case.C, m)
    rows |= set(int(r) for r in np.random.default_rng(seed).choice(case.C, 16, replace=False))
    return sorted(rows)
