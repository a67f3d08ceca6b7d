"""The case list of tests/tuner_classes.py reaches every plan class of the tuner bank's matrix kernel, and the model the
classes are computed from has the launcher's edge values. CPU only; the model itself is held to the library on the GPU
(tests/test_gpu_parity_tuner_classes.py asserts that plan_info equals it field for field in every case)."""
import pytest

import tuner_classes as tc


def test_cases_cover_every_class():
    cases = tc.cases()
    assert len(cases) == len({c.id for c in cases})
    assert tc.missing_classes(cases) == []


def test_coverage_check_sees_a_removed_class():
    """Without the cases that reach a class, the check names that class (for every required class)."""
    cases = tc.cases()
    for cls in sorted(tc.required_classes(), key=repr):
        fewer = [c for c in cases if cls not in tc.classes_of(c)]
        assert len(fewer) < len(cases), cls
        assert cls in tc.missing_classes(fewer), cls
    assert len(tc.missing_classes([])) == len(tc.required_classes())


def test_natural_cases_are_not_forced():
    """Every class but the cross product's (and the instances') is reached at a natural shape: no forced ctw."""
    natural = [c for c in tc.cases() if c.force_ctw is None]
    left = tc.missing_classes(natural)
    assert all(cls[0] in ("cross", "inst") for cls in left), left
    assert len(natural) >= 20 and len(tc.cases()) - len(natural) == 32


@pytest.mark.parametrize("cid,ctw,ctiles,last_wg,last_tile", [
    ("ctw2_even_c256", 2, 16, 2, 16), ("ctw2_raggedwg_c260", 2, 17, 1, 4), ("ctw2_partial_c250", 2, 16, 2, 10),
    ("ctw4_even_c512", 4, 32, 4, 16), ("ctw4_raggedwg_c530", 4, 34, 2, 2), ("ctw4_partial_c500", 4, 32, 4, 4),
    ("ctw8_even_c1024", 8, 64, 8, 16), ("ctw8_ragged_c1000", 8, 63, 7, 8)])
def test_natural_ctw_cases(cid, ctw, ctiles, last_wg, last_tile):
    """The issue's candidates by arithmetic, confirmed against the model: both long calls of the case."""
    case = {c.id: c for c in tc.cases()}[cid]
    short, *long_calls = tc.case_models(case)
    assert short["hot"] == 0 and short["ctw"] == 0 and short["grid_y"] == case.C
    for m in long_calls:
        assert (m["hot"], m["ctw"], m["ctiles"]) == (1, ctw, ctiles), m
        assert m["tiles"] >= tc.MIN_TILES
        assert ctiles - (m["grid_y"] - 1) * ctw == last_wg
    assert case.C - 16 * (ctiles - 1) == last_tile


def test_geometry_cases_have_100_tiles():
    for c in tc.cases():
        if c.force_ctw is None and c.N >= 65536:
            assert all(m["tiles"] >= tc.MIN_TILES for m in tc.case_models(c)[1:]), c.id


def test_model_ctw_thresholds():
    """128 time tiles (65536 samples at /8 from index 0): 1024 workgroups need 8 rows of workgroups."""
    ctw = lambda C, N=65536: tc.model(C, 127, 8, False, 0, N)["ctw"]
    assert tc.model(224, 127, 8, False, 0, 65536)["tiles"] == 128
    assert (ctw(224), ctw(225)) == (1, 2)       # 14 | 15 channel tiles
    assert (ctw(448), ctw(449)) == (2, 4)       # 28 | 29
    assert (ctw(896), ctw(897)) == (4, 8)       # 56 | 57
    assert tc.model(1024, 127, 8, False, 0, 65024)["tiles"] == 127
    assert (ctw(1024, 65024), ctw(1024)) == (4, 8)
    assert (ctw(8192, 1024), ctw(8192, 2048), ctw(8192, 8192)) == (1, 2, 8)   # 512 channel tiles over 2, 4, 16 time tiles
    # forced: only ctw and the grid change
    a, b = tc.model(1000, 127, 8, False, 0, 65536), tc.model(1000, 127, 8, False, 0, 65536, force_ctw=1)
    assert (b["ctw"], b["grid_y"]) == (1, 63) and (a["ctw"], a["grid_y"]) == (8, 8)
    assert {k: v for k, v in a.items() if k not in ("ctw", "grid_y")} == {k: v for k, v in b.items() if k not in ("ctw", "grid_y")}
    assert tc.model(1000, 127, 8, False, 0, 65536, force_ctw=3) == a


@pytest.mark.parametrize("D,plain,fm", [(4, 128, 128), (128, 4, 4), (129, 3, 4), (256, 2, 4), (257, 1, 4), (512, 1, 4)])
def test_model_groups_per_tile(D, plain, fm):
    m0, m1 = tc.model(16, 127, D, False, 0, 65536), tc.model(16, 127, D, True, 0, 65536)
    assert (m0["CG"], m0["OG"]) == (plain, plain)
    assert (m1["CG"], m1["OG"]) == (fm, fm - 1)


def test_model_columns():
    assert tc.cols_of(4, False) == 512 and tc.cols_of(125, False) == 512 and tc.cols_of(125, True) == 512
    assert tc.cols_of(20, True) == 512 and tc.cols_of(300, False) == 320 and tc.cols_of(300, True) == 1216
    assert tc.cols_of(512, True) == 2048 and tc.cols_of(7, False) == 512


def test_model_hot_or_plain():
    hot = lambda **k: tc.model(**dict(dict(C=20, order=127, D=8, fm=False, n0=0, N=4096), **k))["hot"]
    assert hot() == 1 and hot(N=512) == 1 and hot(N=511) == 0
    assert hot(D=4) == 1 and hot(D=3) == 0 and hot(D=512) == 1
    assert hot(hot_plan=False) == 0
    m = tc.model(20, 127, 8, False, 0, 511)
    assert (m["CG"], m["ctw"], m["grid_y"], m["PLB"], m["lds"]) == (256, 0, 20, 0, (2048 + 128 + 8 + 256 + 512) * 4 + 2048 * 8)


def test_model_lds_maximum():
    """Decimation 4 and 513 taps need the most LDS of all matrix-kernel plans, below the launcher's bound of 64 KB."""
    worst = max(((tc.model(16, 16 * S, D, fm, 0, 65536)["lds"], D, S, fm) for D in range(4, 513) for S in range(1, 34) for fm in (False, True)))
    assert worst[:3] == (55200, 4, 33)
    for fm in (False, True):
        m = tc.model(18, 513, 4, fm, 0, 20000)
        assert (m["S"], m["CG"], m["PLB"], m["lds"]) == (33, 128, 2096, 55200)
        assert m["lds"] <= 64 * 1024
    plain = max(tc.model(16, 513, D, False, 0, 100)["lds"] for D in range(1, 513))
    assert plain == tc.model(16, 513, 1, False, 0, 100)["lds"] <= 64 * 1024


def test_oracle_rows():
    by_id = {c.id: c for c in tc.cases()}
    assert tc.oracle_rows(by_id["d4_o16_none"]) == list(range(17))
    c = by_id["ctw8_ragged_c1000"]
    rows = tc.oracle_rows(c)
    # workgroup 0: tiles 0 ... 7; the last one (7): tiles 56 ... 62, the last tile holds channels 992 ... 999; interior (4): 32 ... 39
    want = {0} | {16 * t + o for t in list(range(8)) + list(range(32, 40)) + list(range(56, 62)) for o in (0, 15)} | {992, 999}
    assert want <= set(rows) and len(rows) <= len(want) + 16 and rows == sorted(set(rows))
    assert rows == tc.oracle_rows(c)                                   # (the drawn rows are fixed)
    c = by_id["ctw2_raggedwg_c260"]
    assert {0, 15, 16, 31, 256, 259} <= set(tc.oracle_rows(c))        # the last workgroup walks tile 16 alone: 4 channels
