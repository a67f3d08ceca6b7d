"""The IQBaseBand hot kernel's instance matrix (tests/hot_classes.py) is exactly what libsdrhip.so holds: every launchable
instance has a GPU case in tests/test_gpu_parity_hot_classes.py, and no instance is compiled without one. CPU only: the
host stubs come from `nm -C` of the library, the kernels themselves from `nm -C` of its gfx950 code objects."""
import shutil
import subprocess

import pytest

import hot_classes as hc
from libsdr_amd import abi

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def _nm(path):
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("`nm` (binutils) is not on PATH: the hot-kernel completeness check needs it to list the compiled instances")
    return subprocess.run([nm, "-C", str(path)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(host stubs, device kernels): {key: set of NW} each."""
    host = hc.parse_nm(_nm(abi.SO_PATH))
    d = tmp_path_factory.mktemp("co")
    so = shutil.copy(abi.SO_PATH, d / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", str(so)], capture_output=True, text=True, check=True, cwd=d)
    objs = sorted(d.glob("lib.so.*gfx950"))
    assert len(objs) >= 15, objs
    device = {}
    for o in objs:
        for k, nws in hc.parse_nm(_nm(o)).items():
            device.setdefault(k, set()).update(nws)
    return host, device


def mismatches(matrix, excluded, host, device):
    """What keeps the matrix from describing the build; [] when it does."""
    out = []
    names = lambda keys: sorted(hc.key_str(k) for k in keys)
    want = set(matrix) | set(excluded)
    if set(device) - want:
        out.append(("compiled, in no GPU case and not excluded", names(set(device) - want)))
    if set(matrix) - set(device):
        out.append(("in the matrix, not compiled", names(set(matrix) - set(device))))
    if set(excluded) - set(device):
        out.append(("excluded, but not compiled", names(set(excluded) - set(device))))
    if set(matrix) - set(host):
        out.append(("in the matrix, no host stub", names(set(matrix) - set(host))))
    if set(host) - want:
        out.append(("host stub of an instance outside the matrix", names(set(host) - want)))
    both = dict(matrix)
    both.update({k: v[0] for k, v in excluded.items()})
    for table in (host, device):
        bad = sorted(hc.key_str(k) + " NW=%s" % sorted(v) for k, v in table.items() if len(v) != 1 or (k in both and v != {both[k]}))
        if bad:
            out.append(("not exactly one NW, or another than the matrix's", bad))
    return out


def test_matrix_equals_compiled_instances(compiled):
    host, device = compiled
    assert len(hc.MATRIX) >= 1000, len(hc.MATRIX)
    problems = mismatches(hc.MATRIX, hc.EXCLUDED, host, device)
    assert not problems, problems


def test_every_exclusion_is_compiled_and_explained(compiled):
    _, device = compiled
    assert not set(hc.EXCLUDED) & set(hc.MATRIX)
    for k, (nw, why) in hc.EXCLUDED.items():
        assert k in device and device[k] == {nw}, hc.key_str(k)
        assert "iqbb_hot.hpp" in why and "never launched" in why, why


def test_mismatch_check_sees_a_new_table_entry(compiled):
    """A range added to a table without a compiled instance, or one compiled and missing from the matrix, is reported."""
    host, device = compiled
    one = next(iter(hc.MATRIX))
    fewer = {k: v for k, v in hc.MATRIX.items() if k != one}
    assert any("not excluded" in p[0] for p in mismatches(fewer, hc.EXCLUDED, host, device))
    more = dict(hc.MATRIX)
    more[(one[0], one[1], one[2], one[3], one[4], one[5], one[6], one[7], one[8] + 64)] = 4
    assert any("not compiled" in p[0] for p in mismatches(more, hc.EXCLUDED, host, device))
    steps, ranges, lo = hc._parse_tables(open(hc.HOT_HPP).read().replace("{{3, 3, 4}, ", "{{4, 1, 4}, {3, 3, 4}, "))
    assert ranges[9][0] == (4, 1, 4) and len(ranges[9]) == len(hc.RANGES[9]) + 1


def test_tables_parse():
    assert hc.STEPS == sorted(hc.RANGES)
    for S in hc.STEPS:
        for S0, NH, NW in hc.RANGES[S]:
            assert 0 <= S0 and S0 + NH <= S and NW in (4, 8, 16)
        for L0, NL in hc.LO_RANGES[S]:
            assert 0 <= L0 and L0 + NL <= S
    assert hc.LO_RANGES[9][0] == (1, 7)


@pytest.mark.parametrize("case", hc.cases(), ids=lambda c: c[0])
def test_taps_for_pick_the_case_range(case):
    """The tap builder lands every GPU case's taps in that case's high and low ranges (the model of pick_hot_ranges;
    the GPU test asserts that plan_info agrees)."""
    cid, form, kind, S, R, L, _ = case
    order = hc.largest_order(S, kind)
    taps = hc.taps_for(S, kind, order, range(R[0], R[0] + R[1]), range(L[0], L[0] + L[1]), seed=hc.case_seed(cid))
    ah, al = hc.masks(S, kind, taps)
    assert hc.pick(S, ah, al, form == hc.D8 and kind != hc.REAL)[1:] == (R, L)
    vals = set(taps.ravel().tolist())
    assert set(hc.BOUNDARY) <= vals, (cid, set(hc.BOUNDARY) - vals)


def test_cases_cover_the_matrix():
    covered = set()
    for cid, form, kind, S, R, L, per_rot in hc.cases():
        for rot, epis in per_rot.items():
            for epi in epis:
                covered.add((hc.KERNEL[form], S, R[0], R[1], rot, epi, kind) + tuple(L))
    assert covered == set(hc.MATRIX)
    assert len(hc.cases()) == len({c[0] for c in hc.cases()})


def test_mask_model_edges():
    """Hand-checked masks: a tap that feeds one step, a negated -128 (high plane +1), a multiple of 256 (no low plane)."""
    t = [[0, 0]] * 129
    t = [list(x) for x in t]
    t[16] = [5, 0]                         # window index 16 of 9 steps: step 1 alone
    assert hc.masks(9, hc.CS16, t) == (0, 0b10)
    t[16] = [0, -128]                      # -ki = 128: a high byte
    assert hc.masks(9, hc.CS16, t) == (0b10, 0b10)
    t[16] = [-128, 0]                      # kr = -128 alone fits the low plane
    assert hc.masks(9, hc.CS16, t) == (0, 0b10)
    t[16] = [512, 0]
    assert hc.masks(9, hc.CS16, t) == (0b10, 0)
    t[16] = [0, 0]
    t[15] = [1, 0]                         # index 15: steps 0 and 1
    assert hc.masks(9, hc.CS16, t) == (0, 0b11)
    r = [[0, 0] for _ in range(81)]
    r[40] = [0, 300]                       # real, 3 steps: index 40 = 32 + 8 feeds step 1 alone
    assert hc.masks(3, hc.REAL, r) == (0b10, 0b10)
    r[40] = [0, 0]
    r[20] = [1, 0]                         # 20: steps 0 (-15 ... 31) and 1 (17 ... 63)
    assert hc.masks(3, hc.REAL, r) == (0, 0b11)
