"""The FFT convolution's instance table (tests/fftconv_classes.py) is exactly what libsdrhip.so holds: every compiled
fftconv_fused_kernel<...>, fftconv_kernel, conv_kernel<...> and big_*_kernel<...> has a GPU case in
tests/test_gpu_parity_fftconv_classes.py that must report it through last_kernels(), or a reason in EXCLUDED that names the
line of fftconv.hip which keeps it from being launched; nothing is listed that is not compiled. CPU only: the kernels come
from `nm -C` of the library's gfx950 code objects."""
import re
import shutil
import subprocess

import pytest

import fftconv_classes as fc
from libsdr_amd import abi

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def _nm(path):
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("`nm` (binutils) is not on PATH: the completeness check needs it to list the compiled instances")
    return subprocess.run([nm, "-C", str(path)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    d = tmp_path_factory.mktemp("co")
    so = shutil.copy(abi.SO_PATH, d / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", str(so)], capture_output=True, text=True, check=True, cwd=d)
    objs = sorted(d.glob("lib.so.*gfx950"))
    assert len(objs) >= 15, objs
    got = set()
    for o in objs:
        got |= fc.parse_nm(_nm(o))
    return got


def test_matrix_equals_compiled_instances(compiled):
    assert len(compiled) >= 30, sorted(compiled)
    problems = fc.mismatches(fc.MATRIX, fc.EXCLUDED, compiled)
    assert not problems, problems


def test_every_instance_has_a_case_that_names_it():
    ids = {c.id for c in fc.cases()}
    for name, case_ids in fc.MATRIX.items():
        assert case_ids and set(case_ids) <= ids, name
    assert all(len(c.lens) == 3 and len(c.expect) == 3 and all(c.expect) for c in fc.cases())


def test_every_exclusion_is_compiled_and_explained(compiled):
    src = open(fc.FFTCONV_HIP).read().splitlines()
    for name, (line, text, why) in fc.EXCLUDED.items():
        assert name in compiled and name not in fc.MATRIX, name
        assert "fftconv.hip:%d" % line in why and "never launched" in why, why
        assert text in src[line - 1], (name, line, src[line - 1])
        for other in re.findall(r"fftconv\.hip:(\d+)", why):
            assert 1 <= int(other) <= len(src), other


def test_mismatch_check_sees_an_invented_and_a_removed_instance(compiled):
    """An instance added to the table that is not compiled, and a compiled one missing from it, are each reported."""
    one = fc.fused(12, 1, 256)
    assert one in fc.MATRIX and one in compiled
    fewer = {k: v for k, v in fc.MATRIX.items() if k != one}
    assert ("compiled, in no GPU case and not excluded", [one]) in fc.mismatches(fewer, fc.EXCLUDED, compiled)
    more = dict(fc.MATRIX)
    invented = fc.fused(12, 1, 512)
    more[invented] = ["ct12_b3"]
    assert ("in the matrix, not compiled", [invented]) in fc.mismatches(more, fc.EXCLUDED, compiled)
    gone = dict(fc.EXCLUDED)
    gone[invented] = (1, "", "never launched")
    assert ("excluded, but not compiled", [invented]) in fc.mismatches(fc.MATRIX, gone, compiled)
    assert fc.mismatches(fc.MATRIX, fc.EXCLUDED, compiled | {"big_other_kernel<float2>"})[0][1] == ["big_other_kernel<float2>"]


def test_parse_nm_spelling():
    text = "\n".join([
        "0000000000016d00 R void (anonymous namespace)::fftconv_fused_kernel<14, false, 1024, false, 4, 2>((anonymous namespace)::ConvArgs) [clone .kd]",
        "0000000000018b00 T (anonymous namespace)::fftconv_kernel((anonymous namespace)::ConvArgs)",
        "0000000000129800 T void sdrhip::fftgen::conv_kernel<HIP_vector_type<double, 2u> >(sdrhip::fftgen::GenConvArgs<HIP_vector_type<double, 2u> >)",
        "0000000000017800 R void (anonymous namespace)::big_gather_kernel<HIP_vector_type<float, 2u> >(HIP_vector_type<float, 2u> const*, long) [clone .kd]",
        "000000000001af00 T (anonymous namespace)::hist_roll_kernel(HIP_vector_type<float, 2u> const*, long)",
        "0000000000006d00 T void (anonymous namespace)::fir_cf32_rt_kernel<4, 8>((anonymous namespace)::Fir32Args)"])
    assert fc.parse_nm(text) == {fc.fused(14, 0, 1024, 0, 4, 2), "fftconv_kernel", "conv_kernel<double2>", "big_gather_kernel<float2>"}


def test_case_shapes():
    """The calls of a case: one that ends just behind a block seam, one shorter than the history, one more than a block long;
    the 16-byte pipelined cases keep every length and the row stride even; the pipelined cases have more units than workgroups
    in every call that must run the pipelined form."""
    for c in fc.cases():
        assert c.lens[0] > c.hop and c.lens[1] <= 2 and c.lens[2] > 1 and sum(c.lens) <= 50000 and max(c.lens) <= c.max_in, c.id
        assert 2 <= c.C <= 4 or c.id.endswith("_c8") and c.C == 8 or c.id == "route_fir_1025_c1024_l16384", c.id
        grid = c.env.get("SDRHIP_K7_PIPE_GRID")
        for n, names in zip(c.lens, c.expect):
            for k in names:
                m = re.match(r"fftconv_fused_kernel<14,0,1024,0,([24]),\d>", k)
                if m and grid:
                    assert -(-n // c.hop) * c.C > int(grid), c.id
                if m and m.group(1) == "4":
                    assert c.band == fc.ALIGNED and n % 2 == 0 and c.hop % 2 == 0, c.id
    big = [c for c in fc.cases() if c.C * max(c.lens) * 8 * (2 if c.f64 else 1) > 10e6]
    assert [c.id for c in big] == ["route_fir_1025_c1024_l16384"]
