"""Tuner bank (sdrhip_tuner_i16_*, libsdr_amd/csrc/tuner.hip), what can be checked without a GPU: the ABI is declared, bound
and exported; the kernels exist for gfx950, keep out of scratch, and the hot form is matrix code."""
import os
import re
import subprocess

import pytest

import abi_checks
from abi_checks import LLVM
from libsdr_amd import abi, nodes

TUNER_FUNCTIONS = ["sdrhip_tuner_i16_create", "sdrhip_tuner_i16_destroy", "sdrhip_tuner_i16_kernel_names", "sdrhip_tuner_i16_out_count",
                   "sdrhip_tuner_i16_plan_info", "sdrhip_tuner_i16_process", "sdrhip_tuner_i16_process_dev", "sdrhip_tuner_i16_reset", "sdrhip_tuner_i16_set_input_format",
                   "sdrhip_tuner_i16_set_shift", "sdrhip_tuner_i16_set_taps"]


def test_tuner_abi_is_declared_bound_and_exported():
    L = abi.lib()
    declared = abi.header_functions()
    assert sorted(f for f in declared if f.startswith("sdrhip_tuner_")) == TUNER_FUNCTIONS
    for f in TUNER_FUNCTIONS:
        assert hasattr(L, f), f
        assert f in L._declared, f
    assert hasattr(nodes, "TunerBankI16")
    for m in ("out_count", "process", "process_dev", "set_taps", "set_shift", "set_input_format", "reset", "kernel_names"):
        assert hasattr(nodes.TunerBankI16, m), m


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    objs = abi_checks.code_objects(tmp_path_factory.mktemp("tuner_co"))
    assert objs, "no gfx950 code object in the library"
    return objs


def _tuner_kernels(objs):
    """{kernel name: (code object, scratch bytes)} of every tuner_ kernel."""
    return {name: (o, scratch) for o, name, scratch in abi_checks.kernels(objs) if "tuner_" in name}


def test_tuner_kernels_keep_out_of_scratch(code_objects):
    k = _tuner_kernels(code_objects)
    # both forms x four epilogues x two input kinds
    assert sum("tuner_i16_valu_kernel" in n for n in k) == 8, sorted(k)
    assert sum("tuner_i16_mfma_kernel" in n for n in k) == 8, sorted(k)
    assert not any("iqbb_hot" in n for n in k)   # (the one-tune hot kernel's instance matrix is pinned by its own tests)
    bad = {n: s for n, (_, s) in k.items() if s}
    assert not bad, bad


def test_tuner_hot_form_is_matrix_code(code_objects):
    k = _tuner_kernels(code_objects)
    objs = {o for n, (o, _) in k.items() if "tuner_i16_mfma_kernel" in n}
    assert objs
    hot_with_mfma = set()
    for o in objs:
        dis = subprocess.run([LLVM + "llvm-objdump", "-d", str(o)], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
            elif cur and "tuner_i16_mfma_kernel" in cur and re.search(r"v_mfma_i32_\w+_i8", line):
                hot_with_mfma.add(cur)
    assert len(hot_with_mfma) == 8, sorted(hot_with_mfma)   # every instance of the hot form


SNIPPET = r"""
#include "sdr.hh"
#include "sdr/gpu/nodes.hh"
using namespace sdr;
void graph(Source &src, Sink<int16_t> &audio0, Sink<int16_t> &audio1) {
  gpu::TunerBank<int16_t> bank(127, 8, SDRHIP_EPI_FM);
  const size_t a = bank.addChannel(100e3, 100e3, 50e3), b = bank.addChannel(-300e3, -300e3, 12.5e3);
  src.connect(&bank, true);
  bank.source(a)->connect(&audio0, true);
  bank.source(b)->connect(&audio1, true);
  bank.setCenterFrequency(b, -250e3);
  bank.setFilterFrequency(b, -250e3);
  bank.setFilterWidth(a, 30e3);
}
"""


def _syntax_only(tmp_path, includes):
    src = tmp_path / "snippet.cc"
    src.write_text(SNIPPET)
    cmd = ["g++", "-std=c++17", "-Wall", "-fsyntax-only"]
    for i in includes:
        cmd += ["-I", i]
    r = subprocess.run(cmd + [str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_tuner_bank_node_compiles_against_own_core(tmp_path):
    _syntax_only(tmp_path, [os.path.join(abi.ROOT, "include", "sdr"), os.path.join(abi.ROOT, "include")])


REF = "/root/reference/src"


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
def test_tuner_bank_node_compiles_against_reference_headers(tmp_path):
    _syntax_only(tmp_path, [os.path.join(abi.ROOT, "oracle", "_ref"), REF, os.path.join(abi.ROOT, "include")])
