"""gpu::FilterSink / gpu::FilterSource in C++ graphs (tests/cpp/test_gpu_filter_split.cc), and the drop-in compile of the two
classes against the reference's own headers."""
import os
import subprocess

import pytest

from tests.test_cpp import ROOT, _build, _gpu_link_flags

REF = "/root/reference/src"


def test_filter_split_compiles_and_links():
    _build("test_gpu_filter_split.cc", "test_gpu_filter_split", _gpu_link_flags())


@pytest.mark.gpu
def test_filter_split_in_graphs():
    exe = _build("test_gpu_filter_split.cc", "test_gpu_filter_split", _gpu_link_flags())
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr


SNIPPET = r"""
#include "sdr.hh"
#include "filternode.hh"
#include "sdr/gpu/nodes.hh"
using namespace sdr;
// the reference's own FilterSink feeding a gpu::FilterSource (taken by reference: without FFTW the reference's FFTPlan
// has no constructor that FilterSink could call, so only the wiring is compiled here)
void wire(sdr::FilterSink<float> &ref_sink, gpu::FilterSource<float> &b) { ref_sink.connect(&b, true); }
void graph() {
  gpu::FilterSink<float> sink(1024);
  gpu::FilterSource<float> a(1024, 50e3, 150e3);
  sink.connect(&a, true);
  gpu::FilterNode<float> node(1024);
  gpu::FilterSource<float> *s = node.addFilter(-350e3, -250e3);
  s->setFreq(-300e3, -200e3);
  gpu::FilterSink<double> sd(1000);
  gpu::FilterSource<double> bd(1000, 0, 1e5);
  sd.connect(&bd, true);
}
"""


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
def test_filter_split_compiles_against_reference_headers(tmp_path):
    src = tmp_path / "snippet.cc"
    src.write_text(SNIPPET)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "oracle", "_ref"), "-I", REF,
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
