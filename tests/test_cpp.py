"""C++ side of the boundary: the API-compatible sdr:: core (CPU), and the sdr::gpu nodes wired into
graphs with that core (GPU) and with the UNMODIFIED reference runtime (GPU, drop-in proof)."""
import os
import subprocess

import pytest

from cpp_build import ROOT, SAN, build


def _build(src, out, extra=(), srcdir=("tests", "cpp")):
    """(these programs name their own libraries: the oracle's beside libsdrhip.so, _gpu_link_flags)"""
    return build(src, extra, link=False, out=out, srcdir=srcdir)


def _gpu_link_flags():
    from oracle import pyoracle
    pyoracle.build()
    return ["-I" + os.path.join(ROOT, "oracle"), "-L" + os.path.join(ROOT, "libsdr_amd"), "-lsdrhip",
            "-L" + os.path.join(ROOT, "oracle", "_build"), "-loracle",
            "-Wl,-rpath," + os.path.join(ROOT, "libsdr_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_build")]


def test_core_cpu():
    exe = _build("test_core.cc", "test_core")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr


def test_wav_nodes_cpu(tmp_path):
    """WavSink / WavSource: byte-identical files and identical read-back behaviour vs the reference's nodes."""
    exe = _build("test_wav.cc", "test_wav")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden"), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr


def _run_sanitized(exe, args, timeout=300):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_core_and_wav_under_sanitizers(tmp_path):
    """the host side under -fsanitize=address,undefined in the build container — the API-compatible core
    (Buffer refcounts, Queue thread, config propagation) and the WAV nodes."""
    _run_sanitized(_build("test_core.cc", "test_core_san", SAN), [os.path.join(ROOT, "tests", "golden")])
    _run_sanitized(_build("test_wav.cc", "test_wav_san", SAN), [os.path.join(ROOT, "tests", "golden"), str(tmp_path)])


def test_gpu_node_headers_host_half_under_sanitizers():
    """The host half of include/sdr/gpu/nodes.hh + design.hh (designers against golden vectors, config() rules, buffer
    views, destructors) under -fsanitize=address,undefined; no device needed: a complete Config without a GPU must end in
    a ConfigError ("no CPU fallback"), never in a crash. (Leak checking off for this one: the HIP runtime libsdrhip.so
    brings in is not ours to sanitize.)"""
    exe = _build("test_gpu_nodes.cc", "test_gpu_nodes_san", SAN + _gpu_link_flags())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "--host-only", os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_gpu_nodes_compile_and_link():
    """The node headers build against our core and link against the C-ABI library (no device needed)."""
    _build("test_gpu_nodes.cc", "test_gpu_nodes", _gpu_link_flags())


@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="reference tree only exists in the build container")
def test_gpu_nodes_compile_against_reference_core():
    """Drop-in: include/sdr/gpu/nodes.hh compiles unchanged against the reference's own headers and links
    with the reference's own objects (oracle/Makefile, target _ref/dropin_ref)."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "oracle", "_ref", "dropin_ref"))


@pytest.mark.gpu
def test_gpu_nodes_in_graphs():
    exe = _build("test_gpu_nodes.cc", "test_gpu_nodes", _gpu_link_flags())
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_reference_runtime_drives_gpu_nodes():
    exe = os.path.join(ROOT, "oracle", "_ref", "dropin_ref")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/dropin_ref was not built (needs /root/reference at build time)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr


def test_sdr_rec_wav_builds():
    _build("sdr_rec_wav.cc", "sdr_rec_wav", _gpu_link_flags(), srcdir=("examples",))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["NFM", "USB"])
def test_sdr_rec_wav_file_to_file(tmp_path, mode):
    """examples/sdr_rec.cc headless: cu8 WAV -> [AutoCast+IQBaseBand] -> FM+deemph / USB -> WAV on the MI355X; the
    output file equals, byte for byte, the one the reference chain wrote (tests/golden/g11_chain_*_wav.bin)."""
    import shutil
    exe = _build("sdr_rec_wav.cc", "sdr_rec_wav", _gpu_link_flags(), srcdir=("examples",))
    src, out = tmp_path / "in.wav", tmp_path / "out.wav"
    shutil.copy(os.path.join(ROOT, "tests", "golden", "g11_wav_cu8.bin"), src)
    r = subprocess.run([exe, str(src), mode, str(out), "4096"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = open(os.path.join(ROOT, "tests", "golden", "g11_chain_%s_wav.bin" % mode.lower()), "rb").read()
    assert out.read_bytes() == want


def test_bench_graph_builds():
    _build("bench_graph.cc", "bench_graph", _gpu_link_flags(), srcdir=("examples",))


@pytest.mark.gpu
def test_bench_graph_host_path_floor():
    """examples/bench_graph.cc: the drop-in layer's own throughput (sources -> gpu::ChannelBank -> sinks through the sdr:: core,
    pinned staging, PCIe both ways), so that the node layer cannot regress silently: a loose floor of 3.5 GS/s at 1024 channels
    (measured 4.4 GS/s with the round's H2D copy issued at its end, more with the copies pipelined behind the per-channel
    memcpys — one host core copying 268 MB per round into the staging area is the bound, not PCIe) and 10 us ... 1 ms per
    single-channel round (profiles/r18_host_path.txt holds a full run)."""
    import json
    exe = _build("bench_graph.cc", "bench_graph", _gpu_link_flags(), srcdir=("examples",))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["bench_graph"]
    assert d["c1024_msps"] >= 3500.0, d
    assert 0.01 < d["c1_ms"] < 1.0 and d["c64_msps"] > d["c1_msps"], d
