"""C++ side of the channel group (include/sdr/gpu/changroup.hh), built the way tests/test_cpp_channelizer.py builds its program.
tests/cpp/test_changroup.cc checks on the host that add() is refused after the first call, for a node that is a member already
and beyond eight members, and on the GPU runs a gpu::ChannelGroup of two gpu::Channelizer<int16_t> and one of two gpu::RealAudioChannelizer<int16_t> against the same
nodes' own processDev on twins, bit for bit."""
import subprocess

import pytest

from cpp_build import build


def test_add_is_refused_after_the_first_call():
    exe = build("test_changroup.cc")
    r = subprocess.run([exe, "rules"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rules: 3 adds refused" in r.stdout


@pytest.mark.gpu
def test_a_group_of_nodes_equals_the_nodes_alone():
    exe = build("test_changroup.cc")
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    for node in ("Channelizer<int16_t>", "RealAudioChannelizer<int16_t>"):
        assert "%s: 3 group calls of 2 members equal the twins'" % node in r.stdout
