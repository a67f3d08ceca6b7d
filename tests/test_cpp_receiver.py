"""C++ side of the receiver bank: sdr::gpu::ReceiverBank<int16_t> (include/sdr/gpu/receiver.hh), built the way
tests/test_cpp_tuner_real.py builds its program — the host half (construction, services kept, config() rules, ConfigError on a
wrong input type and on a bad mode or service, the no-device path, destructors) under ASan/UBSan on the CPU as a stand-alone
program; on the GPU the five-channel plan of tests/receiver_plan.py in a graph: source -> ReceiverBank -> one bit recorder and one
audio recorder per channel, against files this module wrote from the CPU references, buffer by buffer."""
import os
import subprocess

import numpy as np
import pytest

import receiver_plan as rp
from cpp_build import SAN, build


def test_receiver_bank_host_half_under_sanitizers():
    exe = build("test_receiver_bank.cc", SAN, out="test_receiver_bank_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.mark.gpu
def test_receiver_bank_in_a_graph(tmp_path, orc):
    """Bits and audio of every channel, buffer by buffer, equal the CPU references' (the FSK LUTs from the product's designer,
    which the node uses too); a buffer without bits sends nothing on bits(c); an FM channel sends no empty audio buffer."""
    import libsdr_amd as sa
    x = rp.antenna()
    x.tofile(tmp_path / "input.cs16")
    want = rp.expected(orc, x, False, lut=sa.design_fsk_lut)
    for c, cfg in enumerate(rp.CHANNELS):
        calls = [(n, want[k][c]) for k, n in enumerate(rp.LENS) if n]       # (an empty input buffer is not processed at all)
        bits = [b for _, (_, b) in calls if b.size]
        audio = [a for _, (a, _) in calls if a.size or cfg[3] != "fm"]       # FMDemod sends nothing for an empty buffer
        assert len(bits) < len(calls) and sum(b.size for b in bits) >= 30
        np.concatenate(bits).astype(np.uint8).tofile(tmp_path / ("bits%d.u8" % c))
        np.array([b.size for b in bits], np.uint32).tofile(tmp_path / ("bits%d.lens" % c))
        np.concatenate(audio).astype(np.int16).tofile(tmp_path / ("audio%d.i16" % c))
        np.array([a.size for a in audio], np.uint32).tofile(tmp_path / ("audio%d.lens" % c))
    exe = build("test_receiver_bank.cc")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout + r.stderr
