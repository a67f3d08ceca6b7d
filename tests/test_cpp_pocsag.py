"""C++ side of the POCSAG decoder bank on the GPU: sdr::gpu::POCSAGBank (include/sdr/gpu/pocsag.hh), built the way
tests/test_cpp_receiver.py builds its program. tests/cpp/test_pocsag_bank.cc runs every golden row as one channel of one bank, in
the recorded call splits, through process() (host rows) and processDev() (device rows); handleMessages(channel) has to deliver
the reference's deliveries, call by call."""
import os
import subprocess

import pytest

import pocsag_cases
from cpp_build import build


@pytest.mark.gpu
def test_pocsag_bank_delivers_the_golden_messages(tmp_path):
    exe = build("test_pocsag_bank.cc")
    n_cases, _ = pocsag_cases.write_cases(tmp_path / "cases.txt")
    g = pocsag_cases.GOLDEN
    r = subprocess.run([exe, str(tmp_path / "cases.txt"), os.path.join(g, "g19_pocsag_inputs.txt"), os.path.join(g, "g19_pocsag_bits.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK (0 failures)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "processDev: %d channels" % n_cases in r.stdout
