"""The Baudot restatement (tests/baudot_restatement.py) against the fixtures the unmodified reference node left
(tests/golden/g23_baudot_*, manifest_baudot.json: tools/golden_baudot), and the parallel formulation — the kernel's algorithm:
candidate mask, greedy gate, setter scan, 64 positions at a time — against the per-bit loop, before any GPU sees it.
No tolerance anywhere: text, states and the calls that send are compared exactly."""
import json
import os

import numpy as np
import pytest

import baudot_restatement as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_baudot.json")))
BITS = np.fromfile(os.path.join(GOLDEN, MANIFEST["bits"]["file"]), np.uint8)
CASES = MANIFEST["cases"]


def run_case(case, cls):
    """-> (what every call sent: hex or None, the state after every call)"""
    dec, at, sends, states = cls(case["stop"]), case["offset"], [], []
    for n in case["splits"]:
        out = dec.process(BITS[at:at + n])
        at += n
        sends.append(out.hex() if out else None)   # the node sends only when a call decoded something (src/baudot.cc:110)
        states.append(list(dec.state()))
    return sends, states


def test_the_fixtures_cover_what_they_should():
    assert BITS.size == MANIFEST["bits"]["count"] and len(CASES) == 3 * 6 * 3
    names = {c["name"] for c in CASES}
    for kind in ("noise", "text", "space_in_figures", "null_and_shifts", "continuous", "mark_and_space"):
        for stop in ("stop1", "stop15", "stop2"):
            for split in ("whole", "by_1", "uneven"):
                assert "%s_%s_%s" % (kind, stop, split) in names
    assert any(0 in c["splits"] for c in CASES) and any(b & 0xFE for b in BITS.tolist())
    whole = {c["name"]: bytes.fromhex("".join(s or "" for s in c["sends"])) for c in CASES if c["name"].endswith("_whole")}
    assert whole["text_stop15_whole"] == b"RYRY 73 DE GPU\nQTH: 4/6 (OK)"
    assert whole["space_in_figures_stop1_whole"] == b"12 PE3  T"      # a space ends the figures run
    assert whole["null_and_shifts_stop2_whole"] == b"\0\0\0\0-A\0"     # code 0 emits a 0 byte in either table
    assert whole["continuous_stop1_whole"] == b"THE QUICK BROWN FOX 1234567890 TIMES"
    assert whole["mark_and_space_stop15_whole"].endswith(b"Q 599K")   # (the mark in front hides the first start bit)
    assert all(len(whole["noise_%s_whole" % s]) >= 3 for s in ("stop1", "stop15", "stop2"))


@pytest.mark.parametrize("cls", [B.Decoder, B.ParallelDecoder], ids=["loop", "parallel"])
def test_the_restatement_equals_the_reference_call_by_call(cls):
    for case in CASES:
        sends, states = run_case(case, cls)
        assert sends == case["sends"], case["name"]
        assert states == case["states"], case["name"]


def test_the_parallel_formulation_equals_the_loop_on_random_rows():
    r = np.random.default_rng(0xBA0D)
    emitted = 0
    for trial in range(400):
        stop = int(r.integers(0, 3))
        n = int(r.integers(0, 201))
        row = r.integers(0, 256, n).astype(np.uint8)
        if trial % 4 == 0 and n >= 40:   # some rows with text in the noise
            t = B.encode("A1 B2", stop)[:n - 20]
            row[10:10 + t.size] = t
        a, b = B.Decoder(stop), B.ParallelDecoder(stop)
        if trial % 3 == 0:   # a carried state of any kind, the gate open, shut or one short
            s = (int(r.integers(0, 1 << 16)), int(r.choice([0, 1, 12, 13, 14, 15, 16, 17, 1 << 40])), int(r.integers(0, 2)))
            a.bitstream, a.bitcount, a.mode = s
            b.bitstream, b.bitcount, b.mode = s
        splits, left = [0] if n == 0 else [], n
        while left:
            splits.append(min(int(r.choice([0, 1, 2, 13, 14, 15, 16, 63, 64, 65, 130, 200])), left))
            left -= splits[-1]
        at = 0
        for k in splits:
            x, y = a.process(row[at:at + k]), b.process(row[at:at + k])
            assert x == y and a.state() == b.state(), (trial, at, k)
            emitted += len(x)
            at += k
    assert emitted > 300


@pytest.mark.parametrize("stop", [B.STOP1, B.STOP15, B.STOP2])
@pytest.mark.parametrize("idle", [0, 1, 5])
def test_decode_of_encode_returns_the_text(stop, idle):
    text = b"THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG 0123456789 -?:(). ,/ \a\n RY 73"
    for cls in (B.Decoder, B.ParallelDecoder):
        assert B.decode(B.encode(text, stop, idle), stop, cls) == text
    # the shift codes appear only where the table changes
    assert B.codes("AB 12 3C") == [3, 25, B.SPA, B.STF, 23, 19, B.SPA, B.STF, 1, B.STL, 14]


def test_config_again_keeps_the_table():
    d = B.Decoder(B.STOP15)
    assert d.process(B.encode_codes([B.STF, 23], B.STOP15)) == b"1" and d.mode == B.FIGURES
    d.config()
    assert d.state() == (0, 0, B.FIGURES)
    assert d.process(B.encode_codes([23], B.STOP15)) == b"1"
    assert B.out_capacity(0) == 1 and B.out_capacity(13) == 1 and B.out_capacity(14) == 2 and B.out_capacity(446) == 32
