"""The restatements of the reference's AX.25 deframer (tests/ax25_restatement.py) against the g24_ax25_* fixtures cut from the
unmodified reference (tools/golden_ax25), against each other — the per-bit loop and the chunked formulation the kernel uses, for
any split into calls — and on the cases the node's rules single out. The Python Message is checked against the messages the
reference built from the same frames. No GPU."""
import json
import os

import numpy as np
import pytest

import ax25_restatement as R
from libsdr_amd import ax25

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "manifest_ax25.json")) as _f:
    MANIFEST = json.load(_f)
BITS = np.fromfile(os.path.join(GOLDEN, MANIFEST["bits"]["file"]), np.uint8)
CASES = MANIFEST["cases"]


def fnv(data):
    h = 2166136261
    for b in data:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def case_calls(case):
    """The rows of a case's calls."""
    at = case["offset"]
    for s in case["splits"]:
        yield BITS[at:at + s]
        at += s


def test_the_fixtures_are_whole():
    assert BITS.size == MANIFEST["bits"]["count"] and len(CASES) == 16
    assert MANIFEST["frames"] == sum(len(call) for case in CASES for call in case["frames"]) == 30
    assert (BITS >> 1).any()     # upper bits are set: only bit 0 is the bit
    for case in CASES:
        assert sum(case["splits"]) == case["n"] and len(case["states"]) == len(case["frames"]) == len(case["splits"])


@pytest.mark.parametrize("cls", [R.Decoder, R.ParallelDecoder], ids=["per_bit", "chunked"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_against_the_reference(case, cls):
    d = cls()
    for row, want_state, want_frames in zip(case_calls(case), case["states"], case["frames"]):
        got = d.process(row)
        assert [f.hex() for f, _ in got] == [w["raw"] for w in want_frames]
        bs, bb, st, ln, rx = d.get_state()
        assert [bs, bb, st, ln, fnv(rx)] == want_state
    assert d.get_state()[4].hex() == case["rxbuffer"]


def test_the_long_row_delivers_512_buffered_bytes_and_loses_513():
    case = next(c for c in CASES if c["name"] == "long_whole")
    lens = [len(w["raw"]) // 2 for call in case["frames"] for w in call]
    assert lens[0] == 510 and 511 not in lens and len(lens) == 2


def both(row, splits):
    """The row through both decoders in the same calls: the frames, with the events and the state compared after every call."""
    a, b, at, out = R.Decoder(), R.ParallelDecoder(), 0, []
    for s in splits:
        x, y = a.process(row[at:at + s]), b.process(row[at:at + s])
        assert x == y, (at, s, x, y)
        assert a.get_state() == b.get_state(), (at, s, a.get_state(), b.get_state())
        out += [(f, at + i) for f, i in x]
        at += s
    assert at >= len(row)
    return out


def random_splits(rng, n, most=80):
    out = []
    while sum(out) < n:
        out.append(int(rng.integers(0, most)))
    return out


def test_chunked_equals_per_bit_on_random_rows_and_splits():
    rng = np.random.default_rng(0xA825)
    for t in range(400):
        n = int(rng.integers(0, 301))
        kind = t % 4
        if kind == 0:
            row = rng.integers(0, 2, n).astype(np.uint8)
        elif kind == 1:        # dense in ones: flags, aborts and stuffed zeros everywhere
            row = (rng.random(n) < 0.8).astype(np.uint8)
        else:
            frames = [bytes(rng.integers(0, 256, int(rng.integers(1, 18)), dtype=np.uint8)) for _ in range(3)]
            row = R.encode(frames, shared_flags=bool(kind == 2), idle_flags=int(rng.integers(0, 2)), abort_after={1: 13} if t % 8 == 3 else None)[:n]
        both(row, random_splits(rng, len(row)))
        both(row, [len(row)])
        both(row, [1] * len(row))


def test_splits_inside_a_flag_a_stuffed_run_and_a_byte():
    fr = b"\xff\xff\x1f ax25"                     # ones: stuffed zeros in the first bytes
    row = R.encode([fr, fr[::-1]], shared_flags=True, lead_flags=2)
    want = [(fr, None), (fr[::-1], None)]
    for cut in range(len(row) + 1):
        got = both(row, [cut, len(row) - cut])
        assert [f for f, _ in got] == [f for f, _ in want]
    for sizes in ([0, 1, 63, 64, 65], [3] * 200, [64] * 10, [65, 63] * 5):
        splits = list(sizes)
        while sum(splits) < len(row):
            splits += sizes
        assert [f for f, _ in both(row, splits)] == [fr, fr[::-1]]


def test_decode_of_encode_gives_the_frames_back():
    rng = np.random.default_rng(7)
    frames = [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in (1, 2, 17, 64, 255)] + [b"\xff" * 9, b"\x7e\x7e\x7e", b"\x00"]
    for kw in (dict(), dict(shared_flags=True), dict(idle_flags=3), dict(lead_flags=5, tail=20), dict(shared_flags=True, idle_flags=1)):
        row = R.encode(frames, **kw)
        assert R.decode(row) == frames and R.decode(row, R.ParallelDecoder) == frames, kw
        data, ev = R.events(R.Decoder().process(row))
        assert data == b"".join(frames) and [e[1] & 0xFFFF for e in ev] == [len(f) for f in frames]


def test_a_single_flag_between_two_frames_closes_one_and_opens_the_next():
    a, b = b"first", b"second frame"
    row = R.encode([a, b], shared_flags=True)
    assert len(row) == 8 * 3 + len(R.frame_bits(a)) + len(R.frame_bits(b))
    assert R.decode(row) == [a, b] == R.decode(row, R.ParallelDecoder)


def test_the_flags_zero_counts_as_stuffed_behind_five_ones():
    rng = np.random.default_rng(3)
    while True:
        fr = bytes(rng.integers(0, 256, 6, dtype=np.uint8))
        if R.ends_in_five_ones(fr):
            break
    with_zero, without = R.encode([fr]), R.encode([fr], stuff_tail=False)
    assert len(with_zero) == len(without) + 1
    for row in (with_zero, without):
        assert [f for f, _ in both(row, [len(row)])] == [fr]
    # six of the flag's bits were pushed as data, not seven: one bit before the flag completes the byte under way holds six bits
    d = R.Decoder()
    d.process(without[:-1])
    bb = d.get_state()[1]
    assert 7 - ((bb & -bb).bit_length() - 1) == 6 and bb >> 2 == 0x3F
    d = R.Decoder()
    d.process(with_zero[:-1])
    bb = d.get_state()[1]
    assert 7 - ((bb & -bb).bit_length() - 1) == 7 and bb >> 1 == 0x7E


def test_an_abort_mid_frame_drops_the_frame_and_idles_to_the_next_flag():
    a, b, c = b"kept one", b"this one is aborted", b"kept two"
    row = R.encode([a, b, c], abort_after={1: 50})
    assert [f for f, _ in both(row, [len(row)])] == [a, c]
    d = R.Decoder()
    at = 8 + len(R.frame_bits(a)) + 16 + 50 + 7
    d.process(row[:at])
    assert d.get_state()[2] == 0 and d.get_state()[3] == 50 // 8     # the buffer keeps what it had


def test_512_buffered_bytes_are_delivered_and_513_are_lost_with_a_stale_bitbuffer():
    full = bytes((7 * i + 3) & 0xFF for i in range(510))
    row = R.encode([full, full + b"!", b"ok"], shared_flags=True)
    assert 8300 < len(row) < 9000
    got = both(row, [len(row)])
    assert [f for f, _ in got] == [full, b"ok"]
    both(row, [4000, 64, 65, 1, 0, 63, len(row)])
    # the state behind the 513th byte
    one = R.encode([full + b"!"])
    d, p = R.Decoder(), R.ParallelDecoder()
    for x in (d, p):
        x.process(one[:-8])                        # everything before the closing flag
        bs, bb, st, ln, rx = x.get_state()
        assert (st, ln) == (0, 512) and rx == (full + b"!" + R.fcs(full + b"!"))[:512]
        assert bb == 1 | (R.fcs(full + b"!")[1] << 1)          # the byte that found no room, under its marker
    assert d.get_state() == p.get_state()


def test_a_bit_count_that_is_no_multiple_of_8():
    """Whole bytes only enter the CRC, and the closing flag's first bits are pushed as data: a frame cut short by k bits is
    completed by the flag's 0, 1, 1 ... and passes exactly where those are the bits it lost."""
    a = b"whole bytes"
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(200):
        b = bytes(rng.integers(0, 128, 12, dtype=np.uint8))
        raw = [(v >> j) & 1 for v in b + R.fcs(b) for j in range(8)]
        if raw[-13:-8].count(1) == 5 or 1 not in raw[-8:-6]:
            continue                                    # (keep stuffing out of the last byte's neighbourhood)
        for drop in range(1, 8):
            row = R.encode([a, b, a], drop_bits={1: drop}, shared_flags=True)
            got = [f for f, _ in both(row, [len(row)])]
            lost_are_the_flags = raw[-drop:] == list(R.FLAG[:drop])
            if "11111" in "".join(map(str, raw[-drop - 5:-drop])):
                continue
            assert got == ([a, b, a] if lost_are_the_flags else [a, a]), (b, drop)
            seen.add((drop, lost_are_the_flags))
    assert {(d, False) for d in range(1, 8)} <= seen and (1, True) in seen and (2, True) in seen


def test_the_smallest_frame_has_three_buffered_bytes():
    row = R.encode([b"Z"])
    assert len(R.frame_bits(b"Z")) >= 24 and [f for f, _ in both(row, [len(row)])] == [b"Z"]
    # two buffered bytes are no frame, whatever they hold: an empty frame's FCS alone passes the CRC and is not delivered
    assert R.crc(R.fcs(b"")) == R.CRC_GOOD
    row = R.encode([b""])
    assert both(row, [len(row)]) == []


def test_the_densest_rows_meet_the_capacities():
    u = R.densest_frames_unit()
    assert u is not None and len(u) == 17
    for k in (1, 2, 3, 17):
        row = np.array(list(R.FLAG) + (u + list(R.FLAG)) * k, np.uint8)
        # the first call ends one bit before the first delivering flag completes: that frame is carried in and completes at 0
        head = 8 + 25 - 1
        d = R.Decoder()
        assert d.process(row[:head]) == []
        rest = row[head:]
        n = len(rest)
        got = d.process(rest)
        assert n == 25 * (k - 1) + 1 and len(got) == k == R.frames_capacity(n) and [i for _, i in got] == list(range(0, n, 25))
        assert all(len(f) == 1 for f, _ in got)
        both(row, [head, n])
    # bytes: 512 buffered bytes carried in and closed by position 0, then one frame over all that is left of the call
    for k in (1, 10, 54):
        row, head = R.densest_bytes_row(k)
        n = len(row) - head
        got = both(row, [head, n])
        assert [(len(f), i) for f, i in got] == [(510, head), (k, head + n - 1)]
        assert 510 + k == R.bytes_most(n) <= R.bytes_capacity(n)
    assert R.bytes_most(0) == 0 and all(R.bytes_most(n) == 510 for n in range(1, 26))
    # no row delivers more: noise and traffic in any split stay below it
    rng = np.random.default_rng(5)
    for _ in range(50):
        d = R.Decoder()
        d.set_state(0x7E, 0x80, 1, bytes(rng.integers(0, 256, 512, dtype=np.uint8)))
        n = int(rng.integers(1, 300))
        got = d.process(R.encode([bytes(rng.integers(0, 256, 3, dtype=np.uint8)) for _ in range(9)], shared_flags=True)[:n])
        assert sum(len(f) for f, _ in got) <= R.bytes_most(n) and len(got) <= R.frames_capacity(n)


# ---- the host-side Message ------------------------------------------------------------------------------------------------------

def test_message_parses_the_fixture_frames_as_the_reference_did():
    seen = 0
    for case in CASES:
        for call in case["frames"]:
            for w in call:
                m = ax25.Message.parse(bytes.fromhex(w["raw"]))
                assert not m.malformed
                assert [m.to.call.encode("latin-1").hex(), m.to.ssid] == w["to"] and [m.from_.call.encode("latin-1").hex(), m.from_.ssid] == w["from"]
                assert [[a.call.encode("latin-1").hex(), a.ssid] for a in m.via] == w["via"]
                assert m.payload.hex() == w["payload"]
                assert str(m).encode("latin-1").hex() == w["text"]
                seen += 1
    assert seen == MANIFEST["frames"]


def test_message_of_frames_that_are_shorter_than_their_addresses():
    good = R.ui_frame(("APRS", 0), ("DL1ABC", 9), [("WIDE1", 1)], b"hi")
    m = ax25.Message.parse(good)
    assert (str(m.to), str(m.from_), [str(a) for a in m.via], m.payload) == ("APRS-0", "DL1ABC-9", ["WIDE1-1"], b"\x03\xf0hi")
    assert str(m) == "DL1ABC-9 > APRS-0 via WIDE1-1 N=4\n\x03\xf0hi"
    assert str(ax25.Message.parse(good[:7] + R.address("K1XYZ", 2, last=True))) == "K1XYZ-2 > APRS-0 N=0\n"
    endless = R.address("A", 0) + R.address("B", 0) + R.address("C", 0) * 3     # no address says it is the last
    for raw in (b"", good[:6], good[:13], good[:14], good[:20], endless):
        m = ax25.Message.parse(raw)
        assert m.malformed and m.raw == raw and m.via == [] and m.to.call == "" and m.payload == b""
        assert str(m).startswith("malformed N=%d\n" % len(raw))
    assert ax25.Address.unpack(R.address("AB CD"))[0].call == "AB C"        # cut to the count of non-spaces, as the reference cuts
