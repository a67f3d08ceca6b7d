"""Writes the INPUT rows of the g24_ax25_* fixtures with the test-side encoder (tests/ax25_restatement.py): g24_ax25_bits.bin
(every row's bytes, one after the other) and g24_ax25_inputs.txt (per case: name, the row's offset and length, the call splits).
`cut` (cut.cc) then runs the unmodified reference on them.

    python make_inputs.py <outdir>

Rows: noise; APRS traffic between closing and opening flags with idle flags and a via path; frames that share single flags; a
frame that ends in five ones with no zero stuffed behind them (the closing flag's zero is dropped as stuffed); a frame aborted
by seven ones, with traffic behind it; a frame cut to a bit count that is no multiple of 8; and one long row with a frame of
exactly 512 buffered bytes (delivered) and one of 513 (lost). Every frame a row can deliver has a whole address field: the
unmodified reference reads behind a shorter one. Splits: one call, uneven calls with empty ones among them, and for two short
rows calls of 1 bit. The bytes carry upper bits: only bit 0 of a byte is the bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import ax25_restatement as R  # noqa: E402

UNEVEN = [13, 0, 1, 64, 15, 63, 65, 0, 16, 7, 129, 8, 257]


def uneven(n):
    out, left, k = [], n, 0
    while left:
        s = min(UNEVEN[k % len(UNEVEN)], left)
        out.append(s)
        left -= s
        k += 1
    return out


def five_ones_frame(rng):
    while True:
        fr = R.ui_frame(("APRS", 0), ("N0CALL", 7), text=bytes(rng.integers(32, 127, 9, dtype=np.uint8)))
        if R.ends_in_five_ones(fr):
            return fr


def rows(rng):
    z = lambda k: np.zeros(k, np.uint8)
    a = R.ui_frame(("APRS", 0), ("DL1ABC", 9), [("WIDE1", 1), ("WIDE2", 2)], b"!5230.00N/01320.00E>GPU deframer")
    b = R.ui_frame(("CQ", 0), ("K1XYZ", 0), text=b">status \xff\x7e\x7f\x00 bytes")
    c = R.ui_frame(("BEACON", 15), ("OE3AB", 3), [("RELAY", 0)], b"T#005,199,000,255,073,123,01101001")
    yield "noise", rng.integers(0, 2, 300).astype(np.uint8), True
    yield "traffic", np.concatenate([z(11), R.encode([a, b, c], idle_flags=2, lead_flags=3, tail=9)]), False
    yield "shared_flags", np.concatenate([z(3), R.encode([b[:16], c[:23]], shared_flags=True, tail=5)]), True
    yield "flag_zero_stuffed", R.encode([five_ones_frame(rng), a], shared_flags=True, stuff_tail=False, tail=3), False
    yield "abort", R.encode([a, b, c], abort_after={1: 77}, tail=2), False
    yield "bit_count", R.encode([a, c, b], drop_bits={1: 3}, shared_flags=True, tail=1), False
    full = R.ui_frame(("APRS", 0), ("DL1ABC", 9), text=bytes(rng.integers(0, 256, 494, dtype=np.uint8)))
    assert len(full) == 510
    yield "long", np.concatenate([R.encode([full, full + b"x", c], shared_flags=True), z(2)]), False


def main(outdir):
    rng = np.random.default_rng(0x24A825)
    bits, lines, offset = [], [], 0
    for kind, row, by_1 in rows(rng):
        row = (row | (rng.integers(0, 128, row.size).astype(np.uint8) << 1)).astype(np.uint8)
        n = int(row.size)
        for split_name, splits in (("whole", [n]), ("uneven", uneven(n))) + ((("by_1", [1] * n),) if by_1 else ()):
            assert sum(splits) == n
            lines.append("%s_%s %d %d %d %s" % (kind, split_name, offset, n, len(splits), " ".join(map(str, splits))))
        bits.append(row)
        offset += n
    np.concatenate(bits).tofile(os.path.join(outdir, "g24_ax25_bits.bin"))
    with open(os.path.join(outdir, "g24_ax25_inputs.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
