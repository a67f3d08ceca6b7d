"""Writes the INPUT rows of the g23_baudot_* fixtures with the test-side encoder (tests/baudot_restatement.py):
g23_baudot_bits.bin (every row's bytes, one after the other) and g23_baudot_inputs.txt (per case: name, stop setting, the row's
offset and length, the call splits). `cut` (cut.cc) then runs the unmodified reference on them.

    python make_inputs.py <outdir>

Rows, for each of the three stop settings: noise (dense in candidates the gate has to refuse), text that uses both tables, a
space inside a figures run, the codes 0, 27 and 31 back to back, continuous traffic, and a long mark and a long space around
text. Every row in three splits: one call, calls of 1 bit, uneven calls with an empty one among them. The bytes carry
upper bits: only bit 0 of a byte is the half-bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import baudot_restatement as B  # noqa: E402

UNEVEN = [13, 0, 1, 64, 15, 63, 65, 0, 16, 14, 129]
NAMES = {B.STOP1: "stop1", B.STOP15: "stop15", B.STOP2: "stop2"}


def uneven(n):
    out, left, k = [], n, 0
    while left:
        s = min(UNEVEN[k % len(UNEVEN)], left)
        out.append(s)
        left -= s
        k += 1
    return out


def rows(stop, rng):
    z = lambda k: np.zeros(k, np.uint8)
    o = lambda k: np.ones(k, np.uint8)
    yield "noise", rng.integers(0, 2, 300).astype(np.uint8)
    yield "text", np.concatenate([z(5), B.encode("RYRY 73 DE GPU\nQTH: 4/6 (OK)", stop, idle=3), z(7)])
    yield "space_in_figures", np.concatenate([z(3), B.encode_codes([B.STF, 23, 19, B.SPA, 22, 1, B.STF, 1, B.SPA, B.SPA, 16], stop, idle=1), z(4)])
    yield "null_and_shifts", np.concatenate([z(9), B.encode_codes([0, B.STF, B.STL, 0, 0, B.STF, B.STF, 0, 3, B.STL, B.STL, 3, 0], stop), z(2)])
    yield "continuous", B.encode("THE QUICK BROWN FOX 1234567890 TIMES", stop)
    yield "mark_and_space", np.concatenate([o(70), B.encode("CQ 599", stop, idle=2), z(40), o(33), z(20), B.encode("K", stop), o(18)])


def main(outdir):
    rng = np.random.default_rng(0x23BA0D07)
    bits, lines, offset = [], [], 0
    for stop in (B.STOP1, B.STOP15, B.STOP2):
        for kind, row in rows(stop, rng):
            row = (row | (rng.integers(0, 128, row.size).astype(np.uint8) << 1)).astype(np.uint8)
            n = int(row.size)
            for split_name, splits in (("whole", [n]), ("by_1", [1] * n), ("uneven", uneven(n))):
                assert sum(splits) == n
                lines.append("%s_%s_%s %d %d %d %d %s" % (kind, NAMES[stop], split_name, stop, offset, n, len(splits), " ".join(map(str, splits))))
            bits.append(row)
            offset += n
    np.concatenate(bits).tofile(os.path.join(outdir, "g23_baudot_bits.bin"))
    with open(os.path.join(outdir, "g23_baudot_inputs.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
