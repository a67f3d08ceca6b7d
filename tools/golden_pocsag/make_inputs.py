"""Writes the INPUT rows of the g19_pocsag_* fixtures with the test-side encoder (tests/pocsag_restatement.py):
g19_pocsag_bits.bin (every row's bytes, one after the other), g19_pocsag_inputs.txt (per row: name, bit count, the call
splits), g19_pocsag_repair_in.bin (uint32 words for pocsag_repair). `cut` (cut.cc) then runs the unmodified reference on them.

    python make_inputs.py <outdir>
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import pocsag_restatement as P  # noqa: E402

TEXT = ((0x2345 << 3) | 2, 3, P.text_words("HELLO POCSAG 42"))
NUM = ((0x777 << 3) | 1, 0, P.numeric_words("0123456789-[]U ."))
RAGGED = [0, 1, 31, 32, 33, 63, 64, 65, 543, 544, 545]


def split(n, head):
    """head, as far as it fits, then the rest in one call"""
    out, left = [], n
    for h in head:
        if h > left:
            break
        out.append(h)
        left -= h
    return out + [left]


def cases():
    rng = np.random.default_rng(0x19C5A6)
    batches = P.frame([TEXT, NUM])
    assert len(batches) == 2
    clean = P.transmission(batches)
    n = clean.size
    data0, addr0 = P.word_offset(0, 5), P.word_offset(0, 4)   # TEXT sits in slot 2: its address word is codeword 4 of batch 0
    assert batches[0][4] == P.address_word(TEXT[0], TEXT[1])
    sync0, sync1 = P.word_offset(0, -1), P.word_offset(1, -1)
    out = [("clean", clean, [n]), ("clean_ragged", clean, split(n, RAGGED)),
           ("clean_by_7s", clean, split(n, [7] * 40 + [129] * 5))]
    for name, base, flips in (("data_1", data0, [3]), ("data_2", data0, [0, 31]), ("addr_1", addr0, [12]), ("addr_2", addr0, [1, 20]),
                              ("sync_1", sync0, [9]), ("sync_2", sync0, [0, 17]), ("data_3_dropped", data0, [2, 11, 25]),
                              ("sync_3_missed", sync0, [4, 5, 30]), ("cont_sync_2", sync1, [6, 28]), ("cont_sync_3_end", sync1, [6, 13, 28])):
        bits = P.flip(clean, [base + f for f in flips])
        out.append((name, bits, split(n, [600 + 37 * len(out), 64, 1, 500])))
    cut = clean[:P.word_offset(0, 9) + 13]
    out.append(("cut_mid_batch", cut, split(cut.size, [300, 300])))
    out.append(("noise", rng.integers(0, 2, 4096).astype(np.uint8), split(4096, [1000, 33, 2048])))
    # a sync word that completes ONE bit after an END: the continuation window is (x, sync[0..30]), then sync[31]
    one = P.frame([TEXT])
    head = P.transmission(one, tail=0)
    late = np.concatenate([head, [1], np.array(P.word_bits(P.SYNC_WORD), np.uint8)] +
                          [np.array(P.word_bits(w), np.uint8) for w in P.frame([NUM])[0]] + [np.array(P.preamble(64), np.uint8)])
    out.append(("sync_one_bit_after_end", late.astype(np.uint8), split(late.size, [head.size + 32, 1, 1])))
    orphan = [P.text_words("AB")[0]] + [P.IDLE_WORD] * 15
    out.append(("data_without_address", P.transmission([orphan]), split(P.transmission([orphan]).size, [545])))
    inside = [P.IDLE_WORD, P.IDLE_WORD, P.SYNC_WORD] + P.text_words("XY") + [P.IDLE_WORD] * 12
    assert len(inside) == 16
    out.append(("sync_inside_batch", P.transmission([inside]), split(P.transmission([inside]).size, [700, 5])))
    out.append(("upper_bits_set", (clean | 0xFE).astype(np.uint8), split(n, [544, 544])))
    return out


def repair_words():
    rng = np.random.default_rng(0x19BC4)
    words = [P.SYNC_WORD, P.IDLE_WORD, 0, 0xFFFFFFFF, P.address_word(TEXT[0], TEXT[1])]
    code = [P.codeword(int(d)) for d in rng.integers(0, 1 << 21, 200)]
    for w in code:
        for k in range(5):
            for _ in range(3):
                e = 0
                for b in rng.choice(32, k, replace=False):
                    e |= 1 << int(b)
                words.append(w ^ e)
    words += [int(v) for v in rng.integers(0, 1 << 32, 1000, dtype=np.uint64)]
    return np.array(words, np.uint32)


def main(outdir):
    rows = cases()
    with open(os.path.join(outdir, "g19_pocsag_inputs.txt"), "w") as f:
        for name, bits, splits in rows:
            assert sum(splits) == bits.size and bits.dtype == np.uint8, name
            f.write("%s %d %d %s\n" % (name, bits.size, len(splits), " ".join(map(str, splits))))
    np.concatenate([b for _, b, _ in rows]).tofile(os.path.join(outdir, "g19_pocsag_bits.bin"))
    repair_words().tofile(os.path.join(outdir, "g19_pocsag_repair_in.bin"))


if __name__ == "__main__":
    main(sys.argv[1])
