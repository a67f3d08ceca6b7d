"""The POCSAG decoder restated in numpy and Python — the test-side reference of the decoder bank (include/sdrhip_pocsag.h):

  * `Decoder`: the reference node's per-bit state machine (src/pocsag.cc:41-95), producing the bank's event stream and the
    node's final state. Its word test is a parameter: `repair_search` (slow, the reference's semantics) or `repair_table`.
  * `syndrome`, and `repair_search` / `repair_search_many`: pocsag_repair as the reference SEARCHES (src/bch31_21.cc:123-212):
    the single-bit candidates, then the 528 candidates (b1 <= b2) in batches of 32 slices, the first batch with a hit, its
    highest slice. Not via the table.
  * `repair_table` and `is_sync_popcount`: the two rules the device code rests on, tested against the search.
  * an encoder that builds test rows (preamble, sync, eight two-word slots per batch, address / text / numeric / idle words,
    BCH parity and the even-parity bit), written from the POCSAG standard, and error injection.
"""
import numpy as np

SYNC_WORD = 0x7CD215D8
IDLE_WORD = 0x7A89C197
GEN = 0o3551            # g(x) = x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
SYNC, WORD, END = 0, 1, 2
WAIT, RECEIVE, CHECK_CONTINUE = 0, 1, 2
BCD = "084 2.6]195-3U7["


def out_capacity(n):
    return n // 32 + n // 256 + 4


# ---- syndrome -----------------------------------------------------------------------------------------------------------
def syndrome(w):
    """11 bits: the remainder of bits 31..1 by g(x), long division; bit 10 set when the whole word has odd parity."""
    sh = (w & 0xFFFFFFFF) >> 1
    for i in range(21):
        if sh & (1 << (30 - i)):
            sh ^= GEN << (20 - i)
    return sh | ((bin(w & 0xFFFFFFFF).count("1") & 1) << 10)


# the long division and the parity are linear over GF(2): a word's syndrome is the XOR of its four bytes' syndromes. These
# tables only make `syndrome` fast on arrays (syndrome_np is tested against the scalar long division).
_BYTE_SYN = np.array([[syndrome(b << (8 * k)) for b in range(256)] for k in range(4)], np.uint32)


def syndrome_np(w):
    w = np.asarray(w, np.uint32)
    return (_BYTE_SYN[0][w & 255] ^ _BYTE_SYN[1][(w >> 8) & 255] ^ _BYTE_SYN[2][(w >> 16) & 255] ^ _BYTE_SYN[3][w >> 24])


# ---- pocsag_repair as the reference searches ----------------------------------------------------------------------------
# the 528 two-bit candidates in the reference's order; b2 == b1 flips the same bit twice: the word itself
_PAIRS = np.array([((1 << b1) ^ (1 << b2)) if b1 != b2 else 0 for b1 in range(32) for b2 in range(b1, 32)], np.uint32)
_SINGLES = (np.uint32(1) << np.arange(32, dtype=np.uint32)).astype(np.uint32)


def repair_search_many(words, chunk=4096):
    """-> (rc [N] int, out [N] uint32): pocsag_repair's return code and the word it leaves, for every word."""
    words = np.asarray(words, np.uint32).ravel()
    rc, out = np.ones(words.size, np.int64), words.copy()
    pad = np.zeros(17 * 32 - _PAIRS.size, np.uint32)   # the leftover half batch: its unused slices hold the word itself
    cand2 = np.concatenate([_PAIRS, pad]).reshape(17, 32)
    for a in range(0, words.size, chunk):
        w = words[a:a + chunk]
        r, o = np.ones(w.size, np.int64), w.copy()
        clean = syndrome_np(w) == 0
        r[clean] = 0
        # single-bit errors: slice i has bit i flipped; the HIGHEST slice with a zero syndrome is taken
        z1 = syndrome_np(w[:, None] ^ _SINGLES[None, :]) == 0
        hit1 = z1.any(axis=1) & ~clean
        n1 = 31 - np.argmax(z1[:, ::-1], axis=1)
        o[hit1] = w[hit1] ^ _SINGLES[n1[hit1]]
        r[hit1] = 0
        # two-bit errors: the FIRST batch of 32 slices with a hit, and in it the highest slice
        z2 = syndrome_np(w[:, None, None] ^ cand2[None, :, :]) == 0
        bh = z2.any(axis=2)
        hit2 = bh.any(axis=1) & ~clean & ~hit1
        b = np.argmax(bh, axis=1)
        zb = z2[np.arange(w.size), b]
        n2 = 31 - np.argmax(zb[:, ::-1], axis=1)
        o[hit2] = w[hit2] ^ cand2[b[hit2], n2[hit2]]
        r[hit2] = 0
        rc[a:a + chunk], out[a:a + chunk] = r, o
    return rc, out


def repair_search(w):
    rc, out = repair_search_many([w])
    return int(rc[0]), int(out[0])


# ---- the two rules of the device code -----------------------------------------------------------------------------------
def build_table():
    """syndrome -> the error pattern of weight <= 2 that has it (-1: none). 529 live entries of 2048."""
    t = np.full(2048, -1, np.int64)
    for i in range(32):
        for j in range(i, 32):
            e = (1 << i) | (1 << j)
            s = syndrome(e)
            assert t[s] in (-1, e)
            t[s] = e
    t[0] = 0
    return t


TABLE = build_table()


def repair_table(w):
    e = int(TABLE[syndrome(w)])
    return (1, w) if e < 0 else (0, w ^ e)


def repair_table_many(words):
    words = np.asarray(words, np.uint32).ravel()
    e = TABLE[syndrome_np(words)]
    return (e < 0).astype(np.int64), np.where(e < 0, words, words ^ (e & 0xFFFFFFFF).astype(np.uint32)).astype(np.uint32)


def is_sync_popcount(w):
    return bin((w ^ SYNC_WORD) & 0xFFFFFFFF).count("1") <= 2


# ---- the node ---------------------------------------------------------------------------------------------------------------
class Decoder:
    """One reference POCSAG node. process(bits) consumes one call's row (bit 0 of every byte) and returns its events as
    (word, info) pairs; state() is (_state, _bitcount, _slot, _bits). A freshly configured node is WAIT with every register 0
    (the reference leaves _bitcount and _slot unset until the first sync word; the golden cut starts them at 0)."""

    def __init__(self, repair=repair_table):
        self.repair = repair
        self.st, self.bitcount, self.slot, self.shift = WAIT, 0, 0, 0

    def state(self):
        return self.st, self.bitcount, self.slot, self.shift

    def _is_sync(self, w):
        rc, r = self.repair(w)
        return rc == 0 and r == SYNC_WORD

    def process(self, bits):
        ev = []
        for i, b in enumerate(np.asarray(bits, np.uint8).tolist()):
            self.shift = ((self.shift << 1) | (b & 1)) & 0xFFFFFFFFFFFFFFFF
            if self.st == WAIT:
                if self._is_sync(self.shift & 0xFFFFFFFF):
                    ev.append((SYNC_WORD, SYNC | (i << 8)))
                    self.st, self.bitcount, self.slot = RECEIVE, 0, 0
            elif self.st == RECEIVE:
                self.bitcount += 1
                if self.bitcount == 64:
                    self.bitcount = 0
                    for w in (self.shift >> 32, self.shift & 0xFFFFFFFF):
                        rc, r = self.repair(w)
                        if rc == 0:
                            ev.append((r, WORD | (self.slot << 2) | (32 if r != w else 0) | (i << 8)))
                    self.slot += 1
                    if self.slot == 8:
                        self.st = CHECK_CONTINUE
            else:
                self.bitcount += 1
                if self.bitcount == 32:
                    if self._is_sync(self.shift & 0xFFFFFFFF):
                        self.st, self.slot, self.bitcount = RECEIVE, 0, 0
                    else:
                        ev.append((0, END | (i << 8)))
                        self.st = WAIT
        return ev


# ---- encoder -----------------------------------------------------------------------------------------------------------------
def codeword(data21):
    """21 information bits -> the 32-bit codeword: 10 BCH check bits (the remainder of data * x^10 by g), then even parity."""
    sh = (data21 & 0x1FFFFF) << 10
    rem = sh
    for i in range(21):
        if rem & (1 << (30 - i)):
            rem ^= GEN << (20 - i)
    cw = sh | rem
    return (cw << 1) | (bin(cw).count("1") & 1)


def address_word(address, function):
    """The address word of a 21-bit address (its low 3 bits choose the slot and are not sent) and a 2-bit function."""
    return codeword((((address >> 3) & 0x3FFFF) << 2) | (function & 3))


def data_words(bits):
    """A payload bit list -> message codewords of 20 bits each (flag bit 1), the last one padded with zeros."""
    bits = list(bits) + [0] * (-len(bits) % 20)
    return [codeword((1 << 20) | int("".join(map(str, bits[k:k + 20])), 2)) for k in range(0, len(bits), 20)]


def text_words(text):
    """7-bit characters, each sent LSB first."""
    return data_words([(ord(ch) >> j) & 1 for ch in text for j in range(7)])


def numeric_words(digits):
    """4-bit BCD symbols; padded to whole codewords with spaces."""
    digits = digits + " " * (-len(digits) % 5)
    return data_words([(BCD.index(ch) >> j) & 1 for ch in digits for j in (3, 2, 1, 0)])


def frame(messages):
    """messages: (address, function, [data codewords]) -> batches of 16 codewords. A message starts in the slot its address
    names, at or behind the previous message's end; everything else is the idle word."""
    words, at = [], 0
    for address, function, data in messages:
        while (at // 2) % 8 != address % 8 or at % 2:
            words.append(IDLE_WORD)
            at += 1
        words += [address_word(address, function)] + list(data)
        at += 1 + len(data)
    words += [IDLE_WORD] * (-len(words) % 16)
    return [words[k:k + 16] for k in range(0, len(words), 16)]


def word_bits(w):
    return [(w >> (31 - k)) & 1 for k in range(32)]


def preamble(n=576):
    return [1 - (k & 1) for k in range(n)]


def transmission(batches, preamble_bits=576, tail=64):
    """-> uint8 bits: preamble, then sync + 16 codewords per batch, then `tail` preamble-like bits (no sync: the END)."""
    b = preamble(preamble_bits)
    for batch in batches:
        for w in [SYNC_WORD] + list(batch):
            b += word_bits(w)
    return np.array(b + preamble(tail), np.uint8)


def word_offset(batch, index, preamble_bits=576):
    """Bit offset of codeword `index` (0 ... 15; -1: the sync word) of batch `batch` in a transmission()."""
    return preamble_bits + batch * 17 * 32 + (index + 1) * 32


def flip(bits, positions):
    bits = np.array(bits, np.uint8)
    for p in positions:
        bits[p] ^= 1
    return bits


def corruptions(word, max_flips=3):
    """Every word that differs from `word` in 1 ... max_flips positions drawn WITH repetition (a position drawn twice cancels)."""
    out = {word}
    level = {word}
    for _ in range(max_flips):
        level = {w ^ (1 << i) for w in level for i in range(32)}
        out |= level
    return sorted(out)
