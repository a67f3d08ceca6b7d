"""Restatement of the reference's AX.25 deframer (src/ax25.hh, src/ax25.cc:79-161) — TEST CODE, written from the description in
include/sdrhip_ax25.h: the per-bit loop (Decoder), the same node in the chunked formulation the kernel uses (ParallelDecoder:
bit word, local classification, segment loop, compaction, running CRC, 64 positions at a time), an encoder for test rows and
the capacity formulas.

The node: per byte b, _bitstream = (_bitstream << 1) | (b & 1) in 32 bits (:105). Then the first rule that matches:
  flag     (_bitstream & 0xff) == 0x7e (:108): with _state == 1 and more than 2 bytes buffered the CRC-CCITT (init 0xffff,
           reflected, good residue 0xf0b8) of the buffered bytes is taken and, if good, the bytes without the last two are
           delivered (:109-120); then _state = 1, the buffer is empty, _bitbuffer = 0x80 (:122-124);
  abort    (_bitstream & 0x7f) == 0x7f: _state = 0 (:129);
  idle     _state == 0 (:132);
  stuffed  (_bitstream & 0x3f) == 0x3e: the bit is dropped (:135);
  data     _bitbuffer |= bit << 8 (:139); with bit 0 of _bitbuffer set a byte is complete: with 512 bytes buffered _state = 0
           and _bitbuffer stays (:144-149), otherwise the byte (_bitbuffer >> 1) & 0xff is stored and _bitbuffer = 0x80
           (:152-154); without it _bitbuffer >>= 1 (:159).
config() sets _bitstream = _bitbuffer = _state = 0 and empties the buffer (:90-93)."""
import numpy as np

RX_MAX = 512
CRC_GOOD = 0xF0B8
FLAG = (0, 1, 1, 1, 1, 1, 1, 0)


def frames_capacity(n_bits):
    """The header's: the most frames n_bits positions can deliver."""
    return n_bits // 25 + 1


def bytes_capacity(n_bits):
    """The header's: room for the frame bytes n_bits positions can deliver."""
    return n_bits // 8 + 512


def bytes_most(n_bits):
    """The most frame bytes n_bits positions do deliver (the header's argument): a frame of 512 buffered bytes carried in and
    closed by position 0, then one frame over the n_bits - 2 positions between that flag's last bit and the next one's."""
    return 0 if n_bits == 0 else 510 + max(0, (n_bits - 2) // 8 - 2)


def crc_update(crc, byte):
    """One byte into the reflected CRC-CCITT (polynomial 0x8408), bit by bit."""
    crc ^= byte
    for _ in range(8):
        crc = (crc >> 1) ^ (0x8408 if crc & 1 else 0)
    return crc


def crc_update_fast(crc, byte):
    """The same step in shifts and exclusive-ors, as the kernel takes it."""
    d = (byte ^ crc) & 0xFF
    d = (d ^ (d << 4)) & 0xFF
    return ((d << 8) | (crc >> 8)) ^ (d >> 4) ^ (d << 3)


_TABLE = [crc_update(0, b) for b in range(256)]


def crc(data, start=0xFFFF):
    for b in data:
        start = (start >> 8) ^ _TABLE[(start ^ b) & 0xFF]
    return start


def fcs(data):
    """The two bytes a sender appends: the complemented CRC, low byte first."""
    v = crc(data) ^ 0xFFFF
    return bytes([v & 0xFF, v >> 8])


class Decoder:
    """One node, bit by bit. process(bits) -> [(frame bytes, bit index)] that call delivers; state() -> (bitstream, bitbuffer,
    state, len, the len buffered bytes)."""

    def __init__(self):
        self.config()

    def config(self):
        self.bitstream, self.bitbuffer, self.state, self.rx = 0, 0, 0, bytearray()

    def get_state(self):
        return self.bitstream, self.bitbuffer, self.state, len(self.rx), bytes(self.rx)

    def set_state(self, bitstream, bitbuffer, state, rx):
        self.bitstream, self.bitbuffer, self.state, self.rx = bitstream, bitbuffer, state, bytearray(rx)

    def process(self, bits):
        out = []
        for i, b in enumerate(np.asarray(bits, np.uint8).ravel().tolist()):
            self.bitstream = ((self.bitstream << 1) | (b & 1)) & 0xFFFFFFFF                     # :105
            if self.bitstream & 0xFF == 0x7E:                                                      # :108
                if self.state == 1 and len(self.rx) > 2 and crc(self.rx) == CRC_GOOD:              # :109-111
                    out.append((bytes(self.rx[:-2]), i))                                           # :117
                self.state, self.rx, self.bitbuffer = 1, bytearray(), 0x80                         # :122-124
                continue
            if self.bitstream & 0x7F == 0x7F:                                                      # :129
                self.state = 0
                continue
            if not self.state:                                                                     # :132
                continue
            if self.bitstream & 0x3F == 0x3E:                                                      # :135
                continue
            self.bitbuffer |= (self.bitstream & 1) << 8                                            # :139
            if self.bitbuffer & 1:                                                                 # :142
                if len(self.rx) >= RX_MAX:                                                         # :144
                    self.state = 0
                    continue
                self.rx.append((self.bitbuffer >> 1) & 0xFF)                                       # :152
                self.bitbuffer = 0x80
                continue
            self.bitbuffer >>= 1                                                                   # :159
        return out


M64 = (1 << 64) - 1


def _select(mask, r):
    """The position of the r-th set bit of a 64-bit mask (r below its population count) by bisection, as a lane finds it."""
    pos, width = 0, 32
    while width:
        low = bin((mask >> pos) & ((1 << width) - 1)).count("1")
        if r >= low:
            r -= low
            pos += width
        width >>= 1
    return pos


class ParallelDecoder(Decoder):
    """The same node, 64 positions at a time, as libsdr_amd/csrc/ax25.hip walks a row: no state is touched per bit. Beside the
    node's members it carries the running CRC of the buffered bytes, which is derived state."""

    def process(self, bits):
        bits = (np.asarray(bits, np.uint8).ravel() & 1).tolist()
        n, out = len(bits), []
        if n == 0:
            return out
        hist = self.bitstream                      # the 32 bits before the chunk, the newest in bit 0
        state, bitbuffer, rx = self.state, self.bitbuffer, self.rx
        run = crc(rx)
        for base in range(0, n, 64):
            chunk = bits[base:base + 64]
            m = len(chunk)
            cur = sum(b << i for i, b in enumerate(chunk))
            valid = (1 << m) - 1
            # classification, local to a lane: its 8-bit window
            F = A = S = 0
            for l in range(m):
                w = 0
                for j in range(8):                 # bit j of the window is position l - j
                    p = l - j
                    w |= (((cur >> p) & 1) if p >= 0 else ((hist >> (-p - 1)) & 1)) << j
                if w == 0x7E:
                    F |= 1 << l
                elif w & 0x7F == 0x7F:
                    A |= 1 << l
                elif w & 0x3F == 0x3E:
                    S |= 1 << l
            D = valid & ~(F | A | S)
            # the segment loop: a segment ends at a flag or at the chunk's end
            start, trips = 0, 0
            while start < m:
                trips += 1
                rest = (M64 << start) & M64
                f = F & rest
                end = (f & -f).bit_length() - 1 if f else m          # the closing flag's position
                seg = rest & ((1 << end) - 1)
                if state == 1:
                    a = A & seg
                    if a:
                        seg &= (a & -a) - 1                           # nothing behind the first abort is live
                    dm = D & seg
                    k = 7 - ((bitbuffer & -bitbuffer).bit_length() - 1)   # bits of the byte under way
                    part = bitbuffer >> (8 - k)
                    nd = bin(dm).count("1")
                    room = (RX_MAX + 1) * 8 - (len(rx) * 8 + k)       # data bits up to and with the one that overflows
                    over = nd >= room
                    if over:
                        nd = room
                    word = sum(((cur >> _select(dm, r)) & 1) << r for r in range(nd))    # the compacted data bits
                    total = part | (word << k)
                    t = k + nd
                    for j in range(t // 8):
                        byte = (total >> (8 * j)) & 0xFF
                        if len(rx) < RX_MAX:
                            rx.append(byte)
                            run = crc_update_fast(run, byte)
                        else:
                            bitbuffer = 1 | (byte << 1)               # the overflowing byte stays in _bitbuffer
                    if over:
                        state = 0
                    else:
                        k2 = t % 8
                        bitbuffer = (0x80 >> k2) | (((total >> (t - k2)) & ((1 << k2) - 1)) << (8 - k2))
                        if a:
                            state = 0
                if end < m:                                           # the flag
                    if state == 1 and len(rx) > 2 and run == CRC_GOOD:
                        out.append((bytes(rx[:-2]), base + end))
                    state, bitbuffer, run = 1, 0x80, 0xFFFF
                    del rx[:]
                start = end + 1
            assert trips <= 11
            hist = ((hist << m) | int(format(cur, "0%db" % m)[::-1], 2)) & 0xFFFFFFFF
        self.bitstream, self.bitbuffer, self.state = hist, bitbuffer, state
        return out


def stuff(bits):
    """A zero behind every five ones."""
    out, ones = [], 0
    for b in bits:
        out.append(b)
        ones = ones + 1 if b else 0
        if ones == 5:
            out.append(0)
            ones = 0
    return out


def frame_bits(frame, with_fcs=True, drop_bits=0, stuff_tail=True):
    """One frame's stuffed bits without flags: the bytes and their FCS, the low bit of a byte first. drop_bits: that many of
    the last bits are left out before stuffing (a bit count that is no multiple of 8). stuff_tail False: a frame that ends in
    five ones gets no zero behind them, so the closing flag's own zero is the one the node drops as stuffed."""
    data = bytes(frame) + (fcs(frame) if with_fcs else b"")
    raw = [(b >> j) & 1 for b in data for j in range(8)]
    if drop_bits:
        raw = raw[:-drop_bits]
    out = stuff(raw)
    if not stuff_tail and out[-6:] == [1, 1, 1, 1, 1, 0] and raw[-5:] == [1, 1, 1, 1, 1]:
        out.pop()
    return out


def encode(frames, shared_flags=False, idle_flags=0, lead_flags=1, abort_after=None, drop_bits=None, tail=0, stuff_tail=True):
    """frames -> one row of bits. Every frame stands between flags; shared_flags: one flag between two frames (it closes one and
    opens the next), otherwise a closing and an opening one; idle_flags: that many more flags between two frames; lead_flags:
    flags in front of the first frame; abort_after: {frame index: bits} — that frame is cut behind so many of its stuffed bits
    and seven ones follow; drop_bits: {frame index: bits} left out of the frame's end; tail: zeros behind the last flag;
    stuff_tail: see frame_bits."""
    abort_after, drop_bits = abort_after or {}, drop_bits or {}
    row = list(FLAG) * lead_flags
    for i, fr in enumerate(frames):
        body = frame_bits(fr, drop_bits=drop_bits.get(i, 0), stuff_tail=stuff_tail)
        if i in abort_after:
            row += body[:abort_after[i]] + [1] * 7 + [0]
            row += list(FLAG)
        else:
            row += body + list(FLAG)
        last = i == len(frames) - 1
        row += list(FLAG) * idle_flags
        if not shared_flags and not last:
            row += list(FLAG)
    row += [0] * tail
    return np.array(row, np.uint8)


def decode(bits, cls=Decoder):
    return [f for f, _ in cls().process(bits)]


def events(found):
    """[(frame, bit index)] -> (frame bytes back to back, [[offset, length | index << 16]]) as a row of the bank holds them."""
    data, ev = b"", []
    for fr, at in found:
        ev.append([len(data), len(fr) | (at << 16)])
        data += fr
    return data, ev


# ---- the densest rows ---------------------------------------------------------------------------------------------------------

def densest_frames_unit():
    """17 bits u such that the row flag, (u, flag) repeated delivers a 1-byte frame at every flag behind the first: every 25
    positions, the least the node allows (three buffered bytes: the 17 bits and the closing flag's first seven). None if there
    is no such u."""
    for v in range(1 << 17):
        # without stuffing inside u the three bytes are u's first sixteen bits and its last with the flag's 0, 1, 1, 1, 1, 1, 1 above it
        if crc([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) | 0xFC]) != CRC_GOOD:
            continue
        u = [(v >> j) & 1 for j in range(17)]
        d = Decoder()
        d.process(list(FLAG))
        if len(d.process(u + list(FLAG))) == 1 and len(d.process(u + list(FLAG))) == 1:
            return u
    return None


def ends_in_five_ones(frame):
    """Whether the frame's last five bits on the air (the top of its second FCS byte) are ones behind a zero."""
    return fcs(frame)[1] >> 2 == 0x3E


def address(call, ssid=0, last=False):
    """The seven bytes of an address field: six characters shifted left, the SSID, and bit 0 set on the last address."""
    return bytes(ord(ch) << 1 for ch in call.ljust(6)) + bytes([0x60 | (ssid << 1) | int(last)])


def ui_frame(to, frm, via=(), text=b""):
    """An APRS-style UI frame: addresses as (call, ssid), control 0x03, protocol 0xf0, the text."""
    addrs = [to, frm] + list(via)
    head = b"".join(address(c, s, i == len(addrs) - 1) for i, (c, s) in enumerate(addrs))
    return head + b"\x03\xf0" + bytes(text)


def densest_bytes_row(n_bytes, seed=1):
    """(row, head): a frame of 510 bytes and one of n_bytes, a single flag between them, no stuffed bit in the second. The first
    call takes `head` bits and ends one bit before the first frame's closing flag completes; the rest, 8 (n_bytes + 2) + 9
    positions, delivers 510 + n_bytes bytes."""
    rng = np.random.default_rng(seed)
    full = bytes((11 * i + 5) & 0xFF for i in range(510))
    while True:
        second = bytes(rng.choice(np.array([0x55, 0x33, 0x0F, 0x5A, 0x00], np.uint8), n_bytes))
        if len(frame_bits(second)) == 8 * (n_bytes + 2):
            break
    row = encode([full, second], shared_flags=True)
    return row, len(row) - (8 * (n_bytes + 2) + 9)
