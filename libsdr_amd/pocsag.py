"""numpy-facing wrapper over include/sdrhip_pocsag.h (libsdr_amd.abi_pocsag): the POCSAG decoder bank — the Python mirror of
sdr::gpu::POCSAGBank (include/sdr/gpu/pocsag.hh) — and the host half of the decoder: MessageAssembler turns the event rows a
call leaves into pager messages by the rules of the reference's _process_word, _finish_message and handleMessages."""
import ctypes as C

import numpy as np

from . import abi_pocsag
from .abi import check
from .abi_pocsag import SYNC, WORD, END
from .nodes import _Handle, _p, _text

__all__ = ["POCSAGBank", "MessageAssembler", "Message"]

IDLE_WORD = 0x7A89C197
SYNC_WORD = 0x7CD215D8
# the numeric (BCD) alphabet of the POCSAG standard: ten digits, a spare, 'U' (urgency), space, hyphen and the two brackets,
# indexed by the nibble as it sits in the payload (the standard sends a digit's bits LSB first)
BCD = "084 2.6]195-3U7["
_CONTROL = ("NUL SOH STX ETX EOT ENQ ACK BEL BS HT LF VT FF CR SO SI DLE DC1 DC2 DC3 DC4 NAK SYN ETB CAN EM SUB ESC FS GS RS "
            "US").split()


def event_fields(info):
    """info -> (kind, slot, repaired, bit index)"""
    info = int(info)
    return info & 3, (info >> 2) & 7, bool(info & 32), info >> 8


class Message:
    """One pager message: the address word's address (with the slot as its low three bits) and function, and the data words'
    20-bit payloads, concatenated MSB first into bytes (the last byte right-aligned where bits is no multiple of 8, as the
    reference leaves it)."""

    def __init__(self, address, function):
        self.address, self.function, self.bits, self.payload = int(address), int(function), 0, bytearray()

    def add_payload(self, word):
        for i in range(30, 10, -1):
            if self.bits % 8 == 0:
                self.payload.append(0)
            self.payload[-1] = ((self.payload[-1] << 1) | ((word >> i) & 1)) & 0xFF
            self.bits += 1

    def _bit(self, i):
        return (self.payload[i // 8] >> (7 - i % 8)) & 1

    def _chars(self):
        """7-bit characters, the first bit received is the character's LSB"""
        return [sum(self._bit(k * 7 + j) << j for j in range(7)) for k in range(self.bits // 7)]

    def _digits(self):
        n = self.bits // 4   # complete nibbles; an odd last one is read from the low half of its byte
        d = []
        for i in range(n // 2):
            d += [(i, self.payload[i] >> 4), (i, self.payload[i] & 15)]
        if n % 2:
            d.append((n // 2, self.payload[n // 2] & 15))
        return d

    def as_text(self):
        return "".join("<%s>" % _CONTROL[c] if c < 32 else chr(c) for c in self._chars())

    def as_numeric(self):
        return "".join(BCD[v] for _, v in self._digits())

    def estimate_text(self):
        """log-likelihood-like score of the payload being 7-bit text: control characters are rare, punctuation uncommon"""
        score = 0
        for c in self._chars():
            if c < 32 or c == 127:
                score -= 5
            elif 32 < c < 48 or 57 < c < 65 or 90 < c < 97 or 122 < c < 127:
                score -= 2
            else:
                score += 1
        return score

    def estimate_numeric(self):
        """the same for BCD digits; `pos` counts payload bytes, and only the first ten earn a bonus: numeric pages are short"""
        score = 0
        for pos, v in self._digits():
            ch = BCD[v]
            if ch == "U":
                score -= 10
            elif ch in "[]":
                score -= 5
            elif ch in " .-":
                score -= 2
            elif pos < 10:
                score += 5
        return score

    def key(self):
        return self.address, self.function, self.bits, bytes(self.payload)

    def __eq__(self, other):
        return isinstance(other, Message) and self.key() == other.key()

    def __repr__(self):
        return "Message(address=%d, function=%d, bits=%d, payload=%s)" % (self.address, self.function, self.bits, bytes(self.payload).hex())


class MessageAssembler:
    """The host half of `channels` POCSAG nodes. feed() takes the event rows of one call and returns, for every END event in
    channel order, (channel, the messages queued since that channel's last END) — what the reference hands to handleMessages."""

    def __init__(self, channels):
        self.channels = int(channels)
        self._open = [None] * self.channels
        self._queue = [[] for _ in range(self.channels)]

    def _finish(self, c):
        if self._open[c] is not None:
            self._queue[c].append(self._open[c])
            self._open[c] = None

    def feed_row(self, c, events):
        """events: [k, 2] uint32 (word, info) of channel c, in order -> the list of message lists, one per END"""
        released = []
        for word, info in np.asarray(events, np.uint32).reshape(-1, 2).tolist():
            kind, slot, _, _ = event_fields(info)
            if kind == SYNC:
                self._open[c] = None
            elif kind == END:
                self._finish(c)
                released.append(self._queue[c])
                self._queue[c] = []
            elif word == IDLE_WORD:
                self._finish(c)
            elif not word & 0x80000000:   # an address word
                self._finish(c)
                self._open[c] = Message((((word >> 13) & 0x3FFFF) << 3) | slot, (word >> 11) & 3)
            elif self._open[c] is not None:   # a data word; one with no open message is dropped
                self._open[c].add_payload(word)
        return released

    def feed(self, events, ev_counts):
        events = np.asarray(events, np.uint32)
        out = []
        for c in range(self.channels):
            out += [(c, msgs) for msgs in self.feed_row(c, events[c, :int(ev_counts[c])])]
        return out


class POCSAGBank(_Handle):
    """`channels` POCSAG nodes on the device (sdrhip_pocsag_create). process_dev takes the device rows and counts
    sdrhip_bits_process_dev or ReceiverBank.process_dev left, with no host copy in between."""

    def __init__(self, ctx, channels, max_bits, enabled=None):
        L = abi_pocsag.lib()
        self._L, self._h = L, C.c_void_p()
        en = np.ascontiguousarray(np.ones(channels, bool) if enabled is None else np.asarray(enabled, bool), np.intc).ravel()
        assert en.size == channels, (en.size, channels)
        self.ctx, self.channels, self.max_bits = ctx, int(channels), int(max_bits)
        check(L.sdrhip_pocsag_create(ctx.handle, _p(en, True), self.channels, self.max_bits, C.byref(self._h)))

    def _release(self):
        self._L.sdrhip_pocsag_destroy(self._h)

    def out_capacity(self, n_bits=None):
        """The events a row of n_bits bits (default max_bits: the smallest event-row stride) can leave."""
        return int(self._L.sdrhip_pocsag_out_capacity(self.max_bits if n_bits is None else n_bits))

    def process_dev(self, bits_ptr, bits_stride, counts_ptr, events_ptr, ev_stride, ev_counts_ptr, status_ptr=0):
        """Device pointers; events / ev_counts / status as sdrhip_pocsag_process_dev leaves them. Nothing is synchronised."""
        check(self._L.sdrhip_pocsag_process_dev(self._h, C.c_void_p(bits_ptr), bits_stride, C.c_void_p(counts_ptr), C.c_void_p(events_ptr),
                                                ev_stride, C.c_void_p(ev_counts_ptr), C.c_void_p(status_ptr) if status_ptr else None))

    def process(self, bits, counts):
        """bits [channels, stride] uint8, counts [channels] -> (events [channels, capacity, 2] uint32, ev_counts [channels]).
        A count above max_bits raises SdrHipError(E_SIZE)."""
        bits = np.ascontiguousarray(bits, np.uint8).reshape(self.channels, -1)
        counts = np.ascontiguousarray(counts, np.uint32)
        assert counts.shape == (self.channels,)
        cap = self.out_capacity()
        ev, evc = np.zeros((self.channels, cap, 2), np.uint32), np.zeros(self.channels, np.uint32)
        check(self._L.sdrhip_pocsag_process(self._h, _p(bits), bits.shape[1], _p(counts), _p(ev), cap, _p(evc)))
        return ev, evc

    def set_enabled(self, c, enabled):
        check(self._L.sdrhip_pocsag_set_enabled(self._h, int(c), int(bool(enabled))))

    def enabled(self):
        e = (C.c_int * self.channels)()
        check(self._L.sdrhip_pocsag_get_enabled(self._h, e, self.channels))
        return [bool(v) for v in e]

    def reset(self):
        check(self._L.sdrhip_pocsag_reset(self._h))

    def reset_channel(self, c):
        check(self._L.sdrhip_pocsag_reset_channel(self._h, int(c)))

    def channel_state(self, c):
        """-> (state, bitcount, slot, shift64) of row c: the reference node's _state, _bitcount, _slot, _bits"""
        s, b, sl, sh = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
        check(self._L.sdrhip_pocsag_channel_state(self._h, int(c), C.byref(s), C.byref(b), C.byref(sl), C.byref(sh)))
        return s.value, b.value, sl.value, sh.value

    @property
    def kernel_names(self):
        return _text(self._L.sdrhip_pocsag_kernel_names, self._h, size=256).split(",")
