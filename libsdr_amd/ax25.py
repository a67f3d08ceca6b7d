"""numpy-facing wrappers over include/sdrhip_ax25.h (libsdr_amd.abi_ax25): the AX.25 deframer bank — the Python mirror of
sdr::gpu::AX25 and sdr::gpu::AX25Bank (include/sdr/gpu/ax25.hh). The reference's AX25 node per row, all rows in one launch: the
bit rows of a BitStreamBank or a ReceiverBank in (an APRS channel: 1200 baud, TRANSITION), CRC-checked frames out. Address and
Message are host-only: the reference's AX25::Address and AX25::Message with the bounds checked."""
import ctypes as C

import numpy as np

from . import abi_ax25, nodes
from .abi import E_SIZE, SdrHipError, check
from .abi_ax25 import RXBUFFER
from .nodes import _Node, _p, _text

__all__ = ["AX25", "AX25Bank", "Address", "Message"]


class AX25Bank(_Node):
    """An AX25 node PER ROW (sdrhip_ax25_create): enabled[c] says whether row c deframes. process(bits, counts) takes host rows;
    process_dev takes the device rows and counts sdrhip_bits_process_dev or ReceiverBank.process_dev left, with no host copy in
    between."""
    _prefix = "sdrhip_ax25"
    _calls = ("frames_capacity bytes_capacity process process_dev set_enabled get_enabled reset reset_channel channel_state "
              "set_channel_state kernel_names")
    _in, _assert_channels = (np.uint8, 0), True

    def __init__(self, ctx, channels, max_bits, enabled=None):
        abi_ax25.lib()
        _Node.__init__(self)
        self.ctx, self.channels, self.max_bits, self._side = ctx, int(channels), int(max_bits), 0
        self._last = None
        en = None if enabled is None else np.ascontiguousarray(np.asarray(enabled, bool), np.intc).ravel()
        assert en is None or en.size == self.channels, (en.size, self.channels)
        check(abi_ax25.lib().sdrhip_ax25_create(ctx.handle, None if en is None else _p(en, True), self.channels, self.max_bits,
                                                C.byref(self._h)))

    def frames_capacity(self, n_bits=None):
        """The frames a row of n_bits bits (default max_bits: the smallest event-row stride) can deliver."""
        return int(self._c_frames_capacity(self.max_bits if n_bits is None else n_bits))

    def bytes_capacity(self, n_bits=None):
        """Room for the frame bytes a row of n_bits bits (default max_bits: the smallest byte-row stride) can deliver."""
        return int(self._c_bytes_capacity(self.max_bits if n_bits is None else n_bits))

    def process_dev(self, bits_ptr, bits_stride, counts_ptr, bytes_ptr, bytes_stride, events_ptr, ev_stride, frame_counts_ptr, status_ptr=0):
        """Device pointers; bytes / events / frame_counts / status as sdrhip_ax25_process_dev leaves them. Nothing is synchronised."""
        check(self._c_process_dev(self._h, C.c_void_p(bits_ptr), bits_stride, C.c_void_p(counts_ptr), C.c_void_p(bytes_ptr), bytes_stride,
                                  C.c_void_p(events_ptr), ev_stride, C.c_void_p(frame_counts_ptr), C.c_void_p(status_ptr) if status_ptr else None))

    def process(self, bits, counts):
        """bits [channels, stride] uint8, counts [channels] -> (bytes [channels, bytes_capacity] uint8, events [channels,
        frames_capacity, 2] uint32, frame_counts [channels] uint32). A count above max_bits raises SdrHipError(E_SIZE). With
        nodes.device_router set the bit and byte rows go through it and process_dev; the counts, the events, the frame counts and
        the status word then pass through a device buffer of the node's own."""
        bits = self._rows(np.ascontiguousarray(bits, np.uint8).reshape(self.channels, -1))
        counts = np.ascontiguousarray(counts, np.uint32)
        assert counts.shape == (self.channels,)
        bcap, fcap, Cn = self.bytes_capacity(), self.frames_capacity(), self.channels
        data, ev, fc = np.zeros((Cn, bcap), np.uint8), np.zeros((Cn, fcap, 2), np.uint32), np.zeros(Cn, np.uint32)
        self._last = (data, ev, fc)
        if nodes.device_router is not None and bits.shape[1]:
            if not self._side:
                self._side = self.ctx.malloc(8 * Cn + 4 + 8 * Cn * fcap)
            side = self._side   # counts, frame counts, status, events
            self.ctx.h2d(side, counts)
            self.ctx.h2d(side + 8 * Cn + 4, ev)
            nodes.device_router(self.ctx, bits, data, lambda i, si, o, so: self.process_dev(i, si, side, o, so, side + 8 * Cn + 4, fcap,
                                                                                            side + 4 * Cn, side + 8 * Cn))
            back = np.zeros(Cn + 1, np.uint32)
            self.ctx.d2h(back, side + 4 * Cn)
            self.ctx.d2h(ev, side + 8 * Cn + 4)
            fc[:] = back[:Cn]
            if back[Cn]:
                raise SdrHipError(E_SIZE, "a row's count exceeds max_bits %d: clamped" % self.max_bits)
            return data, ev, fc
        check(self._c_process(self._h, _p(bits), bits.shape[1], _p(counts), _p(data), bcap, _p(ev), fcap, _p(fc)))
        return data, ev, fc

    def frames(self, c):
        """What row c delivered in the last process() call: [(frame bytes, bit index)]."""
        assert self._last is not None, "no process() call yet"
        data, ev, fc = self._last
        return [(data[c, int(o):int(o) + (int(w) & 0xFFFF)].tobytes(), int(w) >> 16) for o, w in ev[c, :int(fc[c])].tolist()]

    def set_enabled(self, c, enabled):
        check(self._c_set_enabled(self._h, int(c), int(bool(enabled))))

    def get_enabled(self):
        e = (C.c_int * self.channels)()
        check(self._c_get_enabled(self._h, e, self.channels))
        return [bool(v) for v in e]

    def reset(self):
        """Every row a freshly configured node."""
        check(self._c_reset(self._h))

    def reset_channel(self, c):
        check(self._c_reset_channel(self._h, int(c)))

    def channel_state(self, c):
        """-> (bitstream, bitbuffer, state, len, rxbuffer[:len] as bytes) of row c: the reference node's protected members"""
        bs, bb, st, ln = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
        rx = (C.c_uint8 * RXBUFFER)()
        check(self._c_channel_state(self._h, int(c), C.byref(bs), C.byref(bb), C.byref(st), C.byref(ln), rx))
        return bs.value, bb.value, st.value, ln.value, bytes(rx[:ln.value])

    def set_channel_state(self, c, bitstream, bitbuffer, state, rxbuffer=b""):
        rxbuffer = bytes(rxbuffer)
        rx = (C.c_uint8 * RXBUFFER)(*rxbuffer[:RXBUFFER])
        check(self._c_set_channel_state(self._h, int(c), int(bitstream), int(bitbuffer), int(state), len(rxbuffer), rx))

    @property
    def kernel_names(self):
        return _text(self._c_kernel_names, self._h, size=256).split(",")

    def _release(self):
        if self._side:
            self.ctx.free(self._side)
            self._side = 0
        super()._release()


class AX25(AX25Bank):
    """sdr::AX25 on `channels` rows, every row enabled."""

    def __init__(self, ctx, channels, max_bits):
        AX25Bank.__init__(self, ctx, channels, max_bits)


# ---- host only: the frame's addresses and payload -------------------------------------------------------------------------------

class Address:
    """sdr::AX25::Address: a call and an SSID."""

    def __init__(self, call="", ssid=0):
        self.call, self.ssid = call, int(ssid)

    @classmethod
    def unpack(cls, field):
        """The reference's unpackCall on 7 bytes -> (Address, addrExt). The call is the six characters (byte >> 1) cut to the
        NUMBER of those that are no space, as the reference cuts it; the SSID is bits 1 ... 4 of the seventh byte, and another
        address follows where its bit 0 is clear."""
        assert len(field) == 7
        chars = "".join(chr(b >> 1) for b in field[:6])
        return cls(chars[:6 - chars.count(" ")], (field[6] & 0x1F) >> 1), not field[6] & 1

    def __eq__(self, other):
        return isinstance(other, Address) and (self.call, self.ssid) == (other.call, other.ssid)

    def __repr__(self):
        return "Address(%r, %d)" % (self.call, self.ssid)

    def __str__(self):
        return "%s-%d" % (self.call, self.ssid)


class Message:
    """sdr::AX25::Message of one delivered frame (FCS stripped): to, from, via ..., payload — everything behind the address field,
    the control and protocol bytes with it, as the reference keeps it. Where the address field does not fit into the frame (the
    reference reads behind it there) the message is `malformed`: the raw bytes are kept, the addresses stay empty."""

    def __init__(self, raw=b""):
        self.raw, self.to, self.from_, self.via, self.payload, self.malformed = bytes(raw), Address(), Address(), [], b"", False

    @classmethod
    def parse(cls, frame_bytes):
        m = cls(frame_bytes)
        raw, at, via = m.raw, 14, []
        if len(raw) < 14:
            m.malformed = True
            return m
        to, _ = Address.unpack(raw[0:7])
        frm, ext = Address.unpack(raw[7:14])
        while ext:
            if at + 7 > len(raw):
                m.malformed = True
                return m
            a, ext = Address.unpack(raw[at:at + 7])
            via.append(a)
            at += 7
        m.to, m.from_, m.via, m.payload = to, frm, via, raw[at:]
        return m

    def __str__(self):
        """The reference's operator<<, its line break before the payload included; a malformed frame says so in place of the
        addresses and shows its raw bytes."""
        if self.malformed:
            return "malformed N=%d\n%s" % (len(self.raw), self.raw.decode("latin-1"))
        via = " via " + ", ".join(str(a) for a in self.via) if self.via else ""
        return "%s > %s%s N=%d\n%s" % (self.from_, self.to, via, len(self.payload), self.payload.decode("latin-1"))
