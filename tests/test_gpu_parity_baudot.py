"""GPU parity of the Baudot decoder bank (sdrhip_baudot_*, include/sdrhip_baudot.h) with the fixtures the unmodified reference
left (tests/golden/g23_baudot_*, manifest_baudot.json) and with the restatement (tests/baudot_restatement.py): the text bytes,
the counts and (bitstream, bitcount, mode) of every row after every call, bit for bit; there is no tolerance.

The input rows are this test's own device buffers of stride (largest count + 13) whose bytes behind counts[c] are 0xA5 — bit 0
set: a kernel that reads past the count decodes wrongly. The text rows have stride capacity + 5 and a fill pattern that
everything behind out_counts[c] must keep. The shapes are the smallest at which each part of the kernel can go wrong: the
64-position chunk and its neighbours, the three symbol lengths, a symbol, a shift code and a gate decision on either side of a
chunk and of a call boundary."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import baudot_restatement as B
import libsdr_amd as sa
from libsdr_amd import abi_baudot
from redzone import RedZone

pytestmark = pytest.mark.gpu

FILL, BEHIND = 0x5A, 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_baudot.json")))
BITS = np.fromfile(os.path.join(GOLDEN, MANIFEST["bits"]["file"]), np.uint8)
STOPS = (B.STOP1, B.STOP15, B.STOP2)
LENGTHS = [0, 1, 13, 14, 15, 16, 63, 64, 65, 127, 128, 129, 446]


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def traffic(stop, n, seed, lead=0):
    """n half-bits: `lead` idle half-bits, then continuous characters of both tables"""
    r = np.random.default_rng(seed)
    codes = [int(v) for v in r.integers(0, 32, n // 14 + 2)]
    return np.concatenate([np.zeros(lead, np.uint8), B.encode_codes(codes, stop)])[:n].astype(np.uint8)


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)


class Dev:
    """The test's device buffers for `channels` rows of up to max_bits half-bits."""

    def __init__(self, ctx, channels, max_bits):
        self.ctx, self.C, self.max_bits = ctx, channels, max_bits
        self.tstride = B.out_capacity(max_bits) + 5
        self.sizes = (channels * (max_bits + 600), 4 * channels, channels * self.tstride, 4 * channels, 4)
        self.dbits, self.dcnt, self.dtext, self.doutc, self.dstatus = (ctx.malloc(max(b, 16)) for b in self.sizes)

    def call(self, bank, chunks, claim=None):
        """One process_dev call on the rows' chunks; claim: the counts handed to the device where they differ.
        -> (text [C, tstride], out_counts [C], status)"""
        ctx, Cn = self.ctx, self.C
        counts = [len(x) for x in chunks]
        stride = max(counts) + 13
        assert Cn * stride <= self.sizes[0]
        host = np.full((Cn, stride), BEHIND, np.uint8)
        for c in range(Cn):
            host[c, :counts[c]] = chunks[c]
        ctx.h2d(self.dbits, host)
        ctx.h2d(self.dcnt, np.asarray(counts if claim is None else claim, np.uint32))
        ctx.memset(self.dtext, FILL, self.sizes[2]); ctx.memset(self.doutc, FILL, self.sizes[3]); ctx.memset(self.dstatus, FILL, 4)
        bank.process_dev(self.dbits, stride, self.dcnt, self.dtext, self.tstride, self.doutc, self.dstatus)
        ctx.synchronize()
        text, outc, status = np.zeros((Cn, self.tstride), np.uint8), np.zeros(Cn, np.uint32), np.zeros(1, np.uint32)
        ctx.d2h(text, self.dtext); ctx.d2h(outc, self.doutc); ctx.d2h(status, self.dstatus)
        return text, outc, int(status[0])

    def close(self):
        for p in (self.dbits, self.dcnt, self.dtext, self.doutc, self.dstatus):
            self.ctx.free(p)


def check_call(k, got, want_text, bank=None, want_states=None, status=0):
    text, outc, st = got
    assert st == status, (k, st)
    for c, w in enumerate(want_text):
        assert outc[c] == len(w), ("out_counts", k, c, int(outc[c]), len(w))
        assert text[c, :len(w)].tobytes() == w, ("text", k, c, text[c, :len(w)].tobytes(), w)
        assert np.all(text[c, len(w):] == FILL), ("written behind out_counts", k, c)
    if bank is not None:
        for c, s in enumerate(want_states):
            assert bank.channel_state(c) == tuple(s), ("state", k, c, bank.channel_state(c), s)


def drive(ctx, stops, rows, calls, max_bits=None, states_every=1, bank=None, dec=None):
    """rows[c] through a bank of len(rows) nodes in the given calls ([call][row] counts), every call held to the per-bit loop
    of the restatement. -> the bytes every row emitted, per call."""
    own = bank is None
    max_bits = max_bits or (max(1, max(max(c) for c in calls)) if own else bank.max_bits)
    bank = bank or sa.BaudotBank(ctx, stops, max_bits)
    dec = dec or [B.Decoder(s) for s in stops]
    dev = Dev(ctx, len(rows), max_bits)
    try:
        at, out = [0] * len(rows), []
        for k, counts in enumerate(calls):
            chunks = [rows[c][at[c]:at[c] + n] for c, n in enumerate(counts)]
            want = [d.process(x) for d, x in zip(dec, chunks)]
            last = k == len(calls) - 1
            check_call(k, dev.call(bank, chunks), want, bank if (k % states_every == 0 or last) else None, [d.state() for d in dec])
            at = [a + n for a, n in zip(at, counts)]
            out.append(want)
        return out
    finally:
        dev.close()
        if own:
            bank.close()


def test_the_fixtures_call_by_call(ctx):
    """Every fixture case is one row of one bank; call k gives row c its k-th split (nothing once the row is used up). The text
    of every call and the state after it are the reference's own."""
    cases = MANIFEST["cases"]
    stops = [c["stop"] for c in cases]
    n_calls = max(len(c["splits"]) for c in cases)
    longest = max(max(c["splits"]) for c in cases)
    bank, dev = sa.BaudotBank(ctx, stops, longest), Dev(ctx, len(cases), longest)
    dec = [B.Decoder(s) for s in stops]
    try:
        at = [c["offset"] for c in cases]
        for k in range(n_calls):
            counts = [c["splits"][k] if k < len(c["splits"]) else 0 for c in cases]
            chunks = [BITS[a:a + n] for a, n in zip(at, counts)]
            at = [a + n for a, n in zip(at, counts)]
            want = [bytes.fromhex(c["sends"][k] or "") if k < len(c["splits"]) else b"" for c in cases]
            assert want == [d.process(x) for d, x in zip(dec, chunks)]
            states = [c["states"][min(k, len(c["splits"]) - 1)] for c in cases]
            got = dev.call(bank, chunks)
            check_call(k, got, want)
            for c, case in enumerate(cases):   # the state of every row that is still running, and of all after the last call
                if k < len(case["splits"]) or k == n_calls - 1:
                    assert bank.channel_state(c) == tuple(states[c]), ("state", k, c)
    finally:
        dev.close()
        bank.close()


@pytest.mark.parametrize("kind", ["traffic", "noise"])
def test_row_lengths_around_the_chunk_and_the_symbol(ctx, kind):
    stops = [s for s in STOPS for _ in LENGTHS]
    make = (lambda s, n, i: traffic(s, 2 * n + 1, 100 + i, lead=i % 3)) if kind == "traffic" else (lambda s, n, i: noise(2 * n + 1, 200 + i))
    rows = [make(s, n, i) for i, (s, n) in enumerate((s, n) for s in STOPS for n in LENGTHS)]
    lens = [n for _ in STOPS for n in LENGTHS]
    out = drive(ctx, stops, rows, [lens, [n + 1 for n in lens]], max_bits=447)   # a second call goes on from the carried state
    assert sum(len(t) for call in out for t in call) > 100


@pytest.mark.parametrize("stop", STOPS)
def test_a_symbol_that_ends_at_positions_63_64_65(ctx, stop):
    """The window straddles a chunk boundary (one call) and a call boundary (calls of 64 and of 60 half-bits first)."""
    bps = B.PARAMS[stop][1]
    rows = [np.concatenate([np.zeros(p + 1 - bps, np.uint8), B.encode("R4", stop), np.zeros(9, np.uint8)]) for p in (63, 64, 65)]
    n = [r.size for r in rows]
    for calls in ([n], [[64] * 3, [m - 64 for m in n]], [[60] * 3, [4] * 3, [1] * 3, [m - 65 for m in n]]):
        out = drive(ctx, [stop] * 3, rows, calls)
        assert [b"".join(call[c] for call in out) for c in range(3)] == [b"R4"] * 3
    assert drive(ctx, [stop] * 3, rows, [[64] * 3])[0] == [b"R", b"", b""]


@pytest.mark.parametrize("stop", STOPS)
def test_the_gate_at_position_0_of_a_call(ctx, stop):
    """A candidate at position 0: taken with a carried bit count of bitsPerSymbol - 1 or more, refused with one less."""
    stop_h, bps, pattern, mask = B.PARAMS[stop]
    sym = B.encode("K", stop)
    carried = int("".join(str(b) for b in sym[:-1]), 2)   # _bitstream one half-bit before the symbol completes
    rest = np.concatenate([sym[-1:], np.zeros(3, np.uint8), B.encode("M", stop)])
    counts = [bps - 2, bps - 1, bps, 1 << 33, (1 << 64) - 5]
    bank = sa.BaudotBank(ctx, [stop] * len(counts), 64)
    dec = [B.Decoder(stop) for _ in counts]
    try:
        for c, n in enumerate(counts):
            bank.set_channel_state(c, carried, n, B.LETTERS)
            dec[c].bitstream, dec[c].bitcount = carried, n
        out = drive(ctx, [stop] * len(counts), [rest] * len(counts), [[rest.size] * len(counts)], bank=bank, dec=dec)[0]
        # refused at position 0: the gate then opens one half-bit later, inside the stop bits, where nothing matches
        assert out[0] == b"M" and out[1:4] == [b"KM"] * 3
    finally:
        bank.close()


@pytest.mark.parametrize("stop", STOPS)
def test_a_shift_code_at_the_end_of_a_chunk_and_of_a_call(ctx, stop):
    """FIGURES as the last symbol of a chunk (position 63) with the character it governs first in the next chunk, or call."""
    bps = B.PARAMS[stop][1]
    row = np.concatenate([np.zeros(64 - bps, np.uint8), B.encode_codes([B.STF, 23, 1, B.SPA, 1, B.STF, 0, 16, B.STL, 16], stop)])
    for calls in ([[row.size]], [[64], [row.size - 64]], [[64 + bps], [row.size - 64 - bps]]):
        out = drive(ctx, [stop], [row], calls)
        assert b"".join(call[0] for call in out) == b"13 E\0005T"   # code 4 in FIGURES, code 0 a 0 byte
    assert drive(ctx, [stop], [row], [[64]])[0] == [b""]


def test_every_split_of_130_bits_into_two_calls(ctx):
    rows = [np.concatenate([traffic(s, 100, 7 + s, lead=s), noise(30, 9 + s)]) for s in STOPS] + [noise(130, 77 + s) for s in STOPS]
    stops = list(STOPS) * 2
    bank = sa.BaudotBank(ctx, stops, 130)
    try:
        for k in range(131):
            bank.reset()
            drive(ctx, stops, rows, [[k] * 6, [130 - k] * 6], bank=bank, states_every=2)
    finally:
        bank.close()


def test_calls_of_one_bit_over_200_bits(ctx):
    rows = [traffic(s, 200, 31 + s, lead=2) for s in STOPS] + [noise(200, 41 + s) for s in STOPS]
    out = drive(ctx, list(STOPS) * 2, rows, [[1] * 6] * 200, max_bits=1, states_every=8)
    assert sum(len(t) for call in out for t in call[:3]) >= 3 * 12


def test_a_bank_of_67_rows_with_mixed_settings_and_counts(ctx):
    stops = [STOPS[c % 3] for c in range(67)]
    rows = [traffic(stops[c], 900, 300 + c, lead=c % 5) if c % 2 else noise(900, 400 + c) for c in range(67)]
    steps = [0, 446, 1, 64, 15, 200, 0, 65]
    calls = [[steps[(k + c) % len(steps)] for c in range(67)] for k in range(8)]
    out = drive(ctx, stops, rows, calls, max_bits=446, states_every=3)
    assert all(0 in c and len(set(c)) > 3 for c in calls) and sum(len(t) for call in out for t in call) > 500


def test_a_disabled_row_rests_and_resumes(ctx):
    rows = [traffic(B.STOP15, 300, 5), traffic(B.STOP15, 300, 5), traffic(B.STOP2, 300, 6)]
    stops = [B.STOP15, B.STOP15, B.STOP2]
    bank, dev = sa.BaudotBank(ctx, stops, 100, enabled=[True, True, False]), Dev(ctx, 3, 100)
    dec = [B.Decoder(s) for s in stops]
    try:
        assert bank.get_channels() == (stops, [True, True, False])
        check_call(0, dev.call(bank, [r[:100] for r in rows]), [dec[0].process(rows[0][:100]), dec[1].process(rows[1][:100]), b""], bank,
                   [dec[0].state(), dec[1].state(), (0, 0, 0)])
        bank.set_enabled(1, False)
        rested = dec[1].state()
        check_call(1, dev.call(bank, [r[100:200] for r in rows]), [dec[0].process(rows[0][100:200]), b"", b""], bank, [dec[0].state(), rested, (0, 0, 0)])
        bank.set_enabled(1, True)
        bank.set_enabled(2, True)
        assert bank.get_channels() == (stops, [True, True, True])
        # row 1 goes on from the state it had, on bits 200 ... (it never saw 100 ... 200); row 2 starts as a fresh node
        want = [d.process(r[200:300]) for d, r in zip(dec, rows)]
        check_call(2, dev.call(bank, [r[200:300] for r in rows]), want, bank, [d.state() for d in dec])
        assert want[2] and want[0] != want[1]
    finally:
        dev.close()
        bank.close()


def test_set_channel_makes_a_fresh_node_of_one_row(ctx):
    rows = [traffic(B.STOP15, 200, 11), traffic(B.STOP15, 200, 12), traffic(B.STOP15, 200, 13)]
    bank, dev = sa.BaudotBank(ctx, [B.STOP15] * 3, 100), Dev(ctx, 3, 100)
    dec = [B.Decoder(B.STOP15) for _ in range(3)]
    try:
        for c in range(3):   # every row in FIGURES with registers that are not 0
            bank.set_channel_state(c, 0x1234, 7, B.FIGURES)
            dec[c].bitstream, dec[c].bitcount, dec[c].mode = 0x1234, 7, B.FIGURES
        check_call(0, dev.call(bank, [r[:100] for r in rows]), [d.process(r[:100]) for d, r in zip(dec, rows)], bank, [d.state() for d in dec])
        before = [bank.channel_state(c) for c in range(3)]
        bank.set_channel(1, B.STOP1)
        assert [bank.channel_state(c) for c in range(3)] == [before[0], (0, 0, B.LETTERS), before[2]]
        assert bank.get_channels()[0] == [B.STOP15, B.STOP1, B.STOP15]
        dec[1] = B.Decoder(B.STOP1)
        rows[1] = np.concatenate([np.zeros(100, np.uint8), traffic(B.STOP1, 100, 14)])
        check_call(1, dev.call(bank, [r[100:] for r in rows]), [d.process(r[100:]) for d, r in zip(dec, rows)], bank, [d.state() for d in dec])
        for c in (-1, 3):
            for call in (lambda: bank.set_channel(c, B.STOP1), lambda: bank.set_enabled(c, False), lambda: bank.reset_channel(c),
                         lambda: bank.channel_state(c), lambda: bank.set_channel_state(c, 0, 0, 0)):
                with pytest.raises(sa.SdrHipError) as e:
                    call()
                assert e.value.code == sa.abi.E_INVALID and "outside [0,3)" in str(e.value), (c, str(e.value))
        for call in (lambda: bank.set_channel(0, 3), lambda: bank.set_channel_state(0, 0, 0, 2)):
            with pytest.raises(sa.SdrHipError) as e:
                call()
            assert e.value.code == sa.abi.E_INVALID
    finally:
        dev.close()
        bank.close()


def test_reset_with_and_without_keep_mode(ctx):
    bank = sa.Baudot(ctx, 3, 64, stop=B.STOP2)
    try:
        assert bank.get_channels() == ([B.STOP2] * 3, [True] * 3)
        state = [(0xBEEF, 1 << 40, B.FIGURES), (0x0001, 3, B.LETTERS), (0xFFFF, (1 << 64) - 1, B.FIGURES)]
        put = lambda: [bank.set_channel_state(c, *s) for c, s in enumerate(state)]
        put()
        assert [bank.channel_state(c) for c in range(3)] == state   # the round trip, a 64-bit count included
        bank.reset(keep_mode=True)
        assert [bank.channel_state(c) for c in range(3)] == [(0, 0, B.FIGURES), (0, 0, B.LETTERS), (0, 0, B.FIGURES)]
        put()
        bank.reset()
        assert [bank.channel_state(c) for c in range(3)] == [(0, 0, B.LETTERS)] * 3
        put()
        bank.reset_channel(0, keep_mode=True)
        assert [bank.channel_state(c) for c in range(3)] == [(0, 0, B.FIGURES), state[1], state[2]]
        bank.reset_channel(2)
        assert [bank.channel_state(c) for c in range(3)] == [(0, 0, B.FIGURES), state[1], (0, 0, B.LETTERS)]
        # a row that kept FIGURES reads the next character from that table, as the reference's node does after config()
        out = drive(ctx, [B.STOP2] * 3, [B.encode_codes([23], B.STOP2)] * 3, [[16] * 3], bank=bank,
                    dec=[_decoder(B.STOP2, bank.channel_state(c)) for c in range(3)])
        assert out[0][0] == b"1" and out[0][2] == b"Q"
    finally:
        bank.close()


def _decoder(stop, state):
    d = B.Decoder(stop)
    d.bitstream, d.bitcount, d.mode = state
    return d


def test_a_count_above_max_bits_is_clamped_and_reported(ctx):
    MAXB = 100
    rows = [traffic(B.STOP1, 300, 21), traffic(B.STOP15, 300, 22)]
    bank, dev = sa.BaudotBank(ctx, [B.STOP1, B.STOP15], MAXB), Dev(ctx, 2, MAXB)
    dec = [B.Decoder(B.STOP1), B.Decoder(B.STOP15)]
    try:
        got = dev.call(bank, [rows[0][:50], rows[1][:MAXB]], claim=[50, MAXB + 150])
        check_call(0, got, [dec[0].process(rows[0][:50]), dec[1].process(rows[1][:MAXB])], bank, [d.state() for d in dec], status=1)
        # the host-pointer call runs, delivers and answers SDRHIP_E_SIZE
        L = abi_baudot.lib()
        cap = B.out_capacity(MAXB)
        host = np.ascontiguousarray(np.stack([r[:MAXB + 50] for r in rows]))
        cnt = np.array([10, MAXB + 1], np.uint32)
        text, outc = np.zeros((2, cap), np.uint8), np.zeros(2, np.uint32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.sdrhip_baudot_process(bank._h, vp(host), host.shape[1], vp(cnt), vp(text), cap, vp(outc)) == sa.abi.E_SIZE
        assert "max_bits" in L.sdrhip_last_error().decode()
        want = [dec[0].process(host[0, :10]), dec[1].process(host[1, :MAXB])]
        assert [text[c, :outc[c]].tobytes() for c in range(2)] == want and want[1]
        cnt[1] = MAXB
        assert L.sdrhip_baudot_process(bank._h, vp(host), host.shape[1], vp(cnt), vp(text), cap, vp(outc)) == sa.abi.OK
        # a text stride below the capacity is refused before anything runs
        assert L.sdrhip_baudot_process(bank._h, vp(host), host.shape[1], vp(cnt), vp(text), cap - 1, vp(outc)) == sa.abi.E_SIZE
        assert L.sdrhip_baudot_process_dev(bank._h, dev.dbits, 0, dev.dcnt, dev.dtext, cap - 1, dev.doutc, None) == sa.abi.E_SIZE
    finally:
        dev.close()
        bank.close()


def test_a_full_row_of_continuous_stop1_traffic_fills_the_capacity(ctx, redzone):
    """446 half-bits with a symbol completing at position 0 and every 14 behind it: 32 characters, the stated capacity. process()
    runs through the red-zoned arena (tests/redzone.py): the text rows are exactly `capacity` wide between the guard bands."""
    assert RedZone.active and sa.nodes.device_router is not None
    MAXB, Cn = 446, 5
    cap = B.out_capacity(MAXB)
    codes = [1 + (k * 7) % 26 for k in range(40)]
    codes = [c for c in codes if c not in (B.STF, B.STL)]
    stream = B.encode_codes(codes, B.STOP1)
    bank = sa.Baudot(ctx, Cn, MAXB, stop=B.STOP1)
    dec = [B.Decoder(B.STOP1) for _ in range(Cn)]
    try:
        before = RedZone.calls
        head = np.zeros((Cn, MAXB), np.uint8)
        head[:, :13] = stream[:13]
        text, outc = bank.process(head, [13] * Cn)
        assert outc.tolist() == [0] * Cn and [d.process(stream[:13]) for d in dec] == [b""] * Cn
        text, outc = bank.process(np.tile(stream[13:13 + MAXB], (Cn, 1)), [MAXB] * Cn)
        want = dec[0].process(stream[13:13 + MAXB])
        assert len(want) == cap == 32 and text.shape == (Cn, cap)
        assert outc.tolist() == [cap] * Cn and all(text[c].tobytes() == want for c in range(Cn)) and bank.text(Cn - 1) == want
        assert RedZone.calls == before + 2
    finally:
        bank.close()


@pytest.mark.hostptr_only
def test_host_pointer_process_equals_process_dev(ctx):
    assert sa.nodes.device_router is None
    stops = [STOPS[c % 3] for c in range(7)]
    rows = [traffic(stops[c], 700, 50 + c, lead=c) if c % 2 == 0 else noise(700, 60 + c) for c in range(7)]
    steps = [0, 1, 63, 64, 65, 200, 14]
    calls = [[steps[(k + c) % 7] for c in range(7)] for k in range(7)]
    via_dev = drive(ctx, stops, rows, calls, max_bits=200)
    bank = sa.BaudotBank(ctx, stops, 200)
    try:
        cap = B.out_capacity(200)
        assert bank.out_capacity() == cap and bank.out_capacity(446) == 32 and bank.kernel_names == ["baudot_decode_kernel"]
        at = [0] * 7
        for k, counts in enumerate(calls):
            stride = max(counts) + 3
            host = np.full((7, stride), BEHIND, np.uint8)
            for c in range(7):
                host[c, :counts[c]] = rows[c][at[c]:at[c] + counts[c]]
            text, outc = bank.process(host, counts)
            assert text.shape == (7, cap)
            for c, w in enumerate(via_dev[k]):
                assert outc[c] == len(w) and text[c, :len(w)].tobytes() == w == bank.text(c), (k, c)
                assert not text[c, len(w):].any(), ("the bytes behind out_counts arrive as zeros", k, c)
            at = [a + n for a, n in zip(at, counts)]
    finally:
        bank.close()
