"""GPU parity of the AX.25 deframer bank (sdrhip_ax25_*, include/sdrhip_ax25.h) with the fixtures the unmodified reference left
(tests/golden/g24_ax25_*, manifest_ax25.json) and with the restatement (tests/ax25_restatement.py): the frame bytes, the events,
the frame counts and (bitstream, bitbuffer, state, len, rxbuffer) of every row after every call, bit for bit; there is no
tolerance.

The input rows are this test's own device buffers of stride (largest count + 13) whose bytes behind counts[c] are 0xA5 — bit 0
set: a kernel that reads past the count deframes wrongly. The byte rows have stride capacity + 5, the event rows capacity + 2, and
a fill pattern that everything behind a row's frames must keep. The shapes are the smallest at which each part of the kernel can
go wrong: the 64-position chunk and its neighbours, a flag, a stuffed run and a byte on either side of a chunk and of a call
boundary, the buffer's limit, and row counts that are no multiple of the rows of a workgroup."""
import json
import os

import numpy as np
import pytest

import ax25_restatement as R
import libsdr_amd as sa
from libsdr_amd import abi

pytestmark = pytest.mark.gpu

FILL, BEHIND = 0x5A, 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_ax25.json")))
BITS = np.fromfile(os.path.join(GOLDEN, MANIFEST["bits"]["file"]), np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def fnv(data):
    h = 2166136261
    for b in data:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def frame(rng, lo=1, hi=24):
    return bytes(rng.integers(0, 256, int(rng.integers(lo, hi)), dtype=np.uint8))


def traffic(n, seed):
    """n bits of frames between shared and double flags, an abort among them, upper bits set"""
    r = np.random.default_rng(seed)
    rows = []
    while sum(len(x) for x in rows) < n:
        rows.append(R.encode([frame(r) for _ in range(3)], shared_flags=bool(r.integers(0, 2)), idle_flags=int(r.integers(0, 2)),
                             abort_after={1: int(r.integers(1, 30))} if r.integers(0, 4) == 0 else None))
    row = np.concatenate(rows)[:n]
    return (row | (r.integers(0, 128, n).astype(np.uint8) << 1)).astype(np.uint8)


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)


class Dev:
    """The test's device buffers for `channels` rows of up to max_bits bits."""

    def __init__(self, ctx, channels, max_bits):
        self.ctx, self.C, self.max_bits = ctx, channels, max_bits
        self.bstride, self.estride = R.bytes_capacity(max_bits) + 5, R.frames_capacity(max_bits) + 2
        self.sizes = (channels * (max_bits + 600), 4 * channels, channels * self.bstride, 8 * channels * self.estride, 4 * channels, 4)
        self.dbits, self.dcnt, self.dbytes, self.dev, self.dfc, self.dstatus = (ctx.malloc(max(b, 16)) for b in self.sizes)

    def call(self, bank, chunks, claim=None):
        """One process_dev call on the rows' chunks; claim: the counts handed to the device where they differ.
        -> (bytes [C, bstride], events [C, estride, 2], frame_counts [C], status)"""
        ctx, Cn = self.ctx, self.C
        counts = [len(x) for x in chunks]
        stride = max(counts) + 13
        assert Cn * stride <= self.sizes[0]
        host = np.full((Cn, stride), BEHIND, np.uint8)
        for c in range(Cn):
            host[c, :counts[c]] = chunks[c]
        ctx.h2d(self.dbits, host)
        ctx.h2d(self.dcnt, np.asarray(counts if claim is None else claim, np.uint32))
        for p, b in ((self.dbytes, self.sizes[2]), (self.dev, self.sizes[3]), (self.dfc, self.sizes[4]), (self.dstatus, 4)):
            ctx.memset(p, FILL, b)
        bank.process_dev(self.dbits, stride, self.dcnt, self.dbytes, self.bstride, self.dev, self.estride, self.dfc, self.dstatus)
        ctx.synchronize()
        data, ev = np.zeros((Cn, self.bstride), np.uint8), np.zeros((Cn, self.estride, 2), np.uint32)
        fc, status = np.zeros(Cn, np.uint32), np.zeros(1, np.uint32)
        ctx.d2h(data, self.dbytes); ctx.d2h(ev, self.dev); ctx.d2h(fc, self.dfc); ctx.d2h(status, self.dstatus)
        return data, ev, fc, int(status[0])

    def close(self):
        for p in (self.dbits, self.dcnt, self.dbytes, self.dev, self.dfc, self.dstatus):
            self.ctx.free(p)


FILL32 = FILL * 0x01010101


def check_call(k, got, want, bank=None, want_states=None, status=0):
    """want[c]: [(frame, bit index)] of row c in this call"""
    data, ev, fc, st = got
    assert st == status, (k, st)
    for c, found in enumerate(want):
        wdata, wev = R.events(found)
        assert fc[c] == len(found), ("frame_counts", k, c, int(fc[c]), len(found))
        assert ev[c, :len(found)].tolist() == wev, ("events", k, c, ev[c, :len(found)].tolist(), wev)
        assert data[c, :len(wdata)].tobytes() == wdata, ("bytes", k, c)
        assert np.all(data[c, len(wdata):] == FILL), ("written behind the frames' bytes", k, c)
        assert np.all(ev[c, len(found):] == FILL32), ("written behind the events", k, c)
    if bank is not None:
        for c, s in enumerate(want_states):
            assert bank.channel_state(c) == tuple(s), ("state", k, c, bank.channel_state(c)[:4], s[:4])


def drive(ctx, rows, calls, max_bits=None, states_every=1, bank=None, dec=None, enabled=None):
    """rows[c] through a bank of len(rows) nodes in the given calls ([call][row] counts), every call held to the per-bit loop of
    the restatement. -> what every row delivered, per call."""
    own = bank is None
    max_bits = max_bits or (max(1, max(max(c) for c in calls)) if own else bank.max_bits)
    bank = bank or sa.AX25Bank(ctx, len(rows), max_bits, enabled=enabled)
    dec = dec or [R.Decoder() for _ in rows]
    dev = Dev(ctx, len(rows), max_bits)
    try:
        at, out = [0] * len(rows), []
        for k, counts in enumerate(calls):
            chunks = [rows[c][at[c]:at[c] + n] for c, n in enumerate(counts)]
            want = [d.process(x) if enabled is None or enabled[c] else [] for c, (d, x) in enumerate(zip(dec, chunks))]
            last = k == len(calls) - 1
            check_call(k, dev.call(bank, chunks), want, bank if (k % states_every == 0 or last) else None, [d.get_state() for d in dec])
            at = [a + n for a, n in zip(at, counts)]
            out.append(want)
        return out
    finally:
        dev.close()
        if own:
            bank.close()


def split_calls(rows, sizes):
    """[call][row] counts: row c advances by sizes[(k + c) % len(sizes)] in call k until it is used up."""
    left, calls, k = [len(r) for r in rows], [], 0
    while any(left):
        counts = [min(sizes[(k + c) % len(sizes)], n) for c, n in enumerate(left)]
        left = [n - s for n, s in zip(left, counts)]
        calls.append(counts)
        k += 1
    return calls


def test_the_fixtures_call_by_call(ctx):
    """Every fixture case is one row of one bank; call k gives row c its k-th split (nothing once the row is used up). The frames
    of every call and the state after it are the reference's own."""
    cases = MANIFEST["cases"]
    n_calls = max(len(c["splits"]) for c in cases)
    longest = max(max(c["splits"]) for c in cases)
    bank, dev = sa.AX25Bank(ctx, len(cases), longest), Dev(ctx, len(cases), longest)
    dec = [R.Decoder() for _ in cases]
    try:
        at = [c["offset"] for c in cases]
        for k in range(n_calls):
            counts = [c["splits"][k] if k < len(c["splits"]) else 0 for c in cases]
            chunks = [BITS[a:a + n] for a, n in zip(at, counts)]
            at = [a + n for a, n in zip(at, counts)]
            want = [d.process(x) for d, x in zip(dec, chunks)]
            for c, case in enumerate(cases):
                if k < len(case["splits"]):
                    assert [f.hex() for f, _ in want[c]] == [w["raw"] for w in case["frames"][k]]
            check_call(k, dev.call(bank, chunks), want)
            for c, case in enumerate(cases):   # the state of every row that is still running, and of all after the last call
                if k < len(case["splits"]) or k == n_calls - 1:
                    bs, bb, st, ln, rx = bank.channel_state(c)
                    assert [bs, bb, st, ln, fnv(rx)] == case["states"][min(k, len(case["splits"]) - 1)], ("state", k, c)
                    assert (bs, bb, st, ln, rx) == dec[c].get_state()
        for c, case in enumerate(cases):
            assert bank.channel_state(c)[4].hex() == case["rxbuffer"]
    finally:
        dev.close()
        bank.close()


@pytest.mark.parametrize("channels", [1, 5, 9])
def test_call_splits_and_channel_counts(ctx, channels):
    """Traffic and noise rows in calls of 0, 1, 63, 64 and 65 bits, staggered from row to row: a flag, a stuffed run and a byte
    fall on either side of every chunk and call boundary. 5 and 9 rows are no multiple of the rows of a workgroup."""
    rows = [traffic(700, 10 + c) if c % 3 != 2 else noise(700, 10 + c) for c in range(channels)]
    out = drive(ctx, rows, split_calls(rows, [0, 1, 63, 64, 65]), max_bits=65)
    assert sum(len(w) for call in out for w in call) >= 3 * ((channels + 1) // 2)
    whole = drive(ctx, rows, [[700] * channels])
    for c in range(channels):
        assert [f for call in out for f, _ in call[c]] == [f for f, _ in whole[0][c]]


def test_noise_rows(ctx):
    rows = [noise(700, 900 + c) for c in range(9)]
    rows[4] = (np.random.default_rng(4).random(700) < 0.8).astype(np.uint8)     # dense in ones: flags, aborts, stuffed zeros
    drive(ctx, rows, [[700] * 9])
    drive(ctx, rows, split_calls(rows, [97, 128, 1, 200]))


def test_a_clamped_count(ctx):
    rows = [traffic(300, 31), traffic(300, 32), traffic(300, 33)]
    bank, dev = sa.AX25Bank(ctx, 3, 200), Dev(ctx, 3, 300)
    dec = [R.Decoder() for _ in rows]
    try:
        want = [dec[0].process(rows[0][:200]), dec[1].process(rows[1][:150]), dec[2].process(rows[2][:200])]
        got = dev.call(bank, [rows[0], rows[1][:150], rows[2][:200]])
        check_call(0, got, want, bank, [d.get_state() for d in dec], status=1)
        got = dev.call(bank, [rows[0][200:], rows[1][150:], rows[2][200:]])
        check_call(1, got, [dec[0].process(rows[0][200:]), dec[1].process(rows[1][150:]), dec[2].process(rows[2][200:])], bank,
                   [d.get_state() for d in dec], status=0)
        # the host-pointer call runs, delivers and says E_SIZE
        bank.reset()
        with pytest.raises(sa.SdrHipError) as e:
            bank.process(np.stack(rows), [300, 150, 200])
        assert e.value.code == abi.E_SIZE
        fresh = R.Decoder()
        assert bank.frames(0) == fresh.process(rows[0][:200]) and bank.channel_state(0) == fresh.get_state()
    finally:
        dev.close()
        bank.close()


def test_the_host_pointer_call(ctx):
    rows = [traffic(446, 50 + c) for c in range(5)]
    bank = sa.AX25(ctx, 5, 446)
    dec = [R.Decoder() for _ in rows]
    try:
        padded = np.full((5, 460), BEHIND, np.uint8)
        counts = [446, 0, 445, 64, 1]
        for c, n in enumerate(counts):
            padded[c, :n] = rows[c][:n]
        data, ev, fc = bank.process(padded, counts)
        assert data.shape == (5, R.bytes_capacity(446)) and ev.shape == (5, R.frames_capacity(446), 2)
        for c, n in enumerate(counts):
            want = dec[c].process(rows[c][:n])
            assert bank.frames(c) == want and fc[c] == len(want)
            wdata, _ = R.events(want)
            assert not data[c, len(wdata):].any() and not ev[c, len(want):].any()
            assert bank.channel_state(c) == dec[c].get_state()
        assert sum(fc) >= 2
    finally:
        bank.close()


def test_a_disabled_row_keeps_its_state(ctx):
    rows = [traffic(400, 70 + c) for c in range(3)]
    bank, dev = sa.AX25Bank(ctx, 3, 200, enabled=[True, False, True]), Dev(ctx, 3, 200)
    dec = [R.Decoder() for _ in rows]
    try:
        assert bank.get_enabled() == [True, False, True]
        bank.set_channel_state(1, 0x12345678, 0x35, 1, b"stay")
        dec[1].set_state(0x12345678, 0x35, 1, b"stay")
        want = [dec[0].process(rows[0][:200]), [], dec[2].process(rows[2][:200])]
        check_call(0, dev.call(bank, [r[:200] for r in rows]), want, bank, [d.get_state() for d in dec])
        bank.set_enabled(1, True)
        bank.set_enabled(2, False)
        assert bank.get_enabled() == [True, True, False]
        want = [dec[0].process(rows[0][200:]), dec[1].process(rows[1][200:]), []]
        check_call(1, dev.call(bank, [r[200:] for r in rows]), want, bank, [d.get_state() for d in dec])
    finally:
        dev.close()
        bank.close()


def test_the_control_calls(ctx):
    rows = [traffic(300, 80 + c) for c in range(3)]
    bank, dev = sa.AX25Bank(ctx, 3, 300), Dev(ctx, 3, 300)
    dec = [R.Decoder() for _ in rows]
    try:
        assert bank.kernel_names == ["ax25_deframe_kernel"]
        cut = [137, 150, 163]
        check_call(0, dev.call(bank, [r[:n] for r, n in zip(rows, cut)]), [d.process(r[:n]) for d, r, n in zip(dec, rows, cut)], bank,
                   [d.get_state() for d in dec])
        assert any(d.get_state()[3] for d in dec)                     # bytes are buffered
        # the state of row 0 goes to row 2 and back into a decoder: the stream goes on from it, the running CRC recomputed
        s = bank.channel_state(0)
        bank.set_channel_state(2, s[0], s[1], s[2], s[4])
        assert bank.channel_state(2) == s
        dec[2].set_state(s[0], s[1], s[2], s[4])
        bank.reset_channel(1)
        dec[1].config()
        assert bank.channel_state(1) == (0, 0, 0, 0, b"") == dec[1].get_state()
        tails = [rows[0][cut[0]:], rows[1][cut[1]:], rows[0][cut[0]:]]
        want = [d.process(x) for d, x in zip(dec, tails)]
        assert want[0] == want[2] and want[0]
        check_call(1, dev.call(bank, tails), want, bank, [d.get_state() for d in dec])
        bank.reset()
        assert all(bank.channel_state(c) == (0, 0, 0, 0, b"") for c in range(3))
        # states the node cannot reach are refused
        for bad in ((0, 0x80, 2, b""), (0, 0, 1, b""), (0, 0x100, 1, b"")):
            with pytest.raises(sa.SdrHipError) as e:
                bank.set_channel_state(0, *bad)
            assert e.value.code == abi.E_INVALID
        bank.set_channel_state(0, 0, 0x1FF, 0, bytes(512))            # idle behind an overflow: a stale _bitbuffer
        assert bank.channel_state(0) == (0, 0x1FF, 0, 512, bytes(512))
    finally:
        dev.close()
        bank.close()


def test_the_long_row_with_512_and_513_buffered_bytes(ctx):
    full = bytes((7 * i + 3) & 0xFF for i in range(510))
    row = R.encode([full, full + b"!", b"ok"], shared_flags=True)
    row2 = R.encode([full + b"!", full, b"ok"], shared_flags=True, lead_flags=2)
    n = max(len(row), len(row2))
    rows = [np.concatenate([r, np.zeros(n - len(r), np.uint8)]) for r in (row, row2)]
    out = drive(ctx, rows, [[n, n]])
    assert [f for f, _ in out[0][0]] == [full, b"ok"] == [f for f, _ in out[0][1]]
    # in calls: the overflow, and the stale _bitbuffer behind it, carried from call to call
    drive(ctx, rows, split_calls(rows, [4100, 3, 64, 1, 65]), max_bits=4100)
    one = R.encode([full + b"!"])[:-8]
    bank = sa.AX25Bank(ctx, 1, len(one))
    try:
        bank.process(one[None], [len(one)])
        bs, bb, st, ln, rx = bank.channel_state(0)
        assert (st, ln, bb) == (0, 512, 1 | (R.fcs(full + b"!")[1] << 1)) and rx == (full + b"!" + R.fcs(full + b"!"))[:512]
    finally:
        bank.close()


def test_the_densest_rows_fill_what_they_can_and_nothing_behind(ctx):
    u = R.densest_frames_unit()
    k = 18
    row = np.array(list(R.FLAG) + (u + list(R.FLAG)) * k, np.uint8)
    head = 8 + 25 - 1
    n = len(row) - head
    assert n == 25 * (k - 1) + 1 and R.frames_capacity(n) == k
    brow, bhead = R.densest_bytes_row(54)
    bn = len(brow) - bhead
    assert R.bytes_most(bn) == 564 <= R.bytes_capacity(bn)
    # exactly the capacity of the call's own length: max_bits is the second call's count
    for rows, heads, counts in (([row], [head], [n]), ([brow], [bhead], [bn])):
        bank = sa.AX25Bank(ctx, 1, counts[0])
        dev = Dev(ctx, 1, counts[0])
        dec = [R.Decoder()]
        try:
            # the first part in calls of at most max_bits
            at = 0
            while at < heads[0]:
                s = min(counts[0], heads[0] - at)
                check_call(0, dev.call(bank, [rows[0][at:at + s]]), [dec[0].process(rows[0][at:at + s])])
                at += s
            want = [dec[0].process(rows[0][at:])]
            got = dev.call(bank, [rows[0][at:]])
            check_call(1, got, want, bank, [d.get_state() for d in dec])
            if rows[0] is row:
                assert got[2][0] == k == dev.estride - 2 and [i for _, i in want[0]] == list(range(0, n, 25))
            else:
                assert sum(len(f) for f, _ in want[0]) == 564 == R.bytes_most(bn) and want[0][0][1] == 0
        finally:
            dev.close()
            bank.close()
