"""GPU parity of the POCSAG decoder bank (sdrhip_pocsag_*, include/sdrhip_pocsag.h) with the restatement
(tests/pocsag_restatement.py): events, ev_counts and channel_state, bit for bit; there is no tolerance.

Rows: the golden rows (tests/golden/g19_pocsag_*) and seeded rows — noise, and noise with transmissions in it. 1, 3 and 67
channels, max_bits 2048. Every row set runs once in one call and again split into calls of 0, 1, 31, 32, 33, 63, 64, 65, 543, 544,
545 and 2048 bits, the list rotated by the row index, so the counts of one call differ between the rows and include 0.
The input rows are this test's own device buffers of stride (largest count + 13) whose bytes behind counts[c] are 0xA5 — bit 0
set: a kernel that reads past the count decodes wrongly. The event rows have stride capacity + 5 and a fill pattern that
everything behind ev_counts[c] must keep."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import libsdr_amd as sa
import pocsag_restatement as P
from libsdr_amd import abi_pocsag

pytestmark = pytest.mark.gpu

MAX_BITS = 2048
CAP = P.out_capacity(MAX_BITS)
EV_STRIDE = CAP + 5
FILL, BEHIND = 0x5A, 0xA5
STEPS = [0, 1, 31, 32, 33, 63, 64, 65, 543, 544, 545, 2048]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rows():
    man = json.load(open(os.path.join(GOLDEN, "manifest_pocsag.json")))
    bits = np.fromfile(os.path.join(GOLDEN, man["bits"]["file"]), np.uint8)
    rows = [bits[c["offset"]:c["offset"] + c["n"]].copy() for c in man["cases"] if c["name"] not in ("clean_ragged", "clean_by_7s")]
    r = np.random.default_rng(0x67C5A6)
    tx = P.transmission(P.frame([((0x1F00 << 3) | 6, 1, P.text_words("GPU")), ((0x0042 << 3) | 3, 2, P.numeric_words("4711"))]), preamble_bits=40)
    while len(rows) < 67:
        n = int(r.integers(900, 4200))
        row = r.integers(0, 2, n).astype(np.uint8)
        if len(rows) % 3 == 0:   # a transmission somewhere in the noise, a flipped bit in it, upper bits set
            at = int(r.integers(0, n - tx.size - 1)) if n > tx.size + 1 else 0
            row[at:at + tx.size] = tx[:n - at]
            row[at + int(r.integers(0, min(tx.size, n - at)))] ^= 1
            row |= 0xFE
        rows.append(row)
    return rows


ROWS = _rows()


def schedule(rows, whole):
    """-> [call][row] bit count. whole: one call of each row's first max_bits bits."""
    if whole:
        return [[min(r.size, MAX_BITS) for r in rows]]
    left, calls, k = [r.size for r in rows], [], 0
    while any(left):
        counts = [min(STEPS[(k + c) % len(STEPS)], left[c]) for c in range(len(rows))]
        left = [a - b for a, b in zip(left, counts)]
        calls.append(counts)
        k += 1
    return calls


def expect(rows, calls, enabled=None):
    """-> [call] (events per row, states per row); enabled: [call][row] flags (default: all)"""
    dec, at, out = [P.Decoder() for _ in rows], [0] * len(rows), []
    for k, counts in enumerate(calls):
        ev = []
        for c, n in enumerate(counts):
            on = enabled is None or enabled[k][c]
            ev.append(dec[c].process(rows[c][at[c]:at[c] + n]) if on else [])
            at[c] += n   # (a disabled row's bits pass unread)
        out.append((ev, [d.state() for d in dec]))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


class Dev:
    """The test's device buffers for `channels` rows."""

    def __init__(self, ctx, channels):
        self.ctx, self.C = ctx, channels
        self.bstride = MAX_BITS + 13
        self.sizes = (channels * self.bstride, 4 * channels, 8 * channels * EV_STRIDE, 4 * channels, 4)
        self.dbits, self.dcnt, self.dev, self.devc, self.dstatus = (ctx.malloc(max(b, 16)) for b in self.sizes)

    def call(self, bank, rows, at, counts, claim=None):
        """One process_dev call on rows[c][at[c] : at[c] + counts[c]]; claim: the counts handed to the device where they differ.
        -> (events [C, EV_STRIDE, 2], ev_counts [C], status)"""
        ctx, Cn = self.ctx, self.C
        stride = max(counts) + 13
        host = np.full((Cn, stride), BEHIND, np.uint8)
        for c in range(Cn):
            host[c, :counts[c]] = rows[c][at[c]:at[c] + counts[c]]
        ctx.h2d(self.dbits, host)
        ctx.h2d(self.dcnt, np.asarray(counts if claim is None else claim, np.uint32))
        ctx.memset(self.dev, FILL, self.sizes[2]); ctx.memset(self.devc, FILL, self.sizes[3]); ctx.memset(self.dstatus, FILL, 4)
        bank.process_dev(self.dbits, stride, self.dcnt, self.dev, EV_STRIDE, self.devc, self.dstatus)
        ctx.synchronize()
        ev, evc, status = np.zeros((Cn, EV_STRIDE, 2), np.uint32), np.zeros(Cn, np.uint32), np.zeros(1, np.uint32)
        ctx.d2h(ev, self.dev); ctx.d2h(evc, self.devc); ctx.d2h(status, self.dstatus)
        return ev, evc, int(status[0])

    def close(self):
        for p in (self.dbits, self.dcnt, self.dev, self.devc, self.dstatus):
            self.ctx.free(p)


def check_call(k, got, want_ev, bank=None, want_states=None):
    ev, evc, status = got
    assert status == 0, (k, status)
    pat = np.uint32(FILL * 0x01010101)
    for c, w in enumerate(want_ev):
        assert evc[c] == len(w), ("ev_counts", k, c, int(evc[c]), len(w))
        assert ev[c, :len(w)].tolist() == [list(e) for e in w], ("events", k, c)
        assert np.all(ev[c, len(w):] == pat), ("written behind ev_counts", k, c)
    if bank is not None:
        for c, s in enumerate(want_states):
            assert bank.channel_state(c) == s, ("state", k, c, bank.channel_state(c), s)


def run(ctx, rows, calls, enabled=None, states_every=1):
    want = expect(rows, calls, enabled)
    bank = sa.POCSAGBank(ctx, len(rows), MAX_BITS, None if enabled is None else enabled[0])
    dev = Dev(ctx, len(rows))
    try:
        at = [0] * len(rows)
        for k, counts in enumerate(calls):
            if enabled is not None and k:
                for c in range(len(rows)):
                    if enabled[k][c] != enabled[k - 1][c]:
                        bank.set_enabled(c, enabled[k][c])
                assert bank.enabled() == [bool(e) for e in enabled[k]]
            got = dev.call(bank, rows, at, counts)
            last = k == len(calls) - 1
            check_call(k, got, want[k][0], bank if (k % states_every == 0 or last) else None, want[k][1])
            at = [a + n for a, n in zip(at, counts)]
        return want
    finally:
        dev.close()
        bank.close()


@pytest.mark.parametrize("channels", [1, 3, 67])
@pytest.mark.parametrize("whole", [True, False], ids=["one_call", "split"])
def test_events_counts_and_states_equal_the_restatement(ctx, channels, whole):
    rows = ROWS[:channels]
    calls = schedule(rows, whole)
    want = run(ctx, rows, calls, states_every=1 if channels < 67 else 4)
    # guard against a vacuous pass: the rows leave events of every kind, repaired words among them, and the counts differ
    kinds = [i & 3 for ev, _ in want for row in ev for _, i in row]
    assert {P.SYNC, P.WORD, P.END} <= set(kinds)
    assert any(i & 32 for ev, _ in want for row in ev for _, i in row if i & 3 == P.WORD) or channels == 1
    if not whole and channels > 1:
        assert any(len(set(c)) > 1 and 0 in c for c in calls)


def test_a_disabled_row_rests_and_resumes(ctx):
    rows = [ROWS[0], ROWS[0], ROWS[3]]
    calls = [[300, 300, 300], [400, 400, 400], [64, 64, 64], [ROWS[0].size - 764, ROWS[0].size - 764, ROWS[3].size - 764]]
    enabled = [[1, 1, 1], [1, 0, 1], [1, 0, 0], [1, 1, 1]]
    want = run(ctx, rows, calls, enabled)
    assert want[1][1][1] == want[0][1][1] == want[2][1][1] and want[1][0][1] == [] and want[2][0][2] == []   # the state rested
    assert want[3][0][1] and want[3][0][1] != want[3][0][0]   # row 1 missed the sync word row 0 saw: it decodes the second batch only


def test_reset_channel_leaves_the_others_and_reset_keeps_the_flags(ctx):
    rows = [ROWS[0], ROWS[1], ROWS[2]]
    bank, dev = sa.POCSAGBank(ctx, 3, MAX_BITS, [1, 1, 0]), Dev(ctx, 3)
    try:
        n = 700   # inside the first batch: every enabled row is in RECEIVE
        dev.call(bank, rows, [0, 0, 0], [n, n, n])
        before = [bank.channel_state(c) for c in range(3)]
        assert before[0][0] == before[1][0] == P.RECEIVE and before[2] == (P.WAIT, 0, 0, 0)
        bank.reset_channel(1)
        assert [bank.channel_state(c) for c in range(3)] == [before[0], (P.WAIT, 0, 0, 0), before[2]]
        # row 0 goes on where it was; row 1 is a fresh node reading the row from bit n
        dec0, dec1 = P.Decoder(), P.Decoder()
        dec0.process(rows[0][:n])
        m = rows[0].size - n
        got = dev.call(bank, rows, [n, n, n], [m, m, m])
        check_call(1, got, [dec0.process(rows[0][n:]), dec1.process(rows[1][n:n + m]), []], bank, [dec0.state(), dec1.state(), (P.WAIT, 0, 0, 0)])
        bank.reset()
        assert [bank.channel_state(c) for c in range(3)] == [(P.WAIT, 0, 0, 0)] * 3 and bank.enabled() == [True, True, False]
        fresh = P.Decoder()
        check_call(2, dev.call(bank, rows, [0, 0, 0], [n, 0, n]), [fresh.process(rows[0][:n]), [], []])
    finally:
        dev.close()
        bank.close()


def test_the_row_calls_refuse_a_row_outside_the_bank(ctx):
    """The smallest bank that has two rows to tell apart: 2 rows of 64 bits, one call each. Rows -1 and 2 are refused by
    set_enabled, reset_channel and channel_state with the range in the message and nothing changed; a set_enabled and a
    reset_channel that succeed leave row 0 as it is in a bank never touched."""
    rows, n, at = [ROWS[0], ROWS[1]], 64, 560   # (bits 560 ... 688: the sync word in the first call, two words in the second)
    bank, twin, dev = sa.POCSAGBank(ctx, 2, n), sa.POCSAGBank(ctx, 2, n), Dev(ctx, 2)
    try:
        for c in (-1, 2):
            for call in (lambda: bank.set_enabled(c, False), lambda: bank.reset_channel(c), lambda: bank.channel_state(c)):
                with pytest.raises(sa.SdrHipError) as e:
                    call()
                assert e.value.code == sa.abi.E_INVALID and "outside [0,2)" in str(e.value), (c, str(e.value))
        assert bank.enabled() == [True, True]
        dec = [P.Decoder(), P.Decoder()]
        got = dev.call(bank, rows, [at, at], [n, n])
        check_call(0, got, [d.process(r[at:at + n]) for d, r in zip(dec, rows)], bank, [d.state() for d in dec])
        check_call(0, dev.call(twin, rows, [at, at], [n, n]), got_events(got), twin, [d.state() for d in dec])
        assert dec[1].state()[0] == P.RECEIVE   # (the call did move row 1: the reset below is seen)
        bank.reset_channel(1)
        bank.set_enabled(1, False)
        got = dev.call(bank, rows, [at + n, at + n], [n, n])
        check_call(1, got, [dec[0].process(rows[0][at + n:at + 2 * n]), []], bank, [dec[0].state(), (P.WAIT, 0, 0, 0)])
        und = dev.call(twin, rows, [at + n, at + n], [n, n])
        assert got_events(got)[0] == got_events(und)[0] != [] and bank.channel_state(0) == twin.channel_state(0)
    finally:
        dev.close()
        bank.close()
        twin.close()


def got_events(got):
    """A call's events per row, as lists of pairs."""
    ev, evc, _ = got
    return [[tuple(e) for e in ev[c, :int(evc[c])].tolist()] for c in range(ev.shape[0])]


def test_host_pointer_process_equals_process_dev(ctx):
    rows = ROWS[:7]
    calls = schedule(rows, False)
    want = expect(rows, calls)
    bank = sa.POCSAGBank(ctx, len(rows), MAX_BITS)
    try:
        assert bank.out_capacity() == CAP and bank.out_capacity(446) == 446 // 32 + 446 // 256 + 4
        assert bank.kernel_names == ["pocsag_decode_kernel"]
        at = [0] * len(rows)
        for k, counts in enumerate(calls):
            stride = max(counts) + 3
            host = np.full((len(rows), stride), BEHIND, np.uint8)
            for c in range(len(rows)):
                host[c, :counts[c]] = rows[c][at[c]:at[c] + counts[c]]
            ev, evc = bank.process(host, counts)
            assert ev.shape == (len(rows), CAP, 2)
            for c, w in enumerate(want[k][0]):
                assert evc[c] == len(w) and ev[c, :len(w)].tolist() == [list(e) for e in w], (k, c)
                assert not ev[c, len(w):].any(), ("the events behind ev_counts arrive as zeros", k, c)
            at = [a + n for a, n in zip(at, counts)]
        assert [bank.channel_state(c) for c in range(len(rows))] == want[-1][1]
    finally:
        bank.close()


def test_a_count_above_max_bits_is_clamped_and_reported(ctx):
    noise = next(r for r in ROWS if r.size >= MAX_BITS + 500)
    rows = [ROWS[0], noise]
    bank, dev = sa.POCSAGBank(ctx, 2, MAX_BITS), Dev(ctx, 2)
    try:
        d0, d1 = P.Decoder(), P.Decoder()
        w0, w1 = d0.process(rows[0][:1000]), d1.process(rows[1][:MAX_BITS])
        ev, evc, status = dev.call(bank, rows, [0, 0], [1000, MAX_BITS], claim=[1000, MAX_BITS + 500])
        assert status == 1   # and the call decoded the first max_bits bits of the row
        assert evc.tolist() == [len(w0), len(w1)] and ev[0, :len(w0)].tolist() == [list(e) for e in w0]
        assert [bank.channel_state(c) for c in range(2)] == [d0.state(), d1.state()]
        # the host-pointer call runs and answers SDRHIP_E_SIZE
        L = abi_pocsag.lib()
        host = np.zeros((2, MAX_BITS + 500), np.uint8)
        cnt = np.array([10, MAX_BITS + 1], np.uint32)
        evh, evch = np.zeros((2, CAP, 2), np.uint32), np.zeros(2, np.uint32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.sdrhip_pocsag_process(bank._h, vp(host), host.shape[1], vp(cnt), vp(evh), CAP, vp(evch)) == sa.abi.E_SIZE
        assert "max_bits" in L.sdrhip_last_error().decode()
        with pytest.raises(sa.SdrHipError):
            bank.process(host, cnt)
        cnt[1] = MAX_BITS
        assert L.sdrhip_pocsag_process(bank._h, vp(host), host.shape[1], vp(cnt), vp(evh), CAP, vp(evch)) == sa.abi.OK
        # an event stride below the capacity is refused before anything runs
        assert L.sdrhip_pocsag_process(bank._h, vp(host), host.shape[1], vp(cnt), vp(evh), CAP - 1, vp(evch)) == sa.abi.E_SIZE
        assert L.sdrhip_pocsag_process_dev(bank._h, dev.dbits, 0, dev.dcnt, dev.dev, CAP - 1, dev.devc, None) == sa.abi.E_SIZE
    finally:
        dev.close()
        bank.close()
