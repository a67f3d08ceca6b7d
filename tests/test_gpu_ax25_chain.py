"""A packet radio receiver on the device, end to end: AFSK-1200 audio (1200 / 2200 Hz, a zero sent as a change of tone) ->
detector bank -> bit-stream bank (TRANSITION) -> AX.25 bank, every row handed on as a device pointer, in several calls. Frames,
events and counts must equal the restatement chain's (tests/fsk_restatement.py, tests/ax25_restatement.py) bit for bit, call by
call. Three rows carry different frames; a fourth is an RTTY channel (90.90 half-bits per second, NORMAL) whose deframer is
switched off: its bits are produced, and its deframer's state is never touched.

The signal is chosen so that the restatement chain itself recovers the sent frames once its bit clock has locked (the flags in
front give it the transitions to lock on): that is a property of the input, checked on the CPU before the device output is
looked at; it is no tolerance."""
import numpy as np
import pytest

import ax25_restatement as R
import fsk_restatement as F
import libsdr_amd as sa

FS = 22050.0
AX25, RTTY = (1200.0, 1200.0, 2200.0), (90.90, 930.0, 1100.0)     # baud, mark, space
SERVICE = [AX25, AX25, RTTY, AX25]
MODE = [F.TRANSITION, F.TRANSITION, F.NORMAL, F.TRANSITION]
FRAMES = [[R.ui_frame(("APRS", 0), ("DL1ABC", 9), [("WIDE1", 1)], b"!5230.00N/01320.00E>chain"), b"\xff\xff\x7e short"],
          [R.ui_frame(("CQ", 0), ("K1XYZ", 2), text=b">second row"), R.ui_frame(("CQ", 0), ("K1XYZ", 2), text=b"again")],
          None,
          [bytes(range(40, 90))]]
CALLS = [3000, 1, 1999, 2500, 17, 18, 19]   # then the rest in one call
ADVANCE = 9   # samples: the reference's bit clock corrects its rate only, never its phase, so a row starts half a bit into its
#               first bit — the clock's votes then fall into the middle of a tone (0 and 18 lose every frame, 2 ... 16 none)


def keyed(levels, baud, mark, space, n):
    k = np.minimum((np.arange(n) * baud / FS).astype(np.int64), len(levels) - 1)
    phase = 2 * np.pi * np.cumsum(np.where(np.asarray(levels)[k], mark, space) / FS)
    return np.rint(8000 * np.sin(phase)).astype(np.int16)


def audio():
    """[4, n] int16. An AX.25 row keys its encoded bits NRZI — a 0 changes the tone, a 1 keeps it; the RTTY row keys noise."""
    rows = []
    for c, fr in enumerate(FRAMES):
        if fr is None:
            rows.append(np.random.default_rng(3).integers(0, 2, 40).astype(np.uint8))
            continue
        bits = R.encode(fr, lead_flags=10, shared_flags=bool(c == 1), tail=6)
        rows.append(np.cumsum(1 - bits.astype(np.int64)) & 1)
    n = int(max(r.size / s[0] for r, s in zip(rows, SERVICE)) * FS)
    return np.ascontiguousarray(np.stack([keyed(r, *s, n) for r, s in zip(rows, SERVICE)])[:, ADVANCE:])


def splits(n):
    out, left = [], n
    for s in CALLS:
        s = min(s, left)
        if s:
            out.append(s)
            left -= s
    return out + ([left] if left else [])


def restatement_chain(x, luts):
    """-> per call: (the rows' bit arrays, the rows' [(frame, bit index)]); row 2's deframer is off"""
    det = [F.FSKDetector(m, s) for m, s in luts]
    bits = [F.BitStream(FS, s[0], mode) for s, mode in zip(SERVICE, MODE)]
    dec = [R.Decoder() for _ in SERVICE]
    out, at = [], 0
    for n in splits(x.shape[1]):
        b = [bits[c].process(det[c].process(x[c:c + 1, at:at + n]))[0] for c in range(len(SERVICE))]
        out.append((b, [dec[c].process(b[c]) if FRAMES[c] is not None else [] for c in range(len(SERVICE))]))
        at += n
    return out, dec


def check_property(want):
    for c, fr in enumerate(FRAMES):
        got = [f for call in want for f, _ in call[1][c]]
        assert got == (fr or []), (c, got)


def test_the_signal_is_one_the_restatement_chain_reads():
    """No GPU: with the restatement's own LUTs the chain recovers every row's frames."""
    want, _ = restatement_chain(audio(), [(F.fsk_lut(FS, s[0], s[1]), F.fsk_lut(FS, s[0], s[2])) for s in SERVICE])
    check_property(want)


@pytest.mark.gpu
def test_audio_to_frames_on_the_device_equals_the_restatement_chain():
    x = audio()
    Cn, n_all = x.shape
    luts = [(sa.design_fsk_lut(FS, s[0], s[1]), sa.design_fsk_lut(FS, s[0], s[2])) for s in SERVICE]
    want, dec = restatement_chain(x, luts)
    check_property(want)   # the property of the input, with the LUTs the device uses
    ctx = sa.Context(0)
    max_in = max(splits(n_all))
    det = sa.SymbolDetectorBank(ctx, [("fsk", m, s) for m, s in luts], max_in=max_in)
    bits = sa.BitStreamBank(ctx, FS, [s[0] for s in SERVICE], [sa.BITS_TRANSITION if m == F.TRANSITION else sa.BITS_NORMAL for m in MODE], max_in=max_in)
    bcap = bits.out_capacity(max_in)
    bank = sa.AX25Bank(ctx, Cn, bcap, enabled=[fr is not None for fr in FRAMES])
    ycap, ecap = bank.bytes_capacity(), bank.frames_capacity()
    sizes = (2 * Cn * max_in, Cn * max_in, Cn * bcap, 4 * Cn, Cn * ycap, 8 * Cn * ecap, 4 * Cn)
    d_in, d_sym, d_bits, d_cnt, d_bytes, d_ev, d_fc = (ctx.malloc(b) for b in sizes)
    try:
        at = 0
        for k, n in enumerate(splits(n_all)):
            ctx.h2d(d_in, np.ascontiguousarray(x[:, at:at + n]))
            ctx.memset(d_bytes, 0x5A, Cn * ycap)
            ctx.memset(d_ev, 0x5A, 8 * Cn * ecap)
            det.process_dev(d_in, n, n, d_sym, max_in)
            bits.process_dev(d_sym, n, max_in, d_bits, bcap, d_cnt)
            bank.process_dev(d_bits, bcap, d_cnt, d_bytes, ycap, d_ev, ecap, d_fc)   # the rows and the counts never leave the device
            ctx.synchronize()
            cnt, fc = np.zeros(Cn, np.uint32), np.zeros(Cn, np.uint32)
            data, ev = np.zeros((Cn, ycap), np.uint8), np.zeros((Cn, ecap, 2), np.uint32)
            ctx.d2h(cnt, d_cnt); ctx.d2h(fc, d_fc); ctx.d2h(data, d_bytes); ctx.d2h(ev, d_ev)
            wb, wf = want[k]
            assert cnt.tolist() == [len(b) for b in wb], ("bit counts", k)
            for c in range(Cn):
                wdata, wev = R.events(wf[c])
                assert fc[c] == len(wf[c]) and ev[c, :fc[c]].tolist() == wev, ("events", k, c)
                assert data[c, :len(wdata)].tobytes() == wdata, ("bytes", k, c)
                assert np.all(data[c, len(wdata):] == 0x5A) and np.all(ev[c, fc[c]:] == 0x5A5A5A5A), ("written behind the frames", k, c)
            at += n
        assert [bank.channel_state(c) for c in range(Cn)] == [d.get_state() for d in dec]
        assert bank.channel_state(2) == (0, 0, 0, 0, b"")
    finally:
        for p in (d_in, d_sym, d_bits, d_cnt, d_bytes, d_ev, d_fc):
            ctx.free(p)
        for o in (bank, bits, det, ctx):
            o.close()
