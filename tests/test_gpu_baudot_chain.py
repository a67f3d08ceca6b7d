"""An RTTY receiver on the device, end to end: AFSK audio (930 / 1100 Hz, 90.90 half-bits per second) -> detector bank ->
bit-stream bank -> Baudot bank, every row handed on as a device pointer, in several calls. Text and counts must equal the
restatement chain's (tests/fsk_restatement.py, tests/baudot_restatement.py) bit for bit, call by call.

The signal is chosen so that the restatement chain itself recovers the sent text once its bit clock has locked (a run of
RY characters in front gives it the transitions to lock on): that is a property of the input, checked on the CPU before the
device output is looked at; it is no tolerance."""
import numpy as np
import pytest

import baudot_restatement as B
import fsk_restatement as F
import libsdr_amd as sa

FS, BAUD, MARK, SPACE = 8000.0, 90.90, 930.0, 1100.0
LOCK = "RYRYRYRY "
TEXTS = ["CQ DE GPU 73", "QTH: 4/6 (OK)", "TEST 1 2 3\nK"]
STOPS = [B.STOP1, B.STOP15, B.STOP2]
CALLS = [4000, 1, 2999, 6000, 87, 88, 89]   # then the rest in one call


def audio():
    """[3, n] int16: row c keys LOCK + TEXTS[c] in setting STOPS[c]; a half-bit of 1 is the 930 Hz tone (the detector's mark)."""
    rows = [np.concatenate([np.zeros(6, np.uint8), B.encode(LOCK + t, s), np.zeros(8, np.uint8)]) for t, s in zip(TEXTS, STOPS)]
    n_half = max(r.size for r in rows)
    n = int(n_half * FS / BAUD)
    k = np.minimum((np.arange(n) * BAUD / FS).astype(np.int64), n_half - 1)
    out = np.zeros((len(rows), n), np.int16)
    for c, r in enumerate(rows):
        half = np.concatenate([r, np.zeros(n_half - r.size, np.uint8)])[k]
        phase = 2 * np.pi * np.cumsum(np.where(half, MARK, SPACE) / FS)
        out[c] = np.rint(8000 * np.sin(phase)).astype(np.int16)
    return out


def splits(n):
    out, left = [], n
    for s in CALLS:
        s = min(s, left)
        if s:
            out.append(s)
            left -= s
    return out + ([left] if left else [])


def restatement_chain(x, mark, space):
    """-> per call: (the rows' bit arrays, the rows' text)"""
    det, bits = F.FSKDetector(mark, space, channels=len(STOPS)), F.BitStream(FS, BAUD, F.NORMAL, channels=len(STOPS))
    dec = [B.Decoder(s) for s in STOPS]
    out, at = [], 0
    for n in splits(x.shape[1]):
        b = bits.process(det.process(x[:, at:at + n]))
        out.append((b, [d.process(r) for d, r in zip(dec, b)]))
        at += n
    return out


def test_the_signal_is_one_the_restatement_chain_reads():
    """No GPU: with the restatement's own LUTs the chain recovers every row's text behind the lock characters."""
    want = restatement_chain(audio(), F.fsk_lut(FS, BAUD, MARK), F.fsk_lut(FS, BAUD, SPACE))
    for c, t in enumerate(TEXTS):
        got = b"".join(call[1][c] for call in want)
        assert got.endswith(t.encode()) and b"RYRY" in got, (c, got)


@pytest.mark.gpu
def test_audio_to_text_on_the_device_equals_the_restatement_chain():
    x = audio()
    Cn, n_all = x.shape
    mark, space = sa.design_fsk_lut(FS, BAUD, MARK), sa.design_fsk_lut(FS, BAUD, SPACE)
    want = restatement_chain(x, mark, space)
    for c, t in enumerate(TEXTS):   # the property of the input, with the LUTs the device uses
        got = b"".join(call[1][c] for call in want)
        assert got.endswith(t.encode()), (c, got)
    ctx = sa.Context(0)
    max_in = max(splits(n_all))
    det = sa.SymbolDetectorBank(ctx, [("fsk", mark, space)] * Cn, max_in=max_in)
    bits = sa.BitStreamBank(ctx, FS, [BAUD] * Cn, [sa.BITS_NORMAL] * Cn, max_in=max_in)
    bcap = bits.out_capacity(max_in)
    bank = sa.BaudotBank(ctx, STOPS, bcap)
    tcap = bank.out_capacity()
    d_in, d_sym, d_bits, d_cnt, d_text, d_outc = (ctx.malloc(b) for b in (2 * Cn * max_in, Cn * max_in, Cn * bcap, 4 * Cn, Cn * tcap, 4 * Cn))
    try:
        at = 0
        for k, n in enumerate(splits(n_all)):
            ctx.h2d(d_in, np.ascontiguousarray(x[:, at:at + n]))
            ctx.memset(d_text, 0x5A, Cn * tcap)
            det.process_dev(d_in, n, n, d_sym, max_in)
            bits.process_dev(d_sym, n, max_in, d_bits, bcap, d_cnt)
            bank.process_dev(d_bits, bcap, d_cnt, d_text, tcap, d_outc)   # the rows and the counts never leave the device
            ctx.synchronize()
            cnt, outc, text = np.zeros(Cn, np.uint32), np.zeros(Cn, np.uint32), np.zeros((Cn, tcap), np.uint8)
            ctx.d2h(cnt, d_cnt); ctx.d2h(outc, d_outc); ctx.d2h(text, d_text)
            wb, wt = want[k]
            assert cnt.tolist() == [len(b) for b in wb], ("bit counts", k)
            for c in range(Cn):
                assert outc[c] == len(wt[c]) and text[c, :outc[c]].tobytes() == wt[c], ("text", k, c, text[c, :outc[c]].tobytes(), wt[c])
                assert np.all(text[c, outc[c]:] == 0x5A), ("written behind out_counts", k, c)
            at += n
        assert [bank.channel_state(c) for c in range(Cn)] == [_final(want, c) for c in range(Cn)]
    finally:
        for p in (d_in, d_sym, d_bits, d_cnt, d_text, d_outc):
            ctx.free(p)
        for o in (bank, bits, det, ctx):
            o.close()


def _final(want, c):
    d = B.Decoder(STOPS[c])
    for b, _ in want:
        d.process(b[c])
    return d.state()
