"""The decoder bank behind the receiver bank, on the device rows the receiver left: the five-channel plan of
tests/receiver_plan.py, whose ASK channel (row 1: FM, ASKDetector, BitStream 1200 baud NORMAL) here carries an encoded POCSAG
transmission. ReceiverBank.process_dev, then POCSAGBank.process_dev on the same bits / counts buffers with no host copy between
them; the messages have to be what the restatement decodes from the receiver's own bit rows, and row 1's the ones sent."""
import numpy as np
import pytest

import libsdr_amd as sa
import pocsag_restatement as P
import receiver_plan as rp

pytestmark = pytest.mark.gpu

CH = len(rp.CHANNELS)
SENT = [((0x0ABC << 3) | 1, 2, "ON DEVICE", "text"), ((0x0123 << 3) | 5, 0, "555-0199", "numeric")]
CALLS = 13


def pager_bits():
    msgs = [(a, f, P.text_words(s) if kind == "text" else P.numeric_words(s)) for a, f, s, kind in SENT]
    batches = P.frame(msgs)
    assert len(batches) == 1
    return P.transmission(batches, preamble_bits=96, tail=64)


def pager_antenna():
    """One cs16 row of CALLS x 8192 samples: row 1's carrier FM-keyed with the transmission at 1200 baud, row 0's with random
    AFSK, noise of 300."""
    n = CALLS * rp.MAX_IN
    r = np.random.default_rng(20261019)
    t = np.arange(n)
    per = rp.FS / 1200.0
    bits = np.concatenate([pager_bits(), r.integers(0, 2, 64).astype(np.uint8)])
    assert bits.size * per >= n - per
    key = bits[np.minimum((t / per).astype(int), bits.size - 1)]
    s1 = np.exp(1j * (2 * np.pi * rp.CHANNELS[1][0] / rp.FS * t + 2 * np.pi * 2500.0 / rp.FS * np.cumsum(2.0 * key - 1.0)))
    k0 = r.integers(0, 2, bits.size + 2)[(t / per).astype(int)]
    a0 = np.sin(np.cumsum(2 * np.pi * np.where(k0, 2200.0, 1200.0) / rp.FS))
    s0 = np.exp(1j * (2 * np.pi * rp.CHANNELS[0][0] / rp.FS * t + 2 * np.pi * 3000.0 / rp.FS * np.cumsum(a0)))
    x = 3000 * (s0 + s1) + 300 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return np.stack([np.rint(x.real), np.rint(x.imag)], -1).clip(-32768, 32767).astype(np.int16)


def test_pager_messages_from_the_receivers_own_device_rows():
    x = pager_antenna()
    ctx = sa.Context(0)
    comp = rp.components(sa, ctx)
    tuner, deemph, det, bits = comp
    rx = sa.ReceiverBank(ctx, tuner, det, bits, deemph=deemph)
    cap = bits.out_capacity(rp.M)
    bank = sa.POCSAGBank(ctx, CH, cap)
    ecap = bank.out_capacity()
    sizes = (rp.MAX_IN * 4, CH * cap, 4 * CH, 8 * CH * ecap, 4 * CH)
    din, dbits, dcnt, dev, devc = (ctx.malloc(b) for b in sizes)
    asm, dec, ref_asm = sa.MessageAssembler(CH), [P.Decoder() for _ in range(CH)], sa.MessageAssembler(CH)
    got, want, row1 = [], [], []
    try:
        for k in range(CALLS):
            ctx.h2d(din, x[k * rp.MAX_IN:(k + 1) * rp.MAX_IN])
            rx.process_dev(din, rp.MAX_IN, dbits, cap, dcnt)
            bank.process_dev(dbits, cap, dcnt, dev, ecap, devc)     # the same device rows, nothing in between
            ctx.synchronize()
            ev, evc = np.zeros((CH, ecap, 2), np.uint32), np.zeros(CH, np.uint32)
            ctx.d2h(ev, dev); ctx.d2h(evc, devc)
            got += asm.feed(ev, evc)
            # the restatement on the bit rows the receiver left
            b, cnt = np.zeros((CH, cap), np.uint8), np.zeros(CH, np.uint32)
            ctx.d2h(b, dbits); ctx.d2h(cnt, dcnt)
            for c in range(CH):
                e = dec[c].process(b[c, :cnt[c]])
                assert evc[c] == len(e) and ev[c, :len(e)].tolist() == [list(v) for v in e], (k, c)
                want += [(c, m) for m in ref_asm.feed_row(c, np.array(e, np.uint32).reshape(-1, 2))]
            row1.append(b[1, :cnt[1]].copy())
        assert [bank.channel_state(c) for c in range(CH)] == [d.state() for d in dec]
        assert [(c, [m.key() for m in ms]) for c, ms in got] == [(c, [m.key() for m in ms]) for c, ms in want]
        mine = [m for c, ms in got if c == 1 for m in ms]
        assert [(m.address, m.function) for m in mine] == [(a, f) for a, f, _, _ in SENT], (mine, np.concatenate(row1)[:200])
        assert mine[0].as_text().startswith("ON DEVICE") and mine[1].as_numeric().startswith("555-0199")
    finally:
        for p in (din, dbits, dcnt, dev, devc):
            ctx.free(p)
        bank.close()
        rx.close()
        for n in comp:
            n.close()
        ctx.close()
