"""A PSK31 "browser" on the device: one wideband antenna row (64 kS/s) -> tuner bank (SDRHIP_EPI_NONE, / 8, four channels with
one PSK31 signal each, every channel a few Hz off its carrier) -> BPSK31 bank on the tuner's DEVICE rows, no host copy in
between -> Varicode on the host. The bits must equal those of the same rows taken through the host, the decoded text what the
restatement decodes from those rows, and that text holds what was sent."""
import numpy as np
import pytest

import psk31_restatement as R

pytestmark = pytest.mark.gpu

FS, D, ORDER, N = 64000.0, 8, 127, 16384
CARRIERS = [8000.0, -12000.0, 20000.0, -24000.0]
OFFSETS = [2.0, -3.0, 1.0, -1.5]              # what is left for the carrier loop, in Hz
TEXTS = ["hi", "ok", "de", "73"]


def antenna():
    """-> cs16 [n, 2]: the four signals side by side, each 0.15 of full scale, light noise"""
    sent = [R.varicode_bits(t, idle=16) for t in TEXTS]
    n = int((max(len(b) for b in sent) + 5) * (FS / 31.25))
    n = (n + N - 1) // N * N
    t = np.arange(n) / FS
    z = np.zeros(n, complex)
    for c, b in enumerate(sent):
        z += R.modulate(FS, b, n, phase=0.5 * c, amp=0.15) * np.exp(2j * np.pi * (CARRIERS[c] + OFFSETS[c]) * t)
    rng = np.random.default_rng(31)
    z += 0.003 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.rint(np.stack([z.real, z.imag], axis=1) * 32767).astype(np.int16)


def tunes():
    import libsdr_amd as sa
    taps = np.stack([sa.design_iqbb_taps(f, 1000.0, FS, ORDER) for f in CARRIERS])
    return taps, [sa.design_freqshift_inc(f, FS) for f in CARRIERS], [f < 0 for f in CARRIERS]


def test_tuner_bank_to_psk31_bank_on_device_rows():
    import libsdr_amd as sa
    ctx = sa.Context(0)
    x = antenna()
    taps, inc, neg = tunes()
    lut = sa.design_freqshift_lut_i16()
    C = len(CARRIERS)
    cap = N // D + 1
    stride = cap + 24
    tuner = sa.TunerBankI16(ctx, taps, lut, inc, neg, D, max_in=N)
    tuner_host = sa.TunerBankI16(ctx, taps, lut, inc, neg, D, max_in=N)
    psk = sa.BPSK31(ctx, np.int16, FS / D, channels=C, max_in=cap)          # the library's own table
    psk_host = sa.BPSK31(ctx, np.int16, FS / D, channels=C, max_in=cap)
    ref = R.Bank(FS / D, 0.1, sa.design_inpol_taps(), rows=C)
    bcap = psk.out_capacity(cap)
    din, drows, dbits, dcnt = ctx.malloc(N * 4), ctx.malloc(C * stride * 4), ctx.malloc(C * bcap), ctx.malloc(4 * C)
    vd, vh, vr = sa.Varicode(C), sa.Varicode(C), sa.Varicode(C)
    text_dev, text_host, text_ref = [""] * C, [""] * C, [""] * C
    try:
        for k in range(x.shape[0] // N):
            chunk = np.ascontiguousarray(x[k * N:(k + 1) * N])
            ctx.h2d(din, chunk)
            no = tuner.process_dev(din, N, drows, stride)
            assert 0 < no <= cap
            psk.process_dev(drows, no, stride, dbits, bcap, dcnt)    # the tuner's device rows, strided as it left them
            ctx.synchronize()
            bits, counts = np.zeros((C, bcap), np.uint8), np.zeros(C, np.uint32)
            ctx.d2h(bits, dbits)
            ctx.d2h(counts, dcnt)
            dev = [bits[c, :counts[c]] for c in range(C)]
            rows = tuner_host.process(chunk)                         # the same rows through the host
            assert rows.shape == (C, no, 2)
            host = psk_host.process(rows)
            want = ref.process(rows)
            for c in range(C):
                assert np.array_equal(dev[c], host[c]), (k, c)
                assert np.array_equal(dev[c], want[c]), (k, c)
            text_dev = [a + b for a, b in zip(text_dev, vd.feed(dev))]
            text_host = [a + b for a, b in zip(text_host, vh.feed(host))]
            text_ref = [a + b for a, b in zip(text_ref, vr.feed(want))]
        s, sh = psk.get_state(), psk_host.get_state()
        for key in s:
            assert np.array_equal(s[key].view(np.uint32), sh[key].view(np.uint32)), key
        assert text_dev == text_host == text_ref
        for c in range(C):
            assert TEXTS[c] in text_dev[c], (c, text_dev)
    finally:
        for p in (din, drows, dbits, dcnt):
            ctx.free(p)
        for v in (tuner, tuner_host, psk, psk_host):
            v.close()
        ctx.close()
