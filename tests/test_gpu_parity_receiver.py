"""GPU parity of the receiver bank (sdrhip_rxbank_*, include/sdrhip_rx.h): one antenna row in, every channel's bits and audio
out, against (1) the CPU references connected in a row (tests/receiver_plan.py) and (2) the same kinds of component handles
run stage by stage through host arrays. Bit for bit: bits, counts, n_audio and audio rows; there is no tolerance. The bit rows
and audio rows live in this test's own device buffers with a fill pattern, and everything behind counts[c] and n_audio must
keep it.

The plan: 176 400 Hz, 21 taps, /8 (audio 22 050 Hz, FMDeemph alpha = 2), max_in 8192, five channels FM / FM / USB / AM / FM with
AX.25, ASK and RTTY services; calls producing no audio, one sample and no bits are among the 13."""
import ctypes as C

import numpy as np
import pytest

import fsk_restatement as fr
import libsdr_amd as sa
import receiver_plan as rp
from libsdr_amd import abi_rx

pytestmark = pytest.mark.gpu

CH = len(rp.CHANNELS)
FILL = 0x5A


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def x():
    return rp.antenna()


@pytest.fixture(scope="module")
def want(orc, x):
    """[changes][call][row] (audio, bits), computed once and left unchanged"""
    return {ch: rp.expected(orc, x, ch) for ch in (False, True)}


def _close(*nodes):
    for n in nodes:
        n.close()


class Buffers:
    """The test's own device rows: bits [CH, bstride] and audio [CH, astride], refilled with the pattern before every call."""

    def __init__(self, ctx, rows, cap, max_audio, in_bytes):
        self.ctx, self.rows = ctx, rows
        self.bstride, self.astride = cap + 13, max_audio + 5
        self.sizes = (in_bytes, rows * self.bstride, 4 * rows, 2 * rows * self.astride)
        self.din, self.dbits, self.dcnt, self.daud = (ctx.malloc(max(b, 16)) for b in self.sizes)

    def call(self, rx, xin, audio=True):
        ctx, R = self.ctx, self.rows
        if xin.size:
            ctx.h2d(self.din, xin)
        for p, b in ((self.dbits, self.sizes[1]), (self.dcnt, self.sizes[2]), (self.daud, self.sizes[3])):
            ctx.memset(p, FILL, b)
        na = rx.process_dev(self.din, xin.shape[0], self.dbits, self.bstride, self.dcnt, self.daud if audio else 0, self.astride)
        ctx.synchronize()
        bits, cnt, aud = np.zeros((R, self.bstride), np.uint8), np.zeros(R, np.uint32), np.zeros((R, self.astride), np.int16)
        ctx.d2h(bits, self.dbits); ctx.d2h(cnt, self.dcnt); ctx.d2h(aud, self.daud)
        return na, bits, cnt, aud

    def close(self):
        for p in (self.din, self.dbits, self.dcnt, self.daud):
            self.ctx.free(p)


def _check_call(k, got, want_rows, audio=True):
    na, bits, cnt, aud = got
    pat16 = np.int16(FILL | (FILL << 8))
    assert na == want_rows[0][0].size, (k, na)
    for c, (wa, wb) in enumerate(want_rows):
        assert cnt[c] == wb.size and np.array_equal(bits[c, :cnt[c]], wb), ("bits", k, c, int(cnt[c]), wb.size)
        assert np.all(bits[c, cnt[c]:] == FILL), ("written behind the count", k, c)
        if audio:
            assert np.array_equal(aud[c, :na], wa), ("audio", k, c, np.flatnonzero(aud[c, :na] != wa)[:4])
        assert np.all(aud[c, na if audio else 0:] == pat16), ("written behind n_audio", k, c)


@pytest.mark.parametrize("changes", [False, True], ids=["steady", "changes"])
def test_receiver_bank_vs_references_and_stagewise_handles(ctx, x, want, changes):
    want = want[changes]
    # guard against a vacuous pass: the plan produces bits on every row, no row is constant, the counts differ between rows
    totals = [np.concatenate([call[c][1] for call in want]) for c in range(CH)]
    if not changes:
        assert [call[0][0].size for call in want] == rp.N_AUDIO
        assert all(totals[c].size >= 400 for c in (0, 1, 3, 4)) and totals[2].size >= 30
        assert [call[0][1].size for call in want] != [call[4][1].size for call in want]
    assert all(0 < t.sum() < t.size for t in totals)

    comp = rp.components(sa, ctx)
    tuner, deemph, det, bits = comp
    rx = sa.ReceiverBank(ctx, tuner, det, bits, deemph=deemph)
    stage = rp.components(sa, ctx)                    # the same handles again, run one stage at a time through host arrays
    buf = Buffers(ctx, CH, bits.out_capacity(rp.M), rp.M, rp.MAX_IN * 4)
    try:
        at = 0
        for k, n in enumerate(rp.LENS):
            if changes and k == rp.SWITCH:
                rp.apply_changes(sa, *comp)
                rp.apply_changes(sa, *stage)
            xin = x[at:at + n]
            at += n
            na_s, cap_s = rx.sizes(n)
            assert na_s == rp.N_AUDIO[k] and cap_s == bits.out_capacity(na_s) and rx.sizes(n) == (na_s, cap_s)   # (the state rests)
            got = buf.call(rx, xin)
            _check_call(k, got, want[k])
            # stage by stage
            a = stage[0].process(xin)
            assert a.shape == (CH, got[0])
            if a.shape[1]:
                a = stage[1].process(a)
                sb, sc = stage[3].process_raw(stage[2].process(a))
            else:
                sb, sc = np.zeros((CH, 1), np.uint8), np.zeros(CH, np.uint32)
            assert np.array_equal(a, got[3][:, :got[0]]), ("audio vs the stages", k)
            assert np.array_equal(sc, got[2]), ("counts vs the stages", k)
            for c in range(CH):
                assert np.array_equal(sb[c, :sc[c]], got[1][c, :sc[c]]), ("bits vs the stages", k, c)
    finally:
        buf.close()
        rx.close()
        _close(*comp, *stage)


def test_without_audio_and_packed_strides(ctx, x, want):
    """audio = NULL: the same bits, and the audio buffer is never touched; stride 0 = packed rows of this call's sizes."""
    comp = rp.components(sa, ctx)
    rx = sa.ReceiverBank(ctx, comp[0], comp[2], comp[3], deemph=comp[1])
    buf = Buffers(ctx, CH, comp[3].out_capacity(rp.M), rp.M, rp.MAX_IN * 4)
    try:
        at = 0
        for k, n in enumerate(rp.LENS[:2]):
            got = buf.call(rx, x[at:at + n], audio=(k == 1))
            at += n
            _check_call(k, got, want[False][k], audio=(k == 1))
        n = rp.LENS[2]
        na, cap = rx.sizes(n)
        buf.bstride, buf.astride = cap, na                       # what stride 0 must mean
        ctx.h2d(buf.din, x[at:at + n])
        assert rx.process_dev(buf.din, n, buf.dbits, 0, buf.dcnt, buf.daud, 0) == na
        ctx.synchronize()
        b, cnt, aud = np.zeros((CH, cap), np.uint8), np.zeros(CH, np.uint32), np.zeros((CH, na), np.int16)
        ctx.d2h(b, buf.dbits); ctx.d2h(cnt, buf.dcnt); ctx.d2h(aud, buf.daud)
        for c, (wa, wb) in enumerate(want[False][2]):
            assert cnt[c] == wb.size and np.array_equal(b[c, :cnt[c]], wb) and np.array_equal(aud[c], wa), c
        # a stride below the call's need is refused before any stage runs: the next call still matches
        L = abi_rx.lib()
        got = C.c_size_t(0)
        assert L.sdrhip_rxbank_process_dev(rx._h, buf.din, rp.LENS[3], buf.dbits, 3, buf.dcnt, None, 0, C.byref(got)) == sa.abi.E_SIZE
        assert L.sdrhip_rxbank_process_dev(rx._h, buf.din, rp.LENS[3], buf.dbits, 0, buf.dcnt, buf.daud, 5, C.byref(got)) == sa.abi.E_SIZE
        assert L.sdrhip_rxbank_process_dev(rx._h, buf.din, rp.MAX_IN + 1, buf.dbits, 0, buf.dcnt, None, 0, C.byref(got)) == sa.abi.E_SIZE
        buf.bstride, buf.astride = comp[3].out_capacity(rp.M) + 13, rp.M + 5
        _check_call(3, buf.call(rx, x[at + n:at + n + rp.LENS[3]]), want[False][3])
    finally:
        buf.close()
        rx.close()
        _close(*comp)


def test_real_input_tuner_one_parameter_components_host_pointers(ctx, orc):
    """The receiver bank does not care which tuner it got, nor whether a later stage is a bank: a real-input bank of two FM
    rows, no de-emphasis stage, a one-parameter ASK detector and a one-parameter BitStream, through the host-pointer call."""
    Fs, D, order, n_in = 96000.0, 4, 21, 2048
    af = Fs / D
    fc = [12e3, 30e3]
    r = np.random.default_rng(5)
    t = np.arange(3 * n_in + 77)
    key = np.repeat(r.integers(0, 2, t.size // 80 + 2), 80)[:t.size]
    ph = np.cumsum(2 * np.pi * 2000.0 * (2.0 * key - 1.0) / Fs)
    v = 6000 * np.cos(2 * np.pi * fc[0] * t / Fs + ph) + 6000 * np.cos(2 * np.pi * fc[1] * t / Fs - ph) + r.normal(0, 300, t.size)
    xr = np.rint(v).clip(-32768, 32767).astype(np.int16)
    taps = np.stack([np.asarray(sa.design_bb_taps(f, 10e3, Fs, order), np.int32).reshape(-1, 2) for f in fc])
    lut = sa.design_freqshift_lut_i16()
    inc = [sa.design_freqshift_inc(f, Fs) for f in fc]
    tuner = sa.TunerBankI16(ctx, taps, lut, inc, [False, False], D, max_in=n_in, epilogue=sa.EPI_FM, real=True)
    m = n_in // D
    det = sa.ASKDetector(ctx, invert=False, channels=2, max_in=m)
    bits = sa.BitStream(ctx, af, 1200.0, sa.BITS_NORMAL, channels=2, max_in=m)
    rx = sa.ReceiverBank(ctx, tuner, det, bits)
    refs = [(orc.BaseBandI16(orc.bb_design(f, 10e3, Fs, order), orc.freqshift_lut_i16(), orc.freqshift_inc(f, Fs), False, D),
             orc.FMDemodI16(), fr.BitStream(af, 1200.0, fr.NORMAL)) for f in fc]
    total = 0
    try:
        at = 0
        for n in (n_in, 3, 0, n_in - 3, n_in, 77):
            xin = xr[at:at + n]
            at += n
            got_bits, aud = rx.process(xin)
            for c, (bb, fm, bs) in enumerate(refs):
                a = fm.process(bb.process(xin))
                wb = bs.process(fr.ask_detect(a)[None])[0] if a.size else np.zeros(0, np.uint8)
                assert np.array_equal(aud[c], a), (n, c)
                assert np.array_equal(got_bits[c], wb), (n, c)
                total += wb.size
        assert total > 100
    finally:
        rx.close()
        _close(tuner, det, bits)


def test_create_rules(ctx):
    L = abi_rx.lib()
    taps = np.stack([np.asarray(sa.design_iqbb_taps(10e3, 12e3, rp.FS, rp.ORDER), np.int32).reshape(-1, 2)] * 2)
    lut, inc = sa.design_freqshift_lut_i16(), [sa.design_freqshift_inc(10e3, rp.FS)] * 2

    def tuner(epi, max_in=1024):
        return sa.TunerBankI16(ctx, taps, lut, inc, [False, False], rp.D, max_in=max_in, epilogue=epi)

    def create(t, de, d, b):
        h = C.c_void_p(0x1)
        code = L.sdrhip_rxbank_create(ctx.handle, t._h, de._h if de else None, d._h, b._h, C.byref(h))
        if code == sa.abi.OK:
            L.sdrhip_rxbank_destroy(h)
        else:
            assert h.value is None
        return code

    fm, raw = tuner(sa.EPI_FM), tuner(sa.EPI_NONE)
    det, det3, det_small = (sa.ASKDetector(ctx, channels=c, max_in=m) for c, m in ((2, 128), (3, 128), (2, 127)))
    bits, bits_small = (sa.BitStream(ctx, rp.AF, 1200.0, channels=2, max_in=m) for m in (128, 127))
    de, de_small, de3 = (sa.FMDeemphI16(ctx, 2, channels=c, max_in=m) for c, m in ((2, 128), (2, 127), (3, 128)))
    other = sa.Context(0)
    det_other = sa.ASKDetector(other, channels=2, max_in=128)
    try:
        assert create(fm, de, det, bits) == sa.abi.OK and create(fm, None, det, bits) == sa.abi.OK   # 1024 / 8 = 128: just enough
        assert create(raw, de, det, bits) == sa.abi.E_UNSUPPORTED
        assert "cs16" in L.sdrhip_last_error().decode()
        assert create(fm, de, det_other, bits) == sa.abi.E_INVALID
        assert create(raw, de, det_other, bits) == sa.abi.E_INVALID          # the context comes before the row type,
        assert create(raw, de, det3, bits) == sa.abi.E_UNSUPPORTED           # the row type before the channel counts,
        assert create(fm, de, det3, bits_small) == sa.abi.E_INVALID          # and the channel counts before the sizes
        assert create(fm, de3, det, bits) == sa.abi.E_INVALID
        for args in ((fm, de_small, det, bits), (fm, de, det_small, bits), (fm, de, det, bits_small), (fm, None, det, bits_small)):
            assert create(*args) == sa.abi.E_SIZE
            assert "max_in" in L.sdrhip_last_error().decode()
    finally:
        _close(fm, raw, det, det3, det_small, bits, bits_small, de, de_small, de3, det_other)
        other.close()
