"""A packet radio receiver on a uniform channel grid, end to end on the device: one cs16 antenna row -> AudioChannelizer (FM rows,
three selected channels) -> FMDeemphBankI16 -> SymbolDetectorBank -> BitStreamBank (TRANSITION) -> AX25Bank, every row handed on
as a device pointer, in a few unequal calls. Each row must deliver exactly the frame sent on its channel, CRC-checked, and the
device chain must equal, bit for bit and call by call, the same handles fed through the host stage by stage.

Where the calls are cut. By the library's per-call FM convention the first output of every call is q.re, not an angle
difference: a click of the carrier's size, ten times the audio's, which costs the bit it falls into (cutting the same stream
inside the frames loses all three on the CPU chain as well). That is the convention's price on every FM path of the library and
not this test's subject, so the five cuts at the front fall into the first five of 24 flags — 19 remain for the bit clock — and
the one at the end into the 30 idle bits behind the longest frame. The CPU chain below is cut in the same places.

The antenna row. Three distinct AX.25 frames (tests/ax25_restatement.py's encoder, 24 flags in front, 30 idle bits behind),
AFSK 1200 with 1200 / 2200 Hz tones, NRZI as tests/test_gpu_ax25_chain.py builds it, each modulated onto the CENTRE of a
different channel of the grid M = 64, D = 32 at an antenna rate of 32 x 22050 Hz (channels 5, 20 and 50 of 11025 Hz each),
plus white noise, rounded to cs16. The transmitter pre-emphasises, as FM packet transmitters do: the carrier's phase follows the tone, 1.364 rad peak, which
is 3 kHz of deviation on the 2200 Hz tone and 1.6 kHz on the 1200 Hz tone. (The reference's FMDemod<int16_t> halves its angle and
then wraps the difference as an int16, so it answers a phase that crosses +-pi with a spike of half the range; a carrier whose
phase stays within +-pi / 2 of its mean never meets that.)

The levels, chosen on the CPU chain of this file (float64 channelizer -> the restatements and the oracle's de-emphasis) before
anything ran on a device: carriers of amplitude 4000 each, noise sigma 200 per component, gain 4 (an FM row sees its carrier at
about 16000 of 32767). With them all three frames decode for every start offset of 0 ... 8 audio samples (START = 4 is the middle
of that run; the reference's bit clock corrects its rate only, never its phase) and for noise up to sigma 1200, six times the
level used."""
import functools

import numpy as np
import pytest

import ax25_restatement as R
import chanaudio_restatement as A
import fsk_restatement as F

AF, M, D, N_TAPS = 22050.0, 64, 32, 512
FS = AF * D
CHANNELS = [5, 20, 50]
BAUD, MARK, SPACE = 1200.0, 1200.0, 2200.0
AMP, NOISE, GAIN, PEAK_DEV, START = 4000.0, 200.0, 4.0, 3000.0, 4
FRAMES = [R.ui_frame(("APRS", 0), ("DL1ABC", 9), [("WIDE1", 1)], b"!5230.00N/01320.00E>grid"),
          R.ui_frame(("CQ", 0), ("K1XYZ", 2), text=b">second channel"), bytes(range(40, 90))]
CALLS, LAST = [9001, 7, 12013, 31, 33], 3000   # antenna samples: the front, then all but the LAST in one call


def taps():
    t = np.arange(N_TAPS) - (N_TAPS - 1) / 2
    return np.sinc(t / M) / M * np.hanning(N_TAPS + 2)[1:-1]


@functools.lru_cache(maxsize=None)
def antenna():
    """[n, 2] int16"""
    levels = [np.cumsum(1 - R.encode([fr], lead_flags=24, tail=30).astype(np.int64)) & 1 for fr in FRAMES]   # NRZI: a 0 changes the tone
    n = int(max(lv.size for lv in levels) / BAUD * FS)
    t = np.arange(n)
    x = np.zeros(n, np.complex128)
    for k, lv in zip(CHANNELS, levels):
        tone = np.where(lv[np.minimum((t * BAUD / FS).astype(np.int64), lv.size - 1)], MARK, SPACE)
        audio = np.sin(2 * np.pi * np.cumsum(tone / FS))
        x += AMP * np.exp(1j * (2 * np.pi * k * (t % M) / M + PEAK_DEV / SPACE * audio))
    rng = np.random.default_rng(9)
    x = (x + NOISE * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))[START * D:]
    out = np.rint(np.stack([x.real, x.imag], -1)).astype(np.int16)
    out.setflags(write=False)
    return out


def splits(n):
    return CALLS + [n - sum(CALLS) - LAST, LAST]


def test_the_signal_is_one_the_cpu_chain_reads(orc):
    """No GPU: a float64 channelizer, the audio restatement cut into the calls' outputs, the oracle's de-emphasis and the FSK /
    AX.25 restatements recover every channel's frame from the antenna row."""
    x = antenna()
    h = np.asarray(taps(), np.float32).astype(np.float64)
    xc, t = x[:, 0].astype(np.float64) + 1j * x[:, 1], np.arange(len(x))
    for k, fr in zip(CHANNELS, FRAMES):
        y = np.convolve(xc * np.exp(-2j * np.pi * k * (t % M) / M), h)[D - 1:len(xc):D]
        y32, rows, ends = np.stack([y.real, y.imag], -1).astype(np.float32)[None], A.Rows([A.FM], [GAIN]), np.cumsum([0] + splits(len(x))) // D
        audio = np.concatenate([rows.process(y32[:, a:b])[0] for a, b in zip(ends[:-1], ends[1:])])
        assert 12000 < np.abs(A.convert(np.stack([y.real, y.imag], -1)[200:], GAIN).astype(np.int32)).max() < 24000
        audio = orc.FMDeemphI16(AF).process(audio)
        sym = F.FSKDetector(F.fsk_lut(AF, BAUD, MARK), F.fsk_lut(AF, BAUD, SPACE)).process(audio[None])
        bits = F.BitStream(AF, BAUD, F.TRANSITION).process(sym)[0]
        assert R.decode(bits) == [fr], k


@pytest.mark.gpu
def test_antenna_to_frames_on_the_device():
    import libsdr_amd as sa
    x = antenna()
    lens, Cn = splits(len(x)), len(CHANNELS)
    max_in = max(lens)
    acap = -(-max_in // D)
    ctx = sa.Context(0)
    node = sa.AudioChannelizer(ctx, np.int16, M, D, taps(), gains=np.full(M, GAIN, np.float32), channels=CHANNELS, max_in=max_in)
    assert node.get_modes() == [sa.EPI_FM] * Cn and node.plan_info()["fm_rows"] == Cn
    deemph = sa.FMDeemphBankI16(ctx, sa.design_fmdeemph_alpha(AF), [True] * Cn, max_in=acap)
    det = sa.SymbolDetectorBank(ctx, [("fsk", sa.design_fsk_lut(AF, BAUD, MARK), sa.design_fsk_lut(AF, BAUD, SPACE))] * Cn, max_in=acap)
    bits = sa.BitStreamBank(ctx, AF, [BAUD] * Cn, [sa.BITS_TRANSITION] * Cn, max_in=acap)
    bcap = bits.out_capacity(acap)
    bank = sa.AX25Bank(ctx, Cn, bcap)
    ycap, ecap = bank.bytes_capacity(), bank.frames_capacity()
    sizes = (4 * max_in, 2 * Cn * acap, 2 * Cn * acap, Cn * acap, Cn * bcap, 4 * Cn, Cn * ycap, 8 * Cn * ecap, 4 * Cn)
    d_in, d_audio, d_de, d_sym, d_bits, d_cnt, d_bytes, d_ev, d_fc = bufs = [ctx.malloc(b) for b in sizes]
    try:
        # the device chain: nothing but the antenna row goes up between the stages, nothing comes down before the chain's end
        dev, at = [], 0
        for n in lens:
            ctx.h2d(d_in, np.ascontiguousarray(x[at:at + n]))
            no = node.process_dev(d_in, n, d_audio, acap)
            assert no == (at + n) // D - at // D
            rec = {"no": no}
            if no:
                deemph.process_dev(d_audio, no, acap, d_de, acap)
                det.process_dev(d_de, no, acap, d_sym, acap)
                bits.process_dev(d_sym, no, acap, d_bits, bcap, d_cnt)
                bank.process_dev(d_bits, bcap, d_cnt, d_bytes, ycap, d_ev, ecap, d_fc)
                ctx.synchronize()
                rec.update(audio=np.zeros((Cn, acap), np.int16), cnt=np.zeros(Cn, np.uint32), bits=np.zeros((Cn, bcap), np.uint8),
                           fc=np.zeros(Cn, np.uint32), data=np.zeros((Cn, ycap), np.uint8), ev=np.zeros((Cn, ecap, 2), np.uint32))
                for name, ptr in (("audio", d_audio), ("cnt", d_cnt), ("bits", d_bits), ("fc", d_fc), ("data", d_bytes), ("ev", d_ev)):
                    ctx.d2h(rec[name], ptr)
            dev.append(rec)
            at += n
        # every row delivers exactly its frame
        for c, fr in enumerate(FRAMES):
            got = []
            for rec in dev:
                for i in range(int(rec["fc"][c]) if rec["no"] else 0):
                    off, ln = int(rec["ev"][c, i, 0]), int(rec["ev"][c, i, 1]) & 0xFFFF
                    got.append(rec["data"][c, off:off + ln].tobytes())
            assert got == [fr], (c, got)
        # the same handles, from their fresh state, fed through the host stage by stage
        for o in (node, deemph, det, bits, bank):
            o.reset()
        at = 0
        for n, rec in zip(lens, dev):
            audio = node.process(x[at:at + n])
            no = rec["no"]
            assert audio.shape == (Cn, no)
            if no:
                assert np.array_equal(audio, rec["audio"][:, :no]), ("audio", at)
                raw, cnt = bits.process_raw(det.process(deemph.process(audio)))
                assert cnt.tolist() == rec["cnt"].tolist(), ("bit counts", at)
                for c in range(Cn):
                    assert np.array_equal(raw[c, :cnt[c]], rec["bits"][c, :cnt[c]]), ("bits", at, c)
                data, ev, fc = bank.process(raw, cnt)
                assert fc.tolist() == rec["fc"].tolist(), ("frame counts", at)
                for c in range(Cn):
                    k = int(fc[c])
                    assert np.array_equal(ev[c, :k], rec["ev"][c, :k]), ("events", at, c)
                    nb = sum(int(e[1]) & 0xFFFF for e in ev[c, :k])
                    assert np.array_equal(data[c, :nb], rec["data"][c, :nb]), ("bytes", at, c)
            at += n
    finally:
        for p in bufs:
            ctx.free(p)
        for o in (bank, bits, det, deemph, node, ctx):
            o.close()
