"""The five-channel receiver plan of the receiver-bank tests (tests/test_gpu_parity_receiver.py, tests/test_cpp_receiver.py) —
TEST CODE: the antenna, the channel table, the expected values from the CPU references, and the component handles.

Expected values, per row and per call: oracle IQBaseBand<int16_t> -> FMDemod<int16_t> (in-place convention) / AMDemod / USBDemod
-> oracle FMDeemph<int16_t> where enabled -> tests/fsk_restatement.py FSKDetector / ASKDetector -> BitStream.
"""
import numpy as np

import fsk_restatement as fr

FS, D, ORDER = 176400.0, 8, 21
AF = FS / D                                  # 22050 Hz audio: FMDeemph alpha = 2
MAX_IN = 8192
M = (MAX_IN + D - 1) // D                    # the later stages' max_in
LENS = [8192] * 5 + [1000, 0, 1, 7, 513, 4095, 8192, 8192]
N_AUDIO = [1023, 1024, 1024, 1024, 1024, 125, 0, 1, 0, 65, 511, 1024, 1024]
SWITCH = 4                                   # the mid-stream changes happen before the call of this index
AX25, RTTY = (1200.0, 1200.0, 2200.0), (90.90, 930.0, 1100.0)   # baud, mark, space

# Fc, Ff, width, mode, de-emphasis, detector, (baud, BitStream mode)
CHANNELS = [
    (30e3, 30e3, 12.5e3, "fm", True, ("fsk",) + AX25, (1200.0, fr.TRANSITION)),
    (-42e3, -42e3, 12.5e3, "fm", False, ("ask", False), (1200.0, fr.NORMAL)),
    (61e3, 62e3, 2.5e3, "usb", False, ("fsk",) + RTTY, (90.90, fr.NORMAL)),
    (-15e3, -15e3, 9e3, "am", False, ("fsk",) + AX25, (1200.0, fr.NORMAL)),
    (75e3, 75e3, 12.5e3, "fm", True, ("fsk",) + AX25, (1200.0, fr.TRANSITION)),
]
# before call SWITCH, through the component handles
NEW_SHIFT_4 = 74.2e3                         # set_shift on row 4
NEW_MODE_3 = "fm"                            # set_mode AM -> FM on row 3
NEW_DET_2, NEW_BITS_2 = ("fsk",) + AX25, (1200.0, fr.TRANSITION)   # RTTY -> AX.25 on row 2, detector and bit stream
# and set_enabled(0, False)


def antenna():
    """One seeded cs16 row [sum(LENS), 2]: keyed FM / AM / SSB carriers of amplitude about 3000 each, plus noise of 300."""
    n = sum(LENS)
    r = np.random.default_rng(20261019)
    t = np.arange(n)

    def keyed(baud, f0, f1):
        per = FS / baud
        bits = r.integers(0, 2, int(n / per) + 2)
        key = bits[(t / per).astype(int)]
        return np.cumsum(2 * np.pi * np.where(key, f1, f0) / FS), key

    def fm(Fc, audio, dev):
        return np.exp(1j * (2 * np.pi * Fc / FS * t + 2 * np.pi * dev / FS * np.cumsum(audio)))

    a0, _ = keyed(*AX25)
    s0 = fm(30e3, np.sin(a0), 3000.0)
    _, k1 = keyed(1200.0, 0, 0)
    s1 = fm(-42e3, 2.0 * k1 - 1.0, 2500.0)
    a2, _ = keyed(*RTTY)
    s2 = np.exp(1j * (2 * np.pi * 61e3 / FS * t + a2))
    a3, _ = keyed(*AX25)
    s3 = (1 + 0.7 * np.sin(a3)) * np.exp(1j * 2 * np.pi * (-15e3) / FS * t)
    a4, _ = keyed(*AX25)
    s4 = fm(75e3, np.sin(a4), 3000.0)
    x = 3000 * (s0 + s1 + s3 + s4) + 2500 * s2 + 300 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    x = np.stack([np.rint(x.real), np.rint(x.imag)], -1).clip(-32768, 32767).astype(np.int16)
    x.setflags(write=False)
    return x


def _ref_detector(det, lut):
    if det[0] == "ask":
        return lambda a: fr.ask_detect(a, det[1])
    node = fr.FSKDetector(lut(AF, det[1], det[2]), lut(AF, det[1], det[3]))
    return lambda a: node.process(a[None])[0]


class RefRow:
    """One channel as the reference nodes connected in a row."""

    def __init__(self, orc, cfg, lut):
        Fc, Ff, width, mode, de, det, bits = cfg
        self.orc, self.lut = orc, lut
        self.bb = orc.IQBaseBandI16(orc.iqbb_design(Ff, width, FS, ORDER), orc.freqshift_lut_i16(), orc.freqshift_inc(Fc, FS), Fc < 0, D)
        self.set_mode(mode)
        self.deemph, self.enabled = orc.FMDeemphI16(AF), de
        self.set_detector(det)
        self.set_bits(bits)

    def set_mode(self, mode):
        self.mode, self.fm = mode, self.orc.FMDemodI16()

    def set_detector(self, det):
        self.det = _ref_detector(det, self.lut)

    def set_bits(self, bits):
        self.bs = fr.BitStream(AF, bits[0], bits[1])

    def process(self, x):
        """-> (audio the detector read, bits)"""
        y = self.bb.process(x)
        a = self.fm.process(y) if self.mode == "fm" else self.orc.am_i16(y) if self.mode == "am" else self.orc.usb_i16(y)
        a = np.asarray(a, np.int16)
        if not a.size:                       # an empty buffer produces nothing, in any node
            return a, np.zeros(0, np.uint8)
        if self.enabled:
            a = self.deemph.process(a)
        return a, self.bs.process(self.det(a)[None])[0]


def expected(orc, x, changes, lut=fr.fsk_lut):
    """-> [call][row] (audio, bits); changes: the mid-stream changes before call SWITCH. lut(Fs, baud, freq): the FSK LUT
    designer — the restatement's where the product is handed the same arrays, the product's where it designs its own."""
    rows = [RefRow(orc, cfg, lut) for cfg in CHANNELS]
    out, at = [], 0
    for k, n in enumerate(LENS):
        if changes and k == SWITCH:
            rows[4].bb.set_shift(orc.freqshift_inc(NEW_SHIFT_4, FS), NEW_SHIFT_4 < 0)
            rows[3].set_mode(NEW_MODE_3)
            rows[2].set_detector(NEW_DET_2)
            rows[2].set_bits(NEW_BITS_2)
            rows[0].enabled = False
        out.append([r.process(x[at:at + n]) for r in rows])
        at += n
    return out


# ---- the product's side ---------------------------------------------------------------------------------------------------
def _det_cfg(sa, det):
    if det[0] == "ask":
        return ("ask", det[1])
    # (the restatement's LUT on both sides: a different libm must not move a symbol)
    return ("fsk", fr.fsk_lut(AF, det[1], det[2]), fr.fsk_lut(AF, det[1], det[3]))


def components(sa, ctx):
    """-> (tuner, deemph, detector, bits): banks of the five channels, each a handle of its own."""
    EPI = {"fm": sa.EPI_FM, "am": sa.EPI_AM, "usb": sa.EPI_USB}
    taps = np.stack([np.asarray(sa.design_iqbb_taps(Ff, w, FS, ORDER), np.int32).reshape(-1, 2) for _, Ff, w, *_ in CHANNELS])
    tuner = sa.TunerBankI16(ctx, taps, sa.design_freqshift_lut_i16(), [sa.design_freqshift_inc(c[0], FS) for c in CHANNELS],
                            [c[0] < 0 for c in CHANNELS], D, max_in=MAX_IN, modes=[EPI[c[3]] for c in CHANNELS])
    deemph = sa.FMDeemphBankI16(ctx, sa.design_fmdeemph_alpha(AF), [c[4] for c in CHANNELS], max_in=M)
    det = sa.SymbolDetectorBank(ctx, [_det_cfg(sa, c[5]) for c in CHANNELS], max_in=M)
    bits = sa.BitStreamBank(ctx, AF, [c[6][0] for c in CHANNELS], [c[6][1] for c in CHANNELS], max_in=M)
    return tuner, deemph, det, bits


def apply_changes(sa, tuner, deemph, det, bits):
    EPI = {"fm": sa.EPI_FM, "am": sa.EPI_AM, "usb": sa.EPI_USB}
    tuner.set_shift(4, sa.design_freqshift_inc(NEW_SHIFT_4, FS), NEW_SHIFT_4 < 0)
    tuner.set_mode(3, EPI[NEW_MODE_3])
    det.set_channel(2, _det_cfg(sa, NEW_DET_2))
    bits.set_channel(2, NEW_BITS_2[0], NEW_BITS_2[1])
    deemph.set_enabled(0, False)
