"""numpy-facing wrapper over include/sdrhip_chanaudio.h (libsdr_amd.abi_chanaudio): the audio channelizer — the polyphase
channelizer with a demodulator (FM, AM or USB) and a gain per channel in the same launch; int16 audio rows out, one per selected
channel, as the symbol path (FMDeemphBankI16 -> SymbolDetectorBank -> BitStreamBank -> the frame decoders) takes them through
process_dev."""
import numpy as np

from . import abi_chanaudio
from .abi import check, EPI_FM
from .channelizer import Channelizer
from .nodes import _p

__all__ = ["AudioChannelizer"]


class AudioChannelizer(Channelizer):
    """The channelizer's y_k[m] times gain[k], rounded to complex<int16>, through channel k's int16 demodulator
    (sdrhip_chanaudio.h has the contract). modes, gains: per CHANNEL, M entries each (None: every channel FM, every gain 1);
    they and the FM angle `last` stay with their channel whatever is selected. set_mode, set_gain, get_modes, get_gains and
    get_state's `last` speak of the rows of the current selection. process(x) returns [rows, n_out] int16; process_dev takes
    device pointers, out_stride in int16 elements."""
    _prefix = "sdrhip_chanaudio"
    _calls = Channelizer._calls + " set_mode get_modes set_gain get_gains"
    _out_dtype = np.int16
    epilogue = EPI_FM   # (any demodulator: the rows are real)
    _abi = abi_chanaudio
    _create_real = "sdrhip_chanreal_audio_create"

    def __init__(self, ctx, dtype, M, D, taps, modes=None, gains=None, channels=None, max_in=65536, real=False):
        """real=True: a row [n] of real samples; modes and gains have M / 2 + 1 entries (sdrhip_chanreal.h)"""
        m = None if modes is None else np.ascontiguousarray(modes, np.intc).ravel()
        g = None if gains is None else np.ascontiguousarray(gains, np.float32).ravel()
        K = int(M) // 2 + 1 if real else int(M)
        assert m is None or m.size == K, (m.size, K)
        assert g is None or g.size == K, (g.size, K)
        super().__init__(ctx, dtype, M, D, taps, channels, max_in, _more=(None if m is None else _p(m, True), None if g is None else _p(g, True)),
                         real=real)

    def set_mode(self, row, mode):
        """Row `row`'s channel gets the demodulator and starts from last = 0."""
        check(self._c_set_mode(self._h, int(row), int(mode)))

    def set_gain(self, row, gain):
        check(self._c_set_gain(self._h, int(row), float(gain)))

    def get_modes(self):
        v = np.zeros(self.channels, np.intc)
        check(self._c_get_modes(self._h, _p(v, True), v.size))
        return [int(a) for a in v]

    def get_gains(self):
        v = np.zeros(self.channels, np.float32)
        check(self._c_get_gains(self._h, _p(v, True), v.size))
        return v

    def get_state(self):
        """-> {consumed, tail (as Channelizer.get_state), last: every row's FM angle [rows] int32} behind the calls enqueued so far"""
        last = np.zeros(self.channels, np.intc)
        consumed, tail = self._tail_state(_p(last, True), last.size)
        return {"consumed": consumed, "tail": tail, "last": last}

    def plan_info(self):
        """{tile_times, branch_taps, lds_bytes, rows, fm_rows, halo_tiles} of a launch (sdrhip_chanaudio_plan_info)"""
        return self._plan_info("tile_times", "branch_taps", "lds_bytes", "rows", "fm_rows", "halo_tiles")
