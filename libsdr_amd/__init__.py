"""libsdr_amd — MI355X-native libsdr hot path.

The product is `libsdrhip.so` (hand-written HIP for gfx950 behind the C ABI of include/sdrhip.h) and
the header-only C++ nodes of include/sdr/gpu/. This Python package is the ctypes plumbing tests and
bench.py use to reach the C ABI; it contains no compute and no CPU fallback.
"""
from . import abi  # noqa: F401
from .abi import (EPI_NONE, EPI_FM, EPI_AM, EPI_USB, FIR_CS16_EXACT, FIR_CF32, T_CS16, T_CF32,  # noqa: F401
                  FFTCONV_OLA, FFTCONV_OLS, DET_FSK, DET_ASK, BITS_NORMAL, BITS_TRANSITION, SdrHipError)
from .nodes import *  # noqa: F401,F403
from .receiver import FMDeemphBankI16, ReceiverBank  # noqa: F401
from .pocsag import POCSAGBank, MessageAssembler, Message  # noqa: F401
from .agc import AGC, AGCBank, design_agc_lambda, design_agc_target  # noqa: F401
from .psk31 import BPSK31, BPSK31Bank, Varicode, design_inpol_taps  # noqa: F401
from .resample import InpolSubSampler, InpolSubSamplerBank  # noqa: F401
from . import abi_chanreal  # noqa: F401
from .channelizer import Channelizer  # noqa: F401
from .chanaudio import AudioChannelizer  # noqa: F401
from .chanpower import ChannelPower  # noqa: F401
from .changroup import ChannelGroup  # noqa: F401
from .synthesis import Synthesis  # noqa: F401
from . import baudot  # noqa: F401
from .baudot import Baudot, BaudotBank  # noqa: F401
from . import ax25  # noqa: F401
from .ax25 import AX25, AX25Bank  # noqa: F401   (ax25.Address and ax25.Message stay in their module: Message is POCSAG's here)

__version__ = "0.1.0"
