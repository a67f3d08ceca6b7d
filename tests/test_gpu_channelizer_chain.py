"""The channelizer's DEVICE rows as the input of a bank behind it: M = 64, D = 32, a cs16 antenna row with three BPSK31-like
signals on grid channels; the three selected rows, strided as the channelizer left them, go into InpolSubSamplerBank (complex
float) through process_dev with nothing leaving the device in between. The result equals, bit for bit, the resampler bank fed
the same rows through the host, call by call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, D, N_TAPS, FS = 64, 32, 512, 64000.0
CHANNELS = [5, 17, 40]
FRACS = [1.378125, 0.5, 2.0]
CALLS = [4096, 4000, 4192]


def _antenna(n):
    """three carriers at the centres of CHANNELS, each with the phase reversals of a 31.25 baud BPSK signal, and noise"""
    rng = np.random.default_rng(31)
    t = np.arange(n)
    x = 40.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for c, k in enumerate(CHANNELS):
        bits = rng.integers(0, 2, n // 2048 + 2)
        phase = np.cumsum(1 - bits)[t // 2048] % 2          # (a zero bit reverses the phase)
        x += 5000.0 * (1 - 2 * phase) * np.exp(2j * np.pi * (k * t / M + 0.1 * c))
    return np.stack([np.round(x.real), np.round(x.imag)], axis=1).astype(np.int16)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def test_device_rows_into_the_resampler_bank():
    import libsdr_amd as sa
    from libsdr_amd.abi_resample import RESAMPLE_CF32
    ctx = sa.Context(0)
    taps = sa.design_fir_lowpass(N_TAPS, FS / (2 * M), FS)
    x = _antenna(sum(CALLS))
    max_in = max(CALLS)
    rows_cap = -(-max_in // D)
    stride = rows_cap + 11
    chan = sa.Channelizer(ctx, np.int16, M, D, taps, channels=CHANNELS, max_in=max_in)
    chan_host = sa.Channelizer(ctx, np.int16, M, D, taps, channels=CHANNELS, max_in=max_in)
    bank = sa.InpolSubSamplerBank(ctx, RESAMPLE_CF32, FRACS, max_in=rows_cap)
    bank_host = sa.InpolSubSamplerBank(ctx, RESAMPLE_CF32, FRACS, max_in=rows_cap)
    cap = bank.out_capacity(rows_cap)
    C = len(CHANNELS)
    din, drows, dout, dcnt = ctx.malloc(max_in * 4), ctx.malloc(C * stride * 8), ctx.malloc(C * cap * 8), ctx.malloc(4 * C)
    try:
        off, seen = 0, 0
        for n in CALLS:
            chunk = np.ascontiguousarray(x[off:off + n])
            off += n
            ctx.h2d(din, chunk)
            no = chan.process_dev(din, n, drows, stride)
            assert no == chan_host.out_count(n) and 0 < no <= rows_cap
            bank.process_dev(drows, no, stride, dout, cap, dcnt)     # the channelizer's device rows, strided as it left them
            ctx.synchronize()
            out, counts = np.zeros((C, cap, 2), np.float32), np.zeros(C, np.uint32)
            ctx.d2h(out, dout)
            ctx.d2h(counts, dcnt)
            rows = chan_host.process(chunk)                           # the same rows through the host
            assert rows.shape == (C, no, 2) and rows.dtype == np.float32
            want = bank_host.process(rows)
            for c in range(C):
                assert counts[c] == len(want[c]) and same(out[c, :counts[c]], want[c]), (n, c)
            seen += int(counts.sum())
            # the carriers dominate their rows: the chain carried signal, not zeros
            level = np.abs(rows[..., 0].astype(np.float64) + 1j * rows[..., 1])
            assert np.median(level) > 1000.0
        assert seen > 0 and chan.get_state()["consumed"] == sum(CALLS)
    finally:
        for q in (din, drows, dout, dcnt):
            ctx.free(q)
        for v in (chan, chan_host, bank, bank_host):
            v.close()
        ctx.close()
