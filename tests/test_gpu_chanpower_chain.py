"""The scanner loop: the channel power monitor says which channels to select, and a channelizer takes the list. M = 64, D = 32,
512 taps (the windowed sinc of the parity tests), one cs16 antenna row: carriers of amplitude 4000 at the centres of channels 5,
20 and 41 over noise of sigma 200 per component, six calls of 193 * 32 samples, the carriers switched off from call 3 on.
alpha = 0.5, open_thr = 4e6, close_thr = 2.9e6. The restatement's levels per call (tests/chanpower_restatement.py, on the CPU):

    call    carrier channels             largest other channel
    0 - 2   1.54e7, 1.57e7, 1.59e7       <= 7.0e3
    3       8.2e6
    4       4.1e6
    5       2.06e6

so the three channels are occupied behind the calls 0 to 4 — the hysteresis holds them at 4.1e6, above close_thr and hardly above
open_thr — and nothing behind call 5. The scenario is first held to that on the CPU, every compared level at least 10 % away from
the threshold it is compared with; then the device's occupied() behind every call equals the restatement's, and the list read
behind call 0 goes into Channelizer.set_channels: its rows equal the same rows of an all-channels Channelizer bit for bit."""
import functools

import numpy as np
import pytest

import chanpower_restatement as P

M, D, N_TAPS = 64, 32, 512
CARRIERS, AMP, SIGMA = [5, 20, 41], 4000.0, 200.0
CALLS, N_CALL, OFF_FROM = 6, 193 * 32, 3
ALPHA, OPEN_THR, CLOSE_THR = 0.5, 4e6, 2.9e6
TABLE = [1.54e7, 1.57e7, 1.59e7, 8.2e6, 4.1e6, 2.06e6]      # the carrier channels' level behind every call
OTHERS = 7.0e3


def _taps():
    t = np.arange(N_TAPS) - (N_TAPS - 1) / 2
    return np.sinc(t / M) / M * np.hanning(N_TAPS + 2)[1:-1]


@functools.lru_cache(maxsize=None)
def _scenario():
    """(x [CALLS * N_CALL, 2] int16, the restatement's levels [CALLS, M], its occupied list behind every call)"""
    rng = np.random.default_rng(64)
    n = CALLS * N_CALL
    t = np.arange(n)
    x = SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    on = t < OFF_FROM * N_CALL
    for c, k in enumerate(CARRIERS):
        x += on * AMP * np.exp(2j * np.pi * (k * t / M + 0.17 * c))
    x = np.stack([np.round(x.real), np.round(x.imag)], axis=1).astype(np.int16)
    mon = P.Monitor(_taps(), M, D, ALPHA)
    mon.set_thresholds(OPEN_THR, CLOSE_THR)
    levels, occupied = [], []
    for c in range(CALLS):
        mon.process(x[c * N_CALL:(c + 1) * N_CALL])
        levels.append(mon.level.copy())
        occupied.append(mon.occupied())
    return x, np.array(levels), occupied


def test_the_scenario_keeps_its_margins_on_the_cpu():
    _, levels, occupied = _scenario()
    others = [k for k in range(M) if k not in CARRIERS]
    was_open = np.zeros(M, bool)
    for c in range(CALLS):
        # the threshold a level is compared with: close_thr where the flag was set before the call, open_thr elsewhere
        thr = np.where(was_open, CLOSE_THR, OPEN_THR)
        assert np.all(np.abs(levels[c] - thr) >= 0.1 * thr), (c, levels[c][CARRIERS])
        assert np.all(np.abs(levels[c][CARRIERS] - TABLE[c]) <= 0.02 * TABLE[c]), (c, levels[c][CARRIERS])
        assert levels[c][others].max() <= OTHERS, (c, levels[c][others].max())
        was_open = np.isin(np.arange(M), occupied[c])
    assert occupied == [CARRIERS] * 5 + [[]]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


@pytest.mark.gpu
def test_the_monitor_selects_the_channelizers_rows():
    import libsdr_amd as sa
    x, _, occupied = _scenario()
    ctx = sa.Context(0)
    taps = _taps()
    mon = sa.ChannelPower(ctx, np.int16, M, D, taps, alpha=ALPHA, max_in=N_CALL)
    mon.set_thresholds(OPEN_THR, CLOSE_THR)
    picked = sa.Channelizer(ctx, np.int16, M, D, taps, max_in=N_CALL)
    every = sa.Channelizer(ctx, np.int16, M, D, taps, max_in=N_CALL)
    din = ctx.malloc(N_CALL * 4)
    try:
        for c in range(CALLS):
            chunk = np.ascontiguousarray(x[c * N_CALL:(c + 1) * N_CALL])
            ctx.h2d(din, chunk)
            assert mon.process_dev(din, N_CALL) == N_CALL // D            # the state alone: nothing but the list leaves the device
            got = mon.occupied()
            assert got == occupied[c], (c, got)
            if c == 0:
                picked.set_channels(got)                                   # what the monitor read goes in as it is
                assert picked.selected == CARRIERS
            rows, full = picked.process(chunk), every.process(chunk)
            assert rows.shape == (len(CARRIERS), N_CALL // D, 2) and same(rows, full[CARRIERS]), c
            if c < OFF_FROM:
                assert np.hypot(rows[..., 0], rows[..., 1])[:, -50:].min() > 0.9 * AMP   # the carriers are in the picked rows
        level, flags = mon.levels()
        assert not flags.any() and mon.get_state()["calls"] == CALLS and mon.get_state()["consumed"] == CALLS * N_CALL
        assert np.all(level[CARRIERS] < CLOSE_THR) and level.max() == level[CARRIERS].max()
    finally:
        ctx.free(din)
        for v in (mon, picked, every):
            v.close()
        ctx.close()
