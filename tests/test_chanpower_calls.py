"""CPU call trace of libsdr_amd.chanpower.ChannelPower, in the manner of tests/test_nodes_calls.py: the wrapper is driven against
that module's fake library, which answers the names of include/sdrhip_chanpower.h as well, refuses what ctypes would refuse
(argument count, each argument through its declared argtype) and records every call. A mistyped entry point, a wrong argument
count or type, a changed router decision or thresholds that are not broadcast show here, without libsdrhip.so's kernels and
without a device."""
import numpy as np
import pytest

from libsdr_amd import abi
from test_nodes_calls import FakeLib, NAMES, Run, count, ramp

M = 8


def _plan_info(args):
    for a, v in zip(args[1:], (8, 3, 576, 6, 384)):
        a._obj.value = v


def _get_state(args):
    args[1]._obj.value = 1234
    args[2]._arr[...] = 2.5
    args[4]._obj.value = 17


def _get_levels(args):
    args[1]._arr[...] = np.arange(M) * 1.5
    args[2]._arr[...] = [0, 1, 0, 0, 1, 1, 0, 0]


def _get_occupied(args):
    assert args[2] == M
    args[1]._arr[:3] = [1, 4, 5]
    args[3]._obj.value = 3


def _run(monkeypatch, seen):
    """`seen`: the threshold arrays the fake was handed, copied at the call"""
    from libsdr_amd import abi_chanpower
    sigs = dict(abi.SIGNATURES, **abi_chanpower.SIGNATURES)
    answers = {"sdrhip_chanpower_plan_info": _plan_info, "sdrhip_chanpower_get_state": _get_state, "sdrhip_chanpower_get_levels": _get_levels,
               "sdrhip_chanpower_get_occupied": _get_occupied,
               "sdrhip_chanpower_set_thresholds": lambda args: seen.append((args[1]._arr.copy(), args[2]._arr.copy()))}
    return Run(monkeypatch, FakeLib(signatures=sigs, answers=answers, scalars_only=True), hook=False)


def test_wrapper_calls_against_the_fake_library(monkeypatch):
    from libsdr_amd import abi_chanpower, chanpower
    seen = []
    r = _run(monkeypatch, seen)
    ctx = r.ctx()
    x = ramp((16, 2), np.int16, 5)
    node = chanpower.ChannelPower(ctx, np.int16, M, 4, np.linspace(0.0, 1.0, 21), alpha=0.125, max_in=64)
    assert (node.dtype, node.M, node.D, node.n_taps, node.max_in, node.alpha) == (0, M, 4, 21, 64, 0.125)
    assert node.kernel_names == NAMES
    assert node.plan_info() == {"tile_times": 8, "branch_taps": 3, "lds_bytes": 576, "grid": 6, "partial_bytes": 384}
    assert node.out_count(16) == count(16)
    s = node.process(x)
    assert s.shape == (M,) and s.dtype == np.float64
    r.route(True)
    routed = node.process(x)                       # through the router: process_dev on ONE row of M doubles
    empty = node.process(x[:0])                    # an empty call never meets the router
    r.route(False)
    assert routed.shape == (M,) and empty.shape == (M,) and not empty.any()
    assert node.process_dev(0x1000, 16, 0x2000) == count(16)
    assert node.process_dev(0x1000, 16) == count(16)            # the state only: a NULL sum
    node.set_thresholds(4e6, 2.5e6)                             # scalars go to every channel
    node.set_thresholds(np.arange(M) + 10.0, 1.0)
    node.set_thresholds(np.full(M, np.inf), np.arange(M, dtype=np.float32))
    assert [(o.tolist(), c.tolist()) for o, c in seen] == [([4e6] * M, [2.5e6] * M), ([k + 10.0 for k in range(M)], [1.0] * M),
                                                           ([np.inf] * M, [float(k) for k in range(M)])]
    assert all(o.dtype == np.float64 and c.dtype == np.float64 for o, c in seen)
    with pytest.raises(ValueError):
        node.set_thresholds(np.ones(M - 1), 0.0)                # neither a scalar nor M values
    node.set_alpha(0.5)
    assert node.alpha == 0.5
    node.set_taps(np.ones(21))
    with pytest.raises(AssertionError):
        node.set_taps(np.ones(20))
    level, flags = node.levels()
    assert level.dtype == np.float64 and level.tolist() == [1.5 * k for k in range(M)]
    assert flags.dtype == bool and flags.tolist() == [False, True, False, False, True, True, False, False]
    occ = node.occupied()
    assert occ == [1, 4, 5] and all(type(k) is int for k in occ)
    st = node.get_state()
    assert st["consumed"] == 1234 and st["calls"] == 17 and st["tail"].shape == (20, 2) and np.all(st["tail"] == 2.5)
    node.reset()
    f = chanpower.ChannelPower(ctx, np.float32, 12, 6, np.ones(30), max_in=64)
    assert (f.dtype, f._in, f.alpha) == (1, (np.float32, 2), 0.25)
    for o in (node, node, f, ctx):
        o.close()
    names = [c[0] for c in r.fake.calls]
    assert names == [
        "sdrhip_ctx_create", "sdrhip_chanpower_create", "sdrhip_chanpower_kernel_names", "sdrhip_chanpower_plan_info",
        "sdrhip_chanpower_out_count", "sdrhip_chanpower_out_count", "sdrhip_chanpower_process",
        "sdrhip_chanpower_out_count", "router", "sdrhip_chanpower_process_dev",
        "sdrhip_chanpower_out_count", "sdrhip_chanpower_process",
        "sdrhip_chanpower_process_dev", "sdrhip_chanpower_process_dev",
        "sdrhip_chanpower_set_thresholds", "sdrhip_chanpower_set_thresholds", "sdrhip_chanpower_set_thresholds",
        "sdrhip_chanpower_set_alpha", "sdrhip_chanpower_set_taps", "sdrhip_chanpower_get_levels", "sdrhip_chanpower_get_occupied",
        "sdrhip_chanpower_get_state", "sdrhip_chanpower_reset", "sdrhip_chanpower_create",
        "sdrhip_chanpower_destroy", "sdrhip_chanpower_destroy", "sdrhip_ctx_destroy"], names
    calls = {}
    for c in r.fake.calls:
        calls.setdefault(c[0], []).append(c[1:])
    # create: (ctx, dtype, M, D, taps, n_taps, max_in, alpha, out)
    assert calls["sdrhip_chanpower_create"][0][1:4] == (0, M, 4) and calls["sdrhip_chanpower_create"][0][5:8] == (21, 64, 0.125)
    assert calls["sdrhip_chanpower_create"][1][1:4] == (1, 12, 6) and calls["sdrhip_chanpower_create"][1][5:8] == (30, 64, 0.25)
    assert len(calls["sdrhip_chanpower_create"][0]) == 9
    assert [c[2] for c in calls["sdrhip_chanpower_process"]] == [16, 0] and all(len(c) == 5 for c in calls["sdrhip_chanpower_process"])
    assert [c[2] for c in calls["sdrhip_chanpower_process_dev"]] == [16, 16, 16] and all(len(c) == 5 for c in calls["sdrhip_chanpower_process_dev"])
    assert calls["sdrhip_chanpower_set_alpha"][0][1] == 0.5
    assert calls["sdrhip_chanpower_get_levels"][0][3] == M and calls["sdrhip_chanpower_get_occupied"][0][2] == M
    assert calls["sdrhip_chanpower_get_state"][0][3] == 20
    assert set(abi_chanpower.SIGNATURES) <= r.fake.reached, sorted(set(abi_chanpower.SIGNATURES) - r.fake.reached)


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    from libsdr_amd import chanpower
    r = _run(monkeypatch, [])
    ctx = r.ctx()
    monkeypatch.setattr(chanpower.ChannelPower, "_calls", chanpower.ChannelPower._calls + " get_levles")
    with pytest.raises(AttributeError, match="sdrhip_chanpower_get_levles"):
        chanpower.ChannelPower(ctx, np.int16, M, 4, np.ones(8))
