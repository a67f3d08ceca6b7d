"""The audio channelizer's C calls (include/sdrhip_chanaudio.h), what can be checked without a GPU: every function of the header
is exported by libsdrhip.so and has a prototype in libsdr_amd/abi_chanaudio.py, and nothing else of the family is exported; the
header is registered in abi.LATER_SIDE_HEADERS and not in abi.SIDE_HEADERS; every argument rule of create answers BEFORE the
context is looked at, in the header's order — the channelizer's rules, then the modes, then the gains; the calls on a handle
refuse a NULL one; the two kernels exist for gfx950 and use no scratch; and the Python wrapper, driven against the fake library
of tests/test_nodes_calls.py, makes the calls it should."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes
from test_nodes_calls import FakeLib, NAMES, Run, count, ramp

NEW = ["sdrhip_chanaudio_" + n for n in ("create", "destroy", "get_gains", "get_modes", "get_state", "kernel_names", "out_count", "plan_info",
                                         "process", "process_dev", "reset", "set_channels", "set_gain", "set_mode", "set_taps")]
dp, ip, fp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float)
INF, NAN = float("inf"), float("nan")
NONE, FM, AM, USB = abi.EPI_NONE, abi.EPI_FM, abi.EPI_AM, abi.EPI_USB


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_chanaudio
    assert_header_binding(abi_chanaudio, NEW, r"\b(sdrhip_chanaudio[a-z0-9_]*)\b")


def test_the_header_is_in_the_second_table_only():
    import libsdr_amd  # noqa: F401   (the package imports every side header's module)
    from libsdr_amd import abi_chanaudio, abi_channelizer
    assert "sdrhip_chanaudio.h" in abi.LATER_SIDE_HEADERS and "sdrhip_chanaudio.h" not in abi.SIDE_HEADERS
    assert abi.LATER_SIDE_HEADERS["sdrhip_chanaudio.h"].SIGNATURES is abi_chanaudio.SIGNATURES
    assert not set(abi_chanaudio.SIGNATURES) & set(abi.SIGNATURES)
    for name, side in list(abi.SIDE_HEADERS.items()) + list(abi.LATER_SIDE_HEADERS.items()):
        if name != "sdrhip_chanaudio.h":
            assert not set(abi_chanaudio.SIGNATURES) & set(side.SIGNATURES), name
    assert abi.LATER_SIDE_HEADERS["sdrhip_chanaudio.h"].header_functions() == sorted(NEW)
    assert (abi_chanaudio.CHAN_CS16, abi_chanaudio.CHAN_CF32) == (abi_channelizer.CHAN_CS16, abi_channelizer.CHAN_CF32)


def test_the_package_exports_the_class():
    import libsdr_amd
    from libsdr_amd import chanaudio
    assert libsdr_amd.AudioChannelizer is chanaudio.AudioChannelizer and issubclass(chanaudio.AudioChannelizer, nodes._Node)


def _create(dtype=0, M=8, D=4, taps=None, n_taps=None, max_in=1024, modes=None, gains=None, null=()):
    """(code, out) of sdrhip_chanaudio_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_chanaudio
    t = np.ascontiguousarray(np.linspace(0.1, 1.0, 24) if taps is None else taps, np.float64)
    m = None if modes is None else np.ascontiguousarray(modes, np.intc)
    g = None if gains is None else np.ascontiguousarray(gains, np.float32)
    h = C.c_void_p(0x1)
    code = abi_chanaudio.lib().sdrhip_chanaudio_create(None, dtype, M, D, None if "taps" in null else t.ctypes.data_as(dp),
                                                       t.size if n_taps is None else n_taps, max_in,
                                                       None if m is None else m.ctypes.data_as(ip), None if g is None else g.ctypes.data_as(fp),
                                                       None if "out" in null else C.byref(h))
    return code, h.value


def test_create_without_a_context():
    for code, h in (_create(), _create(dtype=1), _create(M=2, D=1), _create(M=2, D=2, taps=[1.0]), _create(M=4096, D=4096),
                    _create(M=1000, D=500), _create(M=13 * 11 * 7, D=3), _create(max_in=1), _create(max_in=(1 << 30) - 1),
                    _create(modes=[FM, AM, USB, FM, AM, USB, FM, AM]), _create(gains=np.linspace(-2, 1e30, 8)),
                    _create(modes=[AM] * 8, gains=[0.0] * 8), _create(M=2, D=1, modes=[USB, FM], gains=[1e-40, -3.5])):
        assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


def _bad_taps(v):
    t = np.linspace(0.1, 1.0, 24)
    t[13] = v
    return t


def _modes(k, v):
    m = [FM, AM, USB, FM, AM, USB, FM, AM]
    m[k] = v
    return m


def _gains(k, v):
    g = [1.0] * 8
    g[k] = v
    return g


RULES = [
    (dict(null=("taps",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(dtype=2), abi.E_INVALID, "dtype"), (dict(dtype=-1), abi.E_INVALID, "dtype"),
    (dict(M=1, D=1), abi.E_SIZE, "M 1"), (dict(M=0, D=1), abi.E_SIZE, "M 0"), (dict(M=4097), abi.E_SIZE, "M 4097"), (dict(M=8192), abi.E_SIZE, "M 8192"),
    (dict(M=17), abi.E_INVALID, "prime factor 17"), (dict(M=2 * 19), abi.E_INVALID, "prime factor 19"), (dict(M=4093), abi.E_INVALID, "prime factor"),
    (dict(D=0), abi.E_INVALID, "D 0"), (dict(D=9), abi.E_INVALID, "D 9"), (dict(D=-4), abi.E_INVALID, "D -4"),
    (dict(n_taps=0), abi.E_SIZE, "n_taps"), (dict(M=2, D=1, taps=np.ones(129)), abi.E_SIZE, "n_taps"), (dict(n_taps=-5), abi.E_SIZE, "n_taps"),
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(max_in=1 << 30), abi.E_SIZE, "max_in"),
    (dict(taps=_bad_taps(NAN)), abi.E_INVALID, "tap 13"), (dict(taps=_bad_taps(-INF)), abi.E_INVALID, "tap 13"),
    (dict(taps=_bad_taps(1e39)), abi.E_INVALID, "tap 13"),      # finite as a double, not as a float
    # the node's own: modes, then gains
    (dict(modes=_modes(5, NONE)), abi.E_UNSUPPORTED, "channel 5 is SDRHIP_EPI_NONE"), (dict(modes=_modes(0, NONE)), abi.E_UNSUPPORTED, "channel 0"),
    (dict(modes=_modes(7, 4)), abi.E_INVALID, "mode 4 of channel 7"), (dict(modes=_modes(2, -1)), abi.E_INVALID, "mode -1 of channel 2"),
    (dict(gains=_gains(3, NAN)), abi.E_INVALID, "gain of channel 3"), (dict(gains=_gains(0, INF)), abi.E_INVALID, "gain of channel 0"),
    (dict(gains=_gains(7, -INF)), abi.E_INVALID, "gain of channel 7"),
    # in the header's order
    (dict(null=("out",), dtype=2), abi.E_INVALID, "NULL"), (dict(dtype=2, M=1), abi.E_INVALID, "dtype"), (dict(M=1, D=0), abi.E_SIZE, "M 1"),
    (dict(M=17, D=0), abi.E_INVALID, "prime"), (dict(D=0, n_taps=0), abi.E_INVALID, "D 0"), (dict(n_taps=0, max_in=0), abi.E_SIZE, "n_taps"),
    (dict(max_in=0, taps=_bad_taps(NAN)), abi.E_SIZE, "max_in"), (dict(taps=_bad_taps(NAN), modes=_modes(1, NONE)), abi.E_INVALID, "tap 13"),
    (dict(modes=_modes(6, NONE), gains=_gains(0, NAN)), abi.E_UNSUPPORTED, "channel 6"), (dict(modes=_modes(6, 9), gains=_gains(0, NAN)), abi.E_INVALID, "mode 9"),
    (dict(modes=[FM, 9, NONE, FM, FM, FM, FM, FM]), abi.E_INVALID, "mode 9 of channel 1"),      # the first offending channel answers
]


@pytest.mark.parametrize("kw,want,text", RULES, ids=[str(i) for i in range(len(RULES))])
def test_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _create(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_chanaudio
    L = abi_chanaudio.lib()
    g, d, idx, t, sz, u = (C.c_float * 16)(), (C.c_double * 16)(), (C.c_int * 4)(0, 1, 2, 3), C.c_int(7), C.c_size_t(9), C.c_uint64(5)
    buf = C.create_string_buffer(64)
    for call in (lambda: L.sdrhip_chanaudio_process_dev(None, None, 0, None, 0, C.byref(sz)),
                 lambda: L.sdrhip_chanaudio_process(None, None, 0, None, 0, None),
                 lambda: L.sdrhip_chanaudio_set_channels(None, idx, 4), lambda: L.sdrhip_chanaudio_set_channels(None, None, 0),
                 lambda: L.sdrhip_chanaudio_set_mode(None, 0, FM), lambda: L.sdrhip_chanaudio_set_gain(None, 0, 1.0),
                 lambda: L.sdrhip_chanaudio_get_modes(None, idx, 4), lambda: L.sdrhip_chanaudio_get_gains(None, g, 16),
                 lambda: L.sdrhip_chanaudio_set_taps(None, d), lambda: L.sdrhip_chanaudio_reset(None),
                 lambda: L.sdrhip_chanaudio_get_state(None, C.byref(u), g, 8, idx, 4), lambda: L.sdrhip_chanaudio_kernel_names(None, buf, 64),
                 lambda: L.sdrhip_chanaudio_plan_info(None, C.byref(t), None, None, None, None, None)):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert sz.value == 0 and t.value == 7 and u.value == 5 and list(idx) == [0, 1, 2, 3]
    sz.value = 9
    assert L.sdrhip_chanaudio_out_count(None, 16, C.byref(sz)) == abi.E_INVALID and sz.value == 9
    assert L.sdrhip_chanaudio_destroy(None) == abi.OK


def test_the_two_kernels_exist_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(chanaudio_[a-z0-9]+_kernel)")
    assert seen == {"chanaudio_cs16_kernel": 0, "chanaudio_cf32_kernel": 0}, seen


# ---- the Python wrapper against a fake library -----------------------------------------------------------------------------------

def _plan_info(args):
    for a, v in zip(args[1:], (8, 3, 648, 5, 2, 31)):
        a._obj.value = v


def _get_state(args):
    args[1]._obj.value = 1234
    args[2]._arr[...] = 2.5
    args[4]._arr[...] = -77


def _get_modes(args):
    args[1]._arr[...] = USB


def _get_gains(args):
    args[1]._arr[...] = 0.25


def _run(monkeypatch):
    """The fake of test_nodes_calls.py, answering include/sdrhip_chanaudio.h's names as well (out_count(n) answers n // 4, the
    process calls report that); it records scalar arguments only, and no close hook."""
    from libsdr_amd import abi_chanaudio
    sigs = dict(abi.SIGNATURES, **abi_chanaudio.SIGNATURES)
    answers = {"sdrhip_chanaudio_plan_info": _plan_info, "sdrhip_chanaudio_get_state": _get_state, "sdrhip_chanaudio_get_modes": _get_modes,
               "sdrhip_chanaudio_get_gains": _get_gains}
    return Run(monkeypatch, FakeLib(signatures=sigs, answers=answers, scalars_only=True), hook=False)


def test_wrapper_calls_against_the_fake_library(monkeypatch):
    from libsdr_amd import abi_chanaudio, chanaudio
    r = _run(monkeypatch)
    ctx = r.ctx()
    x = ramp((16, 2), np.int16, 5)
    node = chanaudio.AudioChannelizer(ctx, np.int16, 8, 4, np.linspace(0.0, 1.0, 21), modes=[FM, AM] * 4, gains=np.arange(8), max_in=64)
    assert (node.dtype, node.M, node.D, node.n_taps, node.max_in, node.channels) == (0, 8, 4, 21, 64, 8) and node.selected == list(range(8))
    assert node.kernel_names == NAMES
    assert node.plan_info() == {"tile_times": 8, "branch_taps": 3, "lds_bytes": 648, "rows": 5, "fm_rows": 2, "halo_tiles": 31}
    assert node.out_count(16) == count(16)
    y = node.process(x)
    assert y.shape == (8, count(16)) and y.dtype == np.int16
    node.set_channels([5, 0, 2])
    assert node.selected == [5, 0, 2] and node.channels == 3
    r.route(True)
    routed = node.process(x)                       # through the router: process_dev with the router's output stride
    empty = node.process(x[:0])                    # an empty call never meets the router
    r.route(False)
    assert routed.shape == (3, count(16)) and empty.shape == (3, 0)
    assert node.process_dev(0x1000, 16, 0x2000, 7) == count(16)
    node.set_mode(2, USB)
    node.set_gain(1, 0.5)
    assert node.get_modes() == [USB] * 3 and node.get_gains().tolist() == [0.25] * 3
    node.set_taps(np.ones(21))
    with pytest.raises(AssertionError):
        node.set_taps(np.ones(20))
    s = node.get_state()
    assert s["consumed"] == 1234 and s["tail"].shape == (20, 2) and np.all(s["tail"] == 2.5) and s["last"].tolist() == [-77] * 3
    node.reset()
    node.set_channels(None)
    assert node.channels == 8
    with pytest.raises(AssertionError):
        chanaudio.AudioChannelizer(ctx, np.int16, 8, 4, np.ones(8), modes=[FM] * 7)
    with pytest.raises(AssertionError):
        chanaudio.AudioChannelizer(ctx, np.int16, 8, 4, np.ones(8), gains=[1.0] * 9)
    f = chanaudio.AudioChannelizer(ctx, np.float32, 12, 6, np.ones(30), channels=[11, 3], max_in=64)
    assert (f.dtype, f.channels, f._in) == (1, 2, (np.float32, 2))
    for o in (node, node, f, ctx):
        o.close()
    names = [c[0].replace("sdrhip_chanaudio_", "") for c in r.fake.calls]
    assert names == [
        "sdrhip_ctx_create", "create", "kernel_names", "plan_info", "out_count", "out_count", "process", "set_channels",
        "out_count", "router", "process_dev", "out_count", "process", "process_dev", "set_mode", "set_gain", "get_modes", "get_gains",
        "set_taps", "get_state", "reset", "set_channels", "create", "set_channels", "destroy", "destroy", "sdrhip_ctx_destroy"], names
    calls = {}
    for c in r.fake.calls:
        calls.setdefault(c[0].replace("sdrhip_chanaudio_", ""), []).append(c[1:])
    assert calls["create"][0][1:4] == (0, 8, 4) and calls["create"][0][5:7] == (21, 64)
    assert calls["create"][1][1:4] == (1, 12, 6) and calls["create"][1][5:9] == (30, 64, None, None)      # no modes, no gains: NULL
    assert calls["process"][0][2] == 16 and calls["process"][0][4] == count(16)
    assert calls["process_dev"][0][2] == 16 and calls["process_dev"][0][4] == count(16) + 3   # the router's stride
    assert calls["process"][1][2] == 0
    assert calls["process_dev"][1][2] == 16 and calls["process_dev"][1][4] == 7
    assert [c[2] for c in calls["set_channels"]] == [3, 0, 2]
    assert calls["set_mode"] == [(None, 2, USB)] and calls["set_gain"] == [(None, 1, 0.5)]
    assert calls["get_modes"][0][-1] == 3 and calls["get_gains"][0][-1] == 3
    assert calls["get_state"][0][3] == 20 and calls["get_state"][0][5] == 3
    assert set(abi_chanaudio.SIGNATURES) <= r.fake.reached, sorted(set(abi_chanaudio.SIGNATURES) - r.fake.reached)


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    from libsdr_amd import chanaudio
    r = _run(monkeypatch)
    ctx = r.ctx()
    monkeypatch.setattr(chanaudio.AudioChannelizer, "_calls", chanaudio.AudioChannelizer._calls + " get_mdoes")
    with pytest.raises(AttributeError, match="sdrhip_chanaudio_get_mdoes"):
        chanaudio.AudioChannelizer(ctx, np.int16, 8, 4, np.ones(8))
