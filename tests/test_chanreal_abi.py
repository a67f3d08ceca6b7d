"""The real-input create calls of the channelizer family (include/sdrhip_chanreal.h), what can be checked without a GPU: the
header's three functions are exported by libsdrhip.so and have prototypes in libsdr_amd/abi_chanreal.py, and nothing else named
sdrhip_chanreal is exported; the header is registered in abi.LATER_SIDE_HEADERS and not in abi.SIDE_HEADERS, and its names are
disjoint from every other header's; every argument rule of the three create calls answers BEFORE the context is looked at, in the
header's order, with its code and message; the six kernels exist for gfx950 and use no scratch; and the Python wrappers under
real=True, driven against the fake library of tests/test_nodes_calls.py, have the attributes and make the calls they should."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes
from test_nodes_calls import FakeLib, Run, count, ramp

NEW = ["sdrhip_chanreal_audio_create", "sdrhip_chanreal_channelizer_create", "sdrhip_chanreal_power_create"]
dp, ip, fp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float)
INF, NAN = float("inf"), float("nan")
NODES = ["channelizer", "audio", "power"]


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_chanreal
    assert_header_binding(abi_chanreal, NEW, r"\b(sdrhip_chanreal[a-z0-9_]*)\b")
    assert (abi_chanreal.CHANREAL_S16, abi_chanreal.CHANREAL_F32) == (0, 1)
    text = open(abi_chanreal.HEADER).read()
    assert "enum { SDRHIP_CHANREAL_S16 = 0, SDRHIP_CHANREAL_F32 = 1 }" in text
    for inc in ("sdrhip_channelizer.h", "sdrhip_chanaudio.h", "sdrhip_chanpower.h"):
        assert '#include "%s"' % inc in text


def test_the_header_is_in_the_second_table_only():
    import libsdr_amd  # noqa: F401   (the package imports every side header's module)
    from libsdr_amd import abi_chanreal
    assert "sdrhip_chanreal.h" in abi.LATER_SIDE_HEADERS and "sdrhip_chanreal.h" not in abi.SIDE_HEADERS
    assert abi.LATER_SIDE_HEADERS["sdrhip_chanreal.h"].SIGNATURES is abi_chanreal.SIGNATURES
    assert not set(abi_chanreal.SIGNATURES) & set(abi.SIGNATURES)
    for name, side in list(abi.SIDE_HEADERS.items()) + list(abi.LATER_SIDE_HEADERS.items()):
        if name != "sdrhip_chanreal.h":
            assert not set(abi_chanreal.SIGNATURES) & set(side.SIGNATURES), name
            assert not set(NEW) & set(side.header_functions()), name
    assert abi.LATER_SIDE_HEADERS["sdrhip_chanreal.h"].header_functions() == sorted(NEW)


def _create(node="channelizer", dtype=0, M=8, D=4, taps=None, n_taps=None, max_in=1024, null=(), modes=None, gains=None, alpha=0.25):
    """(code, out) of the node's real create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_chanreal
    t = np.ascontiguousarray(np.linspace(0.1, 1.0, 24) if taps is None else taps, np.float64)
    h = C.c_void_p(0x1)
    head = (None, dtype, M, D, None if "taps" in null else t.ctypes.data_as(dp), t.size if n_taps is None else n_taps, max_in)
    out = None if "out" in null else C.byref(h)
    L = abi_chanreal.lib()
    if node == "channelizer":
        code = L.sdrhip_chanreal_channelizer_create(*head, out)
    elif node == "audio":
        m = None if modes is None else np.ascontiguousarray(modes, np.intc)
        g = None if gains is None else np.ascontiguousarray(gains, np.float32)
        code = L.sdrhip_chanreal_audio_create(*head, None if m is None else m.ctypes.data_as(ip), None if g is None else g.ctypes.data_as(fp), out)
    else:
        code = L.sdrhip_chanreal_power_create(*head, alpha, out)
    return code, h.value


@pytest.mark.parametrize("node", NODES)
def test_create_without_a_context(node):
    for kw in (dict(), dict(dtype=1), dict(M=4, D=1), dict(M=4, D=4, taps=[1.0]), dict(M=4096, D=4096), dict(M=4096, D=1, taps=np.ones(64 * 4096)),
               dict(M=1000, D=500), dict(M=2 * 13 * 11 * 7, D=3), dict(M=26, D=13), dict(M=8, taps=np.ones(512)), dict(max_in=1),
               dict(max_in=(1 << 30) - 1)):
        code, h = _create(node, **kw)
        assert code == no_ctx_code() and h is None, kw
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


def _bad_taps(v):
    t = np.linspace(0.1, 1.0, 24)
    t[13] = v
    return t


RULES = [
    (dict(null=("taps",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(dtype=2), abi.E_INVALID, "dtype"), (dict(dtype=-1), abi.E_INVALID, "dtype"),
    (dict(M=2, D=1), abi.E_SIZE, "M 2 outside [4,4096]"), (dict(M=3, D=1), abi.E_SIZE, "M 3"), (dict(M=0, D=1), abi.E_SIZE, "M 0"),
    (dict(M=4098), abi.E_SIZE, "M 4098"), (dict(M=4097), abi.E_SIZE, "M 4097"),
    (dict(M=5), abi.E_INVALID, "M 5 is odd"), (dict(M=4095), abi.E_INVALID, "odd"),
    (dict(M=17 * 2), abi.E_INVALID, "M / 2 = 17 has the prime factor 17"), (dict(M=4 * 19), abi.E_INVALID, "prime factor 19"),
    (dict(D=0), abi.E_INVALID, "D 0"), (dict(D=9), abi.E_INVALID, "D 9"),
    (dict(n_taps=0), abi.E_SIZE, "n_taps"), (dict(M=4, D=1, taps=np.ones(257)), abi.E_SIZE, "n_taps"),
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(max_in=1 << 30), abi.E_SIZE, "max_in"),
    (dict(taps=_bad_taps(NAN)), abi.E_INVALID, "tap 13"), (dict(taps=_bad_taps(1e39)), abi.E_INVALID, "tap 13"),
    # in the header's order
    (dict(null=("out",), dtype=2), abi.E_INVALID, "NULL"), (dict(dtype=2, M=2), abi.E_INVALID, "dtype"), (dict(M=2, D=0), abi.E_SIZE, "M 2"),
    (dict(M=5, D=0), abi.E_INVALID, "odd"), (dict(M=34, D=0), abi.E_INVALID, "prime"), (dict(D=0, n_taps=0), abi.E_INVALID, "D 0"),
    (dict(n_taps=0, max_in=0), abi.E_SIZE, "n_taps"), (dict(max_in=0, taps=_bad_taps(NAN)), abi.E_SIZE, "max_in"),
]


@pytest.mark.parametrize("node", NODES)
@pytest.mark.parametrize("kw,want,text", RULES, ids=[str(i) for i in range(len(RULES))])
def test_create_argument_rules_come_before_the_context(node, kw, want, text):
    code, h = _create(node, **kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_the_nodes_own_arguments_have_k_entries():
    # M = 8: K = 5 modes and gains are read, no more (the sixth entry is bad and is not looked at)
    good = [abi.EPI_FM, abi.EPI_AM, abi.EPI_USB, abi.EPI_FM, abi.EPI_AM]
    assert _create("audio", modes=good + [77])[0] == no_ctx_code()
    assert _create("audio", gains=[1.0] * 5 + [NAN])[0] == no_ctx_code()
    code, _ = _create("audio", modes=good[:4] + [77])
    assert code == abi.E_INVALID and "channel 4" in last_error()
    code, _ = _create("audio", modes=good[:4] + [abi.EPI_NONE])
    assert code == abi.E_UNSUPPORTED and "channel 4" in last_error()
    code, _ = _create("audio", gains=[1.0] * 4 + [INF])
    assert code == abi.E_INVALID and "channel 4" in last_error()
    # behind the shared rules, before the context
    code, _ = _create("audio", max_in=0, modes=good[:4] + [77])
    assert code == abi.E_SIZE and "max_in" in last_error()
    for alpha in (0.0, 1.5, NAN):
        code, _ = _create("power", alpha=alpha)
        assert code == abi.E_INVALID and "alpha" in last_error()
    code, _ = _create("power", max_in=0, alpha=0.0)
    assert code == abi.E_SIZE and "max_in" in last_error()


def test_the_six_kernels_exist_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(chan[a-z]+_real_[a-z0-9]+_kernel)")
    want = ["%s_real_%s_kernel" % (f, t) for f in ("channelizer", "chanaudio", "chanpower") for t in ("s16", "f32")]
    assert seen == {k: 0 for k in want}, seen


# ---- the Python wrappers against a fake library ----------------------------------------------------------------------------------

def _get_state(args):
    args[1]._obj.value = 1234
    args[2]._arr[...] = 2.5


def _run(monkeypatch):
    from libsdr_amd import abi_channelizer, abi_chanaudio, abi_chanpower, abi_chanreal
    sigs = dict(abi.SIGNATURES)
    for m in (abi_channelizer, abi_chanaudio, abi_chanpower, abi_chanreal):
        sigs.update(m.SIGNATURES)
    answers = {"sdrhip_%s_get_state" % n: _get_state for n in ("channelizer", "chanaudio", "chanpower")}
    return Run(monkeypatch, FakeLib(signatures=sigs, answers=answers, scalars_only=True), hook=False)


def test_wrappers_under_real(monkeypatch):
    import libsdr_amd as sa
    r = _run(monkeypatch)
    ctx = r.ctx()
    x = ramp((16,), np.int16, 5)
    node = sa.Channelizer(ctx, np.int16, 8, 4, np.linspace(0.0, 1.0, 21), max_in=64, real=True)
    assert (node.real, node.dtype, node.M, node.D, node.n_taps, node.channels, node.n_channels) == (True, 0, 8, 4, 21, 5, 5)
    assert node.selected == [0, 1, 2, 3, 4] and node._in == (np.int16, 0)
    y = node.process(x)
    assert y.shape == (5, count(16), 2) and y.dtype == np.float32
    with pytest.raises(AssertionError):
        node.process(ramp((16, 2), np.int16, 5))          # a complex row
    node.set_channels([4, 0])
    assert node.selected == [4, 0] and node.channels == 2
    node.set_channels(None)
    assert node.selected == [0, 1, 2, 3, 4]
    s = node.get_state()
    assert s["consumed"] == 1234 and s["tail"].shape == (20, 2)
    f = sa.Channelizer(ctx, np.float32, 12, 5, np.ones(30), channels=[6, 0], max_in=64, real=True)
    assert (f.dtype, f.channels, f.n_channels, f._in) == (1, 2, 7, (np.float32, 0))
    audio = sa.AudioChannelizer(ctx, np.int16, 8, 4, np.ones(21), modes=[abi.EPI_FM] * 5, gains=np.ones(5), max_in=64, real=True)
    assert (audio.real, audio.channels, audio.n_channels) == (True, 5, 5)
    assert audio.process(x).shape == (5, count(16)) and audio.get_state()["last"].shape == (5,)
    for bad in (dict(modes=[abi.EPI_FM] * 8), dict(gains=np.ones(8))):
        with pytest.raises(AssertionError):
            sa.AudioChannelizer(ctx, np.int16, 8, 4, np.ones(21), max_in=64, real=True, **bad)
    power = sa.ChannelPower(ctx, np.float32, 8, 4, np.ones(21), alpha=0.5, max_in=64, real=True)
    assert (power.real, power.n_channels, power._in) == (True, 5, (np.float32, 0))
    assert power.process(ramp((16,), np.float32, 2)).shape == (5,)
    power.set_thresholds(2.0, 1.0)
    level, flags = power.levels()
    assert level.shape == flags.shape == (5,)
    power.occupied()
    # real=False: what the wrappers send is what they sent before
    c = sa.Channelizer(ctx, np.int16, 8, 4, np.ones(21), max_in=64)
    assert (c.real, c.channels, c.n_channels, c._in) == (False, 8, 8, (np.int16, 2))
    for o in (node, f, audio, power, c, ctx):
        o.close()
    calls = {}
    for call in r.fake.calls:
        calls.setdefault(call[0], []).append(call[1:])
    assert [v[1:4] for v in calls["sdrhip_chanreal_channelizer_create"]] == [(0, 8, 4), (1, 12, 5)]
    assert calls["sdrhip_chanreal_channelizer_create"][0][5:7] == (21, 64)
    assert len(calls["sdrhip_chanreal_audio_create"]) == 1 and len(calls["sdrhip_chanreal_power_create"]) == 1
    assert calls["sdrhip_chanreal_power_create"][0][7] == 0.5
    assert len(calls["sdrhip_channelizer_create"]) == 1 and "sdrhip_chanaudio_create" not in calls and "sdrhip_chanpower_create" not in calls
    assert [v[2] for v in calls["sdrhip_channelizer_set_channels"]] == [2, 0, 2]
    assert calls["sdrhip_chanpower_get_levels"][0][-1] == 5 and calls["sdrhip_chanpower_get_occupied"][0][2] == 5
    assert calls["sdrhip_channelizer_process"][0][2] == 16
