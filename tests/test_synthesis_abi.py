"""The synthesis bank's C calls (include/sdrhip_synthesis.h), what can be checked without a GPU: every function of the header is
exported by libsdrhip.so and has a prototype in libsdr_amd/abi_synthesis.py, and nothing else of the family is exported; the
header is registered in abi.LATER_SIDE_HEADERS and not in abi.SIDE_HEADERS; every argument rule of create answers BEFORE the
context is looked at, in the header's order; the calls on a handle refuse a NULL one; the two kernels exist for gfx950 and use no
scratch; and the Python wrapper, driven against the fake library of tests/test_nodes_calls.py, makes the calls it should."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes
from test_nodes_calls import FakeLib, NAMES, Run, count, ramp

NEW = ["sdrhip_synthesis_create", "sdrhip_synthesis_destroy", "sdrhip_synthesis_get_state", "sdrhip_synthesis_kernel_names",
       "sdrhip_synthesis_out_count", "sdrhip_synthesis_plan_info", "sdrhip_synthesis_process", "sdrhip_synthesis_process_dev",
       "sdrhip_synthesis_reset", "sdrhip_synthesis_set_channels", "sdrhip_synthesis_set_taps"]
dp = C.POINTER(C.c_double)
INF, NAN = float("inf"), float("nan")


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_synthesis
    assert_header_binding(abi_synthesis, NEW, r"\b(sdrhip_synthesis[a-z0-9_]*)\b")


def test_the_header_is_in_the_second_table_only():
    import libsdr_amd  # noqa: F401   (the package imports every side header's module)
    from libsdr_amd import abi_synthesis
    assert "sdrhip_synthesis.h" in abi.LATER_SIDE_HEADERS and "sdrhip_synthesis.h" not in abi.SIDE_HEADERS
    assert abi.LATER_SIDE_HEADERS["sdrhip_synthesis.h"].SIGNATURES is abi_synthesis.SIGNATURES
    assert not set(abi_synthesis.SIGNATURES) & set(abi.SIGNATURES)
    for name, side in list(abi.SIDE_HEADERS.items()) + list(abi.LATER_SIDE_HEADERS.items()):
        if name != "sdrhip_synthesis.h":
            assert not set(abi_synthesis.SIGNATURES) & set(side.SIGNATURES), name
    assert sorted(abi.lib()._declared) == abi.header_functions()
    assert abi.LATER_SIDE_HEADERS["sdrhip_synthesis.h"].header_functions() == sorted(NEW)


def test_the_package_exports_the_class():
    import libsdr_amd
    from libsdr_amd import synthesis
    assert libsdr_amd.Synthesis is synthesis.Synthesis and issubclass(synthesis.Synthesis, nodes._Node)


def _create(M=8, D=4, taps=None, n_taps=None, max_in=1024, null=()):
    """(code, out) of sdrhip_synthesis_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_synthesis
    t = np.ascontiguousarray(np.linspace(0.1, 1.0, 24) if taps is None else taps, np.float64)
    h = C.c_void_p(0x1)
    code = abi_synthesis.lib().sdrhip_synthesis_create(None, M, D, None if "taps" in null else t.ctypes.data_as(dp),
                                                       t.size if n_taps is None else n_taps, max_in, None if "out" in null else C.byref(h))
    return code, h.value


def test_create_without_a_context():
    for code, h in (_create(), _create(M=2, D=1), _create(M=2, D=2, taps=[1.0]), _create(M=4096, D=4096, max_in=64),
                    _create(M=4096, D=1, taps=np.ones(64), max_in=(1 << 16) - 63), _create(M=1000, D=500), _create(M=13 * 11 * 7, D=3),
                    _create(M=8, D=8, taps=np.ones(512)), _create(max_in=1), _create(M=2, D=1, taps=[1.0], max_in=(1 << 27)),
                    _create(M=8, D=8, taps=[1.0], max_in=1 << 25), _create(taps=[1e-60, 1.0])):
        assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


def _bad_taps(v):
    t = np.linspace(0.1, 1.0, 24)
    t[13] = v
    return t


RULES = [
    (dict(null=("taps",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(M=1, D=1), abi.E_SIZE, "M 1"), (dict(M=0, D=1), abi.E_SIZE, "M 0"), (dict(M=4097), abi.E_SIZE, "M 4097"), (dict(M=8192), abi.E_SIZE, "M 8192"),
    (dict(M=17), abi.E_INVALID, "prime factor 17"), (dict(M=2 * 19), abi.E_INVALID, "prime factor 19"), (dict(M=4093), abi.E_INVALID, "prime factor"),
    (dict(D=0), abi.E_INVALID, "D 0"), (dict(D=9), abi.E_INVALID, "D 9"), (dict(D=-4), abi.E_INVALID, "D -4"),
    (dict(n_taps=0), abi.E_SIZE, "n_taps"), (dict(M=8, D=2, taps=np.ones(129)), abi.E_SIZE, "n_taps"), (dict(n_taps=-5), abi.E_SIZE, "n_taps"),
    (dict(D=1, taps=np.ones(65)), abi.E_SIZE, "n_taps"),            # (64 M admits it: the bound is 64 D)
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(max_in=1 << 30), abi.E_SIZE, "max_in"),
    (dict(M=8, D=8, max_in=1 << 27), abi.E_SIZE, "2^30"),           # max_in D = 2^30
    (dict(M=4096, D=1, taps=[1.0], max_in=(1 << 16) + 1), abi.E_SIZE, "2^28"),   # the workspace: max_in M above 2^28
    (dict(M=4096, D=1, taps=np.ones(64), max_in=(1 << 16) - 62), abi.E_SIZE, "2^28"),   # (Q - 1 + max_in) M = 2^28 + M
    (dict(taps=_bad_taps(NAN)), abi.E_INVALID, "tap 13"), (dict(taps=_bad_taps(-INF)), abi.E_INVALID, "tap 13"),
    (dict(taps=_bad_taps(1e39)), abi.E_INVALID, "tap 13"),      # finite as a double, not as a float
    # in the header's order
    (dict(null=("out",), M=1), abi.E_INVALID, "NULL"), (dict(M=1, D=0), abi.E_SIZE, "M 1"),
    (dict(M=17, D=0), abi.E_INVALID, "prime"), (dict(D=0, n_taps=0), abi.E_INVALID, "D 0"), (dict(n_taps=0, max_in=0), abi.E_SIZE, "n_taps"),
    (dict(max_in=0, taps=_bad_taps(NAN)), abi.E_SIZE, "max_in"),
    (dict(M=8, D=8, max_in=1 << 27, taps=_bad_taps(NAN)), abi.E_SIZE, "2^30"),
    (dict(M=4096, D=1, max_in=1 << 17, taps=_bad_taps(NAN)), abi.E_SIZE, "2^28"),
    (dict(M=4096, D=4096, max_in=1 << 18), abi.E_SIZE, "2^30"),     # both size rules broken: the outputs' comes first
]


@pytest.mark.parametrize("kw,want,text", RULES, ids=[str(i) for i in range(len(RULES))])
def test_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _create(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_synthesis
    L = abi_synthesis.lib()
    g, d, idx, t, sz, u = (C.c_float * 16)(), (C.c_double * 16)(), (C.c_int * 4)(0, 1, 2, 3), C.c_int(7), C.c_size_t(9), C.c_uint64(5)
    buf = C.create_string_buffer(64)
    for call in (lambda: L.sdrhip_synthesis_process_dev(None, None, 0, 0, None, C.byref(sz)),
                 lambda: L.sdrhip_synthesis_process(None, None, 0, 0, None, None),
                 lambda: L.sdrhip_synthesis_set_channels(None, idx, 4), lambda: L.sdrhip_synthesis_set_channels(None, None, 0),
                 lambda: L.sdrhip_synthesis_set_taps(None, d), lambda: L.sdrhip_synthesis_reset(None),
                 lambda: L.sdrhip_synthesis_get_state(None, C.byref(u), g, 8), lambda: L.sdrhip_synthesis_kernel_names(None, buf, 64),
                 lambda: L.sdrhip_synthesis_plan_info(None, C.byref(t), None, None, None)):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert sz.value == 0 and t.value == 7 and u.value == 5
    sz.value = 9
    assert L.sdrhip_synthesis_out_count(None, 16, C.byref(sz)) == abi.E_INVALID and sz.value == 9
    assert L.sdrhip_synthesis_destroy(None) == abi.OK


def test_the_two_kernels_exist_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(synthesis_[a-z0-9]+_kernel)")
    assert seen == {"synthesis_transform_kernel": 0, "synthesis_overlap_kernel": 0}, seen


# ---- the Python wrapper against a fake library -----------------------------------------------------------------------------------

def _plan_info(args):
    for a, v in zip(args[1:], (8, 3, 288, 5)):
        a._obj.value = v


def _get_state(args):
    args[1]._obj.value = 1234
    args[2]._arr[...] = 2.5


def _run(monkeypatch):
    """The fake of test_nodes_calls.py, answering include/sdrhip_synthesis.h's names as well (out_count(n) answers n // 4, the
    process calls report that); it records scalar arguments only, and no close hook."""
    from libsdr_amd import abi_synthesis
    sigs = dict(abi.SIGNATURES, **abi_synthesis.SIGNATURES)
    answers = {"sdrhip_synthesis_plan_info": _plan_info, "sdrhip_synthesis_get_state": _get_state}
    return Run(monkeypatch, FakeLib(signatures=sigs, answers=answers, scalars_only=True), hook=False)


def test_wrapper_calls_against_the_fake_library(monkeypatch):
    from libsdr_amd import abi_synthesis, synthesis
    r = _run(monkeypatch)
    ctx = r.ctx()
    x = ramp((8, 16, 2), np.float32, 5)
    node = synthesis.Synthesis(ctx, 8, 4, np.linspace(0.0, 1.0, 21), max_in=64)
    assert (node.M, node.D, node.n_taps, node.Q, node.max_in, node.channels) == (8, 4, 21, 6, 64, 8) and node.selected == list(range(8))
    assert node.kernel_names == NAMES and node.plan_info() == {"tile_times": 8, "branch_taps": 3, "lds_bytes": 288, "rows": 5}
    assert node.out_count(16) == count(16)
    y = node.process(x)
    assert y.shape == (count(16), 2) and y.dtype == np.float32
    with pytest.raises(AssertionError):
        node.process(x[:3])                        # the rows are the selection's
    node.set_channels([5, 0, 2])
    assert node.selected == [5, 0, 2] and node.channels == 3
    r.route(True)
    routed = node.process(x[:3])                   # through the router: process_dev with the router's input stride
    empty = node.process(x[:3, :0])                # an empty call never meets the router
    r.route(False)
    assert routed.shape == (count(16), 2) and empty.shape == (0, 2)
    assert node.process_dev(0x1000, 16, 23, 0x2000) == count(16)
    node.set_taps(np.ones(21))
    with pytest.raises(AssertionError):
        node.set_taps(np.ones(20))
    s = node.get_state()
    assert s["consumed"] == 1234 and s["cols"].shape == (5, 8, 2) and np.all(s["cols"] == 2.5)
    node.reset()
    node.set_channels(None)
    assert node.channels == 8
    f = synthesis.Synthesis(ctx, 12, 6, np.ones(30), channels=[11, 3], max_in=64)
    assert (f.channels, f.Q, f._in) == (2, 5, (np.float32, 2))
    for o in (node, node, f, ctx):
        o.close()
    names = [c[0] for c in r.fake.calls]
    assert names == [
        "sdrhip_ctx_create", "sdrhip_synthesis_create", "sdrhip_synthesis_kernel_names", "sdrhip_synthesis_plan_info",
        "sdrhip_synthesis_out_count", "sdrhip_synthesis_out_count", "sdrhip_synthesis_process", "sdrhip_synthesis_set_channels",
        "sdrhip_synthesis_out_count", "router", "sdrhip_synthesis_process_dev",
        "sdrhip_synthesis_out_count", "sdrhip_synthesis_process",
        "sdrhip_synthesis_process_dev", "sdrhip_synthesis_set_taps", "sdrhip_synthesis_get_state", "sdrhip_synthesis_reset",
        "sdrhip_synthesis_set_channels", "sdrhip_synthesis_create", "sdrhip_synthesis_set_channels",
        "sdrhip_synthesis_destroy", "sdrhip_synthesis_destroy", "sdrhip_ctx_destroy"], names
    calls = {}
    for c in r.fake.calls:
        calls.setdefault(c[0], []).append(c[1:])
    assert calls["sdrhip_synthesis_create"][0][1:3] == (8, 4) and calls["sdrhip_synthesis_create"][0][4:6] == (21, 64)
    assert calls["sdrhip_synthesis_create"][1][1:3] == (12, 6) and calls["sdrhip_synthesis_create"][1][4:6] == (30, 64)
    assert calls["sdrhip_synthesis_process"][0][2:4] == (16, 16)
    assert calls["sdrhip_synthesis_process_dev"][0][2:4] == (16, 16 + 3)      # the router's stride
    assert calls["sdrhip_synthesis_process"][1][2] == 0
    assert calls["sdrhip_synthesis_process_dev"][1][2:4] == (16, 23)
    assert [c[2] for c in calls["sdrhip_synthesis_set_channels"]] == [3, 0, 2]
    assert calls["sdrhip_synthesis_get_state"][0][-1] == 5 * 8
    assert set(abi_synthesis.SIGNATURES) <= r.fake.reached, sorted(set(abi_synthesis.SIGNATURES) - r.fake.reached)


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    from libsdr_amd import synthesis
    r = _run(monkeypatch)
    ctx = r.ctx()
    monkeypatch.setattr(synthesis.Synthesis, "_calls", synthesis.Synthesis._calls + " get_sttae")
    with pytest.raises(AttributeError, match="sdrhip_synthesis_get_sttae"):
        synthesis.Synthesis(ctx, 8, 4, np.ones(8))
