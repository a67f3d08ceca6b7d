"""The interpolating resampler bank's C calls (include/sdrhip_resample.h), what can be checked without a GPU: every function of
the header is exported by libsdrhip.so and has a prototype in libsdr_amd/abi_resample.py, and nothing else of the family is
exported; the header is registered in abi.LATER_SIDE_HEADERS and not in abi.SIDE_HEADERS; every argument rule of the two create
calls answers BEFORE the context is looked at, in the header's order; the calls on a handle refuse a NULL one; the capacity
formula of the restatement is the header's; the four kernels exist for gfx950 and use no scratch; and the Python wrappers, driven
against the fake library of tests/test_nodes_calls.py, make the calls they should."""
import ctypes as C

import numpy as np
import pytest

import resample_restatement as R
from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes
from test_nodes_calls import FakeLib, NAMES, Run, ramp

NEW = ["sdrhip_resample_create", "sdrhip_resample_destroy", "sdrhip_resample_get_state", "sdrhip_resample_kernel_names",
       "sdrhip_resample_out_capacity", "sdrhip_resample_plan_info", "sdrhip_resample_process", "sdrhip_resample_process_dev",
       "sdrhip_resample_reset", "sdrhip_resample_set_channel", "sdrhip_resamplebank_create"]
fp = C.POINTER(C.c_float)
INF, NAN = float("inf"), float("nan")


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_resample
    assert_header_binding(abi_resample, NEW, r"\b(sdrhip_resample[a-z0-9_]*)\b")


def test_the_header_is_in_the_second_table_only():
    import libsdr_amd  # noqa: F401   (the package imports every side header's module)
    from libsdr_amd import abi_resample
    assert "sdrhip_resample.h" in abi.LATER_SIDE_HEADERS and "sdrhip_resample.h" not in abi.SIDE_HEADERS
    assert abi.LATER_SIDE_HEADERS["sdrhip_resample.h"].SIGNATURES is abi_resample.SIGNATURES
    assert not set(abi_resample.SIGNATURES) & set(abi.SIGNATURES)           # abi.SIGNATURES stays the binding of sdrhip.h alone
    assert sorted(abi.lib()._declared) == abi.header_functions()
    for side in abi.SIDE_HEADERS.values():
        assert not set(abi_resample.SIGNATURES) & set(side.SIGNATURES)
    # bind_header enters a binding in the table it is given, and in SIDE_HEADERS when it is given none
    table, before = {}, sorted(abi.SIDE_HEADERS)
    b = abi.bind_header("sdrhip_resample.h", abi_resample.SIGNATURES, registry=table)
    assert list(table) == ["sdrhip_resample.h"] and table["sdrhip_resample.h"] is b and sorted(abi.SIDE_HEADERS) == before
    assert b.header_functions() == sorted(NEW) and b.lib() is abi.lib()


def test_the_package_exports_this_modules_classes():
    import libsdr_amd
    from libsdr_amd import resample
    assert libsdr_amd.InpolSubSampler is resample.InpolSubSampler and libsdr_amd.InpolSubSamplerBank is resample.InpolSubSamplerBank
    assert issubclass(resample.InpolSubSampler, resample.InpolSubSamplerBank) and issubclass(resample.InpolSubSamplerBank, nodes._Node)
    assert issubclass(resample.InpolSubSamplerBank, nodes._TilePlan)


def _bank(dtype=0, frac=(0.5, 1.0, 7.9), table=None, channels=None, max_in=1024, null=()):
    """(code, out) of sdrhip_resamplebank_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_resample
    frac = np.ascontiguousarray(frac, np.float32)
    t = np.ascontiguousarray(R.table() if table is None else table, np.float32)
    h = C.c_void_p(0x1)
    code = abi_resample.lib().sdrhip_resamplebank_create(None, dtype, None if "frac" in null else frac.ctypes.data_as(fp),
                                                         None if "table" in null else t.ctypes.data_as(fp),
                                                         frac.size if channels is None else channels, max_in, None if "out" in null else C.byref(h))
    return code, h.value


def _one(dtype=0, frac=1.378125, table=None, channels=3, max_in=1024, null=()):
    from libsdr_amd import abi_resample
    t = np.ascontiguousarray(R.table() if table is None else table, np.float32)
    h = C.c_void_p(0x1)
    code = abi_resample.lib().sdrhip_resample_create(None, dtype, frac, None if "table" in null else t.ctypes.data_as(fp), channels, max_in,
                                                     None if "out" in null else C.byref(h))
    return code, h.value


def test_create_without_a_context():
    for code, h in (_bank(), _one(), _bank(dtype=1), _one(dtype=1), _one(dtype=2), _bank(dtype=3), _one(frac=0.125), _one(frac=4096.0),
                    _one(frac=1.0), _one(channels=1), _one(channels=65535), _one(max_in=1), _one(max_in=(1 << 30) - 1)):
        assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


def _bad_table(v):
    t = R.table().copy()
    t[77, 3] = v
    return t


RULES = [
    (dict(null=("table",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(dtype=4), abi.E_INVALID, "dtype"), (dict(dtype=-1), abi.E_INVALID, "dtype"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=65536), abi.E_INVALID, "channels"),
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(max_in=1 << 30), abi.E_SIZE, "max_in"),
    (dict(table=_bad_table(NAN)), abi.E_INVALID, "table"), (dict(table=_bad_table(-INF)), abi.E_INVALID, "table"),
    # in the header's order
    (dict(null=("out",), dtype=4), abi.E_INVALID, "NULL"), (dict(dtype=4, channels=0), abi.E_INVALID, "dtype"),
    (dict(channels=0, max_in=0), abi.E_INVALID, "channels"), (dict(max_in=0, table=_bad_table(NAN)), abi.E_SIZE, "max_in"),
]
BANK_RULES = RULES + [
    (dict(null=("frac",)), abi.E_INVALID, "NULL"),
    (dict(frac=(0.5, 0.1249, 2.0)), abi.E_INVALID, "frac"), (dict(frac=(0.5, 2.0, 4096.5)), abi.E_INVALID, "frac"),
    (dict(frac=(NAN, 2.0, 2.0)), abi.E_INVALID, "frac"), (dict(frac=(2.0, INF, 2.0)), abi.E_INVALID, "frac"),
    (dict(frac=(2.0, 0.0, 2.0)), abi.E_INVALID, "frac"), (dict(frac=(2.0, 2.0, -2.0)), abi.E_INVALID, "frac"),
    (dict(max_in=0, frac=(0.0, 2.0, 2.0)), abi.E_SIZE, "max_in"), (dict(frac=(0.0, 2.0, 2.0), table=_bad_table(NAN)), abi.E_INVALID, "frac"),
]
ONE_RULES = RULES + [
    (dict(frac=0.0), abi.E_INVALID, "frac"), (dict(frac=-1.5), abi.E_INVALID, "frac"), (dict(frac=NAN), abi.E_INVALID, "frac"),
    (dict(frac=INF), abi.E_INVALID, "frac"), (dict(frac=0.12), abi.E_INVALID, "frac"), (dict(frac=5000.0), abi.E_INVALID, "frac"),
    (dict(max_in=0, frac=0.0), abi.E_SIZE, "max_in"), (dict(frac=0.0, table=_bad_table(INF)), abi.E_INVALID, "frac"),
]


@pytest.mark.parametrize("kw,want,text", BANK_RULES, ids=[str(i) for i in range(len(BANK_RULES))])
def test_bank_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _bank(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


@pytest.mark.parametrize("kw,want,text", ONE_RULES, ids=[str(i) for i in range(len(ONE_RULES))])
def test_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _one(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_resample
    L = abi_resample.lib()
    g, e, t, sz = (C.c_float * 16)(), (C.c_int16 * 16)(), C.c_int(7), C.c_size_t(9)
    buf = C.create_string_buffer(64)
    assert L.sdrhip_resample_process_dev(None, None, 0, 0, None, 0, None) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_resample_process(None, None, 0, 0, None, 0, None) == abi.E_INVALID and "NULL" in last_error()
    for call in (lambda: L.sdrhip_resample_set_channel(None, 0, 2.0), lambda: L.sdrhip_resample_get_state(None, g, g, g, e, 1),
                 lambda: L.sdrhip_resample_reset(None), lambda: L.sdrhip_resample_kernel_names(None, buf, 64),
                 lambda: L.sdrhip_resample_out_capacity(None, 16, C.byref(sz))):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert sz.value == 9
    assert L.sdrhip_resample_plan_info(None, 16, C.byref(t), None) == abi.E_INVALID and t.value == 7
    assert L.sdrhip_resample_destroy(None) == abi.OK


def test_the_capacity_formula_is_the_headers():
    """floor((n + 1) / frac) + 2 in double from the float frac; n for a frac of 1; 0 for n = 0; a bank: the largest of its rows"""
    f = lambda v: float(np.float32(v))
    for frac, n, want in ((0.5, 300, 604), (2.0, 5, 5), (2.0, 10, 7), (7.9, 1000, int((1001.0) / f(7.9)) + 2), (1.0, 300, 300), (0.125, 256, 2058),
                          (4096.0, 4095, 3), (1.378125, 773, int(774.0 / f(1.378125)) + 2), (300.0, 255, 2), (0.5, 0, 0), (1.0, 0, 0)):
        assert R.out_capacity([frac], n) == want, (frac, n)
    assert R.out_capacity([1.0, 7.9], 300) == 300 and R.out_capacity([1.0, 0.5, 7.9], 300) == 604 and R.out_capacity([45.35, 7.9], 300) == 40


def test_the_four_kernels_exist_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(resample_[a-z0-9_]+_kernel)")
    assert seen == {"resample_f32_kernel": 0, "resample_cf32_kernel": 0, "resample_i16_kernel": 0, "resample_cs16_cf32_kernel": 0}, seen


# ---- the Python wrappers against a fake library --------------------------------------------------------------------------------

def _plan_info(args):
    args[2]._obj.value, args[3]._obj.value = 256, 4


def _get_state(args):
    for a, v in zip(args[1:5], (2.0, 0.5, 3.0, 3)):
        if a is not None:
            a._arr[...] = v


def _process(args):
    args[6]._arr[...] = (3, 1)   # counts
    args[4]._arr[...] = 9        # outputs


def _taps(args):
    args[0]._arr[...] = 0.5


def _run(monkeypatch):
    """The fake of test_nodes_calls.py, answering include/sdrhip_resample.h's names as well, and the table designer of
    sdrhip_psk31.h (out_capacity(n) answers n // 4); it records scalar arguments only, and no close hook."""
    from libsdr_amd import abi_psk31, abi_resample
    answers = {"sdrhip_resample_plan_info": _plan_info, "sdrhip_resample_get_state": _get_state, "sdrhip_resample_process": _process,
               "sdrhip_design_inpol_taps": _taps}
    sigs = dict(abi.SIGNATURES, **abi_psk31.SIGNATURES)
    sigs.update(abi_resample.SIGNATURES)
    return Run(monkeypatch, FakeLib(signatures=sigs, answers=answers, scalars_only=True), hook=False)


def _drive(r):
    from libsdr_amd import resample
    ctx = r.ctx()
    X = ramp((2, 16, 2), np.int16, 5)
    bank = resample.InpolSubSamplerBank(ctx, np.int16, [0.5, 7.9], iq=True, max_in=64)     # (no table: the designer's)
    assert (bank.dtype, bank.channels, bank.max_in, bank.iq, bank.out_dtype) == (3, 2, 64, True, np.float32) and np.all(bank.table == 0.5)
    assert bank.kernel_names == NAMES and bank.plan_info() == {"tile_samples": 256, "channels_per_group": 4}
    assert bank.out_capacity(16) == 4
    rows = bank.process(X)
    assert [r_.tolist() for r_ in rows] == [[[9, 9]] * 3, [[9, 9]]] and rows[0].dtype == np.float32
    r.route(True)
    routed = bank.process(X)                       # through the router: process_dev with the router's strides, counts from the device
    empty = bank.process(X[:, :0])                 # an empty call never meets the router
    r.route(False)
    assert [v.shape for v in empty] == [(0, 2), (0, 2)]
    bank.process_dev(0x1000, 16, 19, 0x2000, 7, 0x3000)
    bank.set_channel(1, 2.5)
    s = bank.get_state()
    assert s["frac"].tolist() == [2.0, 2.0] and s["mu"].tolist() == [0.5, 0.5] and s["line"].shape == (2, 8, 2) and np.all(s["line"] == 3.0)
    bank.reset()
    one = resample.InpolSubSampler(ctx, np.int16, 1.5, channels=2, table=R.table(), max_in=64)
    assert (one.dtype, one.frac, one.channels, one.iq, one.out_dtype) == (2, 1.5, 2, False, np.int16)
    s = one.get_state()
    assert s["line"].shape == (2, 8) and s["line"].dtype == np.int16 and np.all(s["line"] == 3)
    assert [v.tolist() for v in one.process(ramp((2, 16), np.int16, 9))] == [[9, 9, 9], [9]]
    for dtype, iq, code in ((np.float32, False, 0), (np.float32, True, 1), (3, False, 3)):
        n = resample.InpolSubSampler(ctx, dtype, 2.0, iq=iq, table=R.table(), max_in=64)
        assert n.dtype == code
        n.close()
    for o in (bank, bank, one, ctx):
        o.close()
    return routed


def test_wrapper_calls_against_the_fake_library(monkeypatch):
    r = _run(monkeypatch)
    _drive(r)
    names = [c[0] for c in r.fake.calls]
    assert names == [
        "sdrhip_ctx_create", "sdrhip_design_inpol_taps", "sdrhip_resamplebank_create", "sdrhip_resample_kernel_names", "sdrhip_resample_plan_info",
        "sdrhip_resample_out_capacity", "sdrhip_resample_out_capacity", "sdrhip_resample_process",
        "sdrhip_resample_out_capacity", "sdrhip_malloc", "router", "sdrhip_resample_process_dev", "sdrhip_memcpy_d2h",
        "sdrhip_resample_out_capacity", "sdrhip_resample_process",
        "sdrhip_resample_process_dev", "sdrhip_resample_set_channel", "sdrhip_resample_get_state", "sdrhip_resample_reset",
        "sdrhip_resample_create", "sdrhip_resample_get_state", "sdrhip_resample_out_capacity", "sdrhip_resample_process",
        "sdrhip_resample_create", "sdrhip_resample_destroy", "sdrhip_resample_create", "sdrhip_resample_destroy",
        "sdrhip_resample_create", "sdrhip_resample_destroy",
        "sdrhip_free", "sdrhip_resample_destroy", "sdrhip_resample_destroy", "sdrhip_ctx_destroy"], names
    calls = {}
    for c in r.fake.calls:
        calls.setdefault(c[0], []).append(c[1:])
    assert calls["sdrhip_resamplebank_create"][0][1] == 3 and calls["sdrhip_resamplebank_create"][0][4:6] == (2, 64)
    assert calls["sdrhip_resample_create"][0][1:3] == (2, 1.5) and calls["sdrhip_resample_create"][0][4:6] == (2, 64)
    assert [c[1] for c in calls["sdrhip_resample_create"]] == [2, 0, 1, 3]
    assert calls["sdrhip_resample_plan_info"][0][1] == 64                                   # 0: a call of max_in samples
    assert calls["sdrhip_resample_process"][0][2:4] == (16, 16) and calls["sdrhip_resample_process"][0][5] == 4
    assert calls["sdrhip_resample_process_dev"][0][2:4] == (16, 19) and calls["sdrhip_resample_process_dev"][0][5] == 4 + 3   # the router's strides
    assert calls["sdrhip_resample_process"][1][2:4] == (0, 0)
    assert calls["sdrhip_resample_process_dev"][1][2:4] == (16, 19) and calls["sdrhip_resample_process_dev"][1][5] == 7
    assert calls["sdrhip_resample_set_channel"][0][1:] == (1, 2.5)
    assert calls["sdrhip_resample_get_state"][0][-1] == 2
    from libsdr_amd import abi_resample
    assert set(abi_resample.SIGNATURES) <= r.fake.reached, sorted(set(abi_resample.SIGNATURES) - r.fake.reached)


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    from libsdr_amd import resample
    r = _run(monkeypatch)
    ctx = r.ctx()
    monkeypatch.setattr(resample.InpolSubSamplerBank, "_calls", resample.InpolSubSamplerBank._calls + " get_sttae")
    with pytest.raises(AttributeError, match="sdrhip_resample_get_sttae"):
        resample.InpolSubSamplerBank(ctx, np.int16, [2.0])
