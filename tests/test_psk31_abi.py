"""The BPSK31 bank's C calls (include/sdrhip_psk31.h), what can be checked without a GPU: every function of the header is exported
by libsdrhip.so and has a prototype in libsdr_amd/abi_psk31.py, and nothing else of the family is exported (tests/test_side_headers.py
holds what the headers' bindings owe each other); every argument rule of the two create calls answers BEFORE the context is looked at, in the header's
order; the calls on a handle refuse a NULL one; both kernels exist for gfx950 and use no scratch; and the Python wrappers, driven
against the fake library of tests/test_nodes_calls.py, make the calls they should."""
import ctypes as C

import numpy as np
import pytest

import psk31_restatement as R
from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes
from test_nodes_calls import FakeLib, NAMES, Run, ramp

NEW = ["sdrhip_design_inpol_taps", "sdrhip_psk31_create", "sdrhip_psk31_destroy", "sdrhip_psk31_get_state", "sdrhip_psk31_kernel_names",
       "sdrhip_psk31_out_capacity", "sdrhip_psk31_plan_info", "sdrhip_psk31_process", "sdrhip_psk31_process_dev", "sdrhip_psk31_reset",
       "sdrhip_psk31_set_channel", "sdrhip_psk31bank_create"]
fp = C.POINTER(C.c_float)
INF, NAN = float("inf"), float("nan")


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_psk31
    assert_header_binding(abi_psk31, NEW, r"\b(sdrhip_(?:psk31[a-z0-9_]*|design_inpol[a-z0-9_]*))\b")


def test_the_package_exports_this_modules_classes():
    import libsdr_amd
    from libsdr_amd import psk31
    assert libsdr_amd.BPSK31 is psk31.BPSK31 and libsdr_amd.BPSK31Bank is psk31.BPSK31Bank and libsdr_amd.Varicode is psk31.Varicode
    assert issubclass(psk31.BPSK31, psk31.BPSK31Bank) and issubclass(psk31.BPSK31Bank, nodes._Node)


def _bank(dtype=0, Fs=8000.0, dF=(0.1, 0.05, 3.0), table=None, channels=None, max_in=1024, null=()):
    """(code, out) of sdrhip_psk31bank_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_psk31
    dF = np.ascontiguousarray(dF, np.float32)
    t = np.ascontiguousarray(R.table() if table is None else table, np.float32)
    h = C.c_void_p(0x1)
    code = abi_psk31.lib().sdrhip_psk31bank_create(None, dtype, Fs, None if "dF" in null else dF.ctypes.data_as(fp),
                                                   None if "table" in null else t.ctypes.data_as(fp), dF.size if channels is None else channels,
                                                   max_in, None if "out" in null else C.byref(h))
    return code, h.value


def _one(dtype=0, Fs=8000.0, dF=0.1, table=None, channels=3, max_in=1024, null=()):
    from libsdr_amd import abi_psk31
    t = np.ascontiguousarray(R.table() if table is None else table, np.float32)
    h = C.c_void_p(0x1)
    code = abi_psk31.lib().sdrhip_psk31_create(None, dtype, Fs, dF, None if "table" in null else t.ctypes.data_as(fp), channels, max_in,
                                               None if "out" in null else C.byref(h))
    return code, h.value


def test_create_without_a_context():
    for code, h in (_bank(), _one(), _bank(dtype=1), _one(dtype=1), _one(Fs=2000.0), _one(dF=np.pi), _one(channels=1), _one(channels=65535),
                    _one(max_in=1), _one(max_in=(1 << 30) - 1), _one(Fs=1e6)):
        assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


def _bad_table(v):
    t = R.table().copy()
    t[77, 3] = v
    return t


RULES = [
    (dict(null=("table",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(dtype=2), abi.E_INVALID, "dtype"), (dict(dtype=-1), abi.E_INVALID, "dtype"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=65536), abi.E_INVALID, "channels"),
    (dict(max_in=0), abi.E_SIZE, "max_in"), (dict(max_in=1 << 30), abi.E_SIZE, "max_in"),
    (dict(Fs=1999.9), abi.E_INVALID, "sample_rate"), (dict(Fs=NAN), abi.E_INVALID, "sample_rate"), (dict(Fs=INF), abi.E_INVALID, "sample_rate"),
    (dict(Fs=-8000.0), abi.E_INVALID, "sample_rate"),
    (dict(table=_bad_table(NAN)), abi.E_INVALID, "table"), (dict(table=_bad_table(-INF)), abi.E_INVALID, "table"),
    # in the header's order
    (dict(null=("out",), dtype=2), abi.E_INVALID, "NULL"), (dict(dtype=2, channels=0), abi.E_INVALID, "dtype"),
    (dict(channels=0, max_in=0), abi.E_INVALID, "channels"), (dict(max_in=0, Fs=100.0), abi.E_SIZE, "max_in"),
]
BANK_RULES = RULES + [
    (dict(null=("dF",)), abi.E_INVALID, "NULL"),
    (dict(dF=(0.1, 0.0, 0.1)), abi.E_INVALID, "dF"), (dict(dF=(0.1, 0.1, -0.1)), abi.E_INVALID, "dF"), (dict(dF=(NAN, 0.1, 0.1)), abi.E_INVALID, "dF"),
    (dict(dF=(0.1, 3.2, 0.1)), abi.E_INVALID, "dF"), (dict(dF=(0.1, INF, 0.1)), abi.E_INVALID, "dF"),
    (dict(Fs=100.0, dF=(0.0, 0.1, 0.1)), abi.E_INVALID, "sample_rate"), (dict(dF=(0.0, 0.1, 0.1), table=_bad_table(NAN)), abi.E_INVALID, "dF"),
]
ONE_RULES = RULES + [
    (dict(dF=0.0), abi.E_INVALID, "dF"), (dict(dF=-0.1), abi.E_INVALID, "dF"), (dict(dF=NAN), abi.E_INVALID, "dF"), (dict(dF=3.15), abi.E_INVALID, "dF"),
    (dict(Fs=100.0, dF=0.0), abi.E_INVALID, "sample_rate"), (dict(dF=0.0, table=_bad_table(INF)), abi.E_INVALID, "dF"),
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
    from libsdr_amd import abi_psk31
    L = abi_psk31.lib()
    g, e, t, sz = (C.c_float * 4)(), (C.c_int * 4)(), C.c_int(7), C.c_size_t(9)
    buf = C.create_string_buffer(64)
    assert L.sdrhip_psk31_process_dev(None, None, 0, 0, None, 0, None) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_psk31_process(None, None, 0, 0, None, 0, None) == abi.E_INVALID and "NULL" in last_error()
    for call in (lambda: L.sdrhip_psk31_set_channel(None, 0, 0.1), lambda: L.sdrhip_psk31_get_state(None, g, g, g, g, e, e, 4),
                 lambda: L.sdrhip_psk31_reset(None), lambda: L.sdrhip_psk31_kernel_names(None, buf, 64),
                 lambda: L.sdrhip_psk31_out_capacity(None, 16, C.byref(sz))):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert sz.value == 9
    assert L.sdrhip_psk31_plan_info(None, 16, C.byref(t), None) == abi.E_INVALID and t.value == 7
    assert L.sdrhip_psk31_destroy(None) == abi.OK
    assert L.sdrhip_design_inpol_taps(None) == abi.E_INVALID


def test_both_kernels_exist_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(psk31_[a-z0-9_]+_kernel)")
    assert seen == {"psk31_cs16_kernel": 0, "psk31_cf32_kernel": 0}, seen


# ---- the Python wrappers against a fake library --------------------------------------------------------------------------------

def _plan_info(args):
    args[2]._obj.value, args[3]._obj.value = 256, 4


def _get_state(args):
    for a, v in zip(args[1:7], (1.0, 2.0, 3.0, 4.0, 5, -1)):
        a._arr[...] = v


def _process(args):
    args[6]._arr[...] = (2, 1)   # counts
    args[4]._arr[...] = 1        # bits


def _taps(args):
    args[0]._arr[...] = 0.5


def _run(monkeypatch):
    """The fake of test_nodes_calls.py, answering include/sdrhip_psk31.h's names as well (out_capacity(n) answers n // 4); it
    records scalar arguments only, and no close hook."""
    from libsdr_amd import abi_psk31
    answers = {"sdrhip_psk31_plan_info": _plan_info, "sdrhip_psk31_get_state": _get_state, "sdrhip_psk31_process": _process,
               "sdrhip_design_inpol_taps": _taps}
    return Run(monkeypatch, FakeLib(signatures=dict(abi.SIGNATURES, **abi_psk31.SIGNATURES), answers=answers, scalars_only=True), hook=False)


def _drive(r):
    from libsdr_amd import psk31
    ctx = r.ctx()
    X = ramp((2, 16, 2), np.int16, 5)
    bank = psk31.BPSK31Bank(ctx, np.int16, 8000.0, [0.1, 0.05], max_in=64)     # (no table: the designer's)
    assert (bank.dtype, bank.channels, bank.max_in, bank.Fs) == (0, 2, 64, 8000.0) and np.all(bank.table == 0.5)
    assert bank.kernel_names == NAMES and bank.plan_info() == {"tile_samples": 256, "channels_per_group": 4}
    assert bank.out_capacity(16) == 4
    rows = bank.process(X)
    assert [r_.tolist() for r_ in rows] == [[1, 1], [1]]
    r.route(True)
    routed = bank.process(X)                       # through the router: process_dev with the router's strides, counts from the device
    empty = bank.process(X[:, :0])                 # an empty call never meets the router
    r.route(False)
    assert [len(v) for v in empty] == [0, 0]
    bank.process_dev(0x1000, 16, 19, 0x2000, 7, 0x3000)
    bank.set_channel(1, 0.02)
    s = bank.get_state()
    assert s["P"].tolist() == [1.0, 1.0] and s["omega"].tolist() == [4.0, 4.0] and s["hist_idx"].tolist() == [5, 5] and s["last"].tolist() == [-1, -1]
    bank.reset()
    one = psk31.BPSK31(ctx, np.float32, 2000.0, channels=2, table=R.table(), max_in=64)
    assert (one.dtype, one.dF, one.channels) == (1, 0.1, 2)
    one.process(ramp((2, 16, 2), np.float32, 9))
    for o in (bank, bank, one, ctx):
        o.close()
    return routed


def test_wrapper_calls_against_the_fake_library(monkeypatch):
    r = _run(monkeypatch)
    _drive(r)
    names = [c[0] for c in r.fake.calls]
    assert names == [
        "sdrhip_ctx_create", "sdrhip_design_inpol_taps", "sdrhip_psk31bank_create", "sdrhip_psk31_kernel_names", "sdrhip_psk31_plan_info",
        "sdrhip_psk31_out_capacity", "sdrhip_psk31_out_capacity", "sdrhip_psk31_process",
        "sdrhip_psk31_out_capacity", "sdrhip_malloc", "router", "sdrhip_psk31_process_dev", "sdrhip_memcpy_d2h",
        "sdrhip_psk31_out_capacity", "sdrhip_psk31_process",
        "sdrhip_psk31_process_dev", "sdrhip_psk31_set_channel", "sdrhip_psk31_get_state", "sdrhip_psk31_reset",
        "sdrhip_psk31_create", "sdrhip_psk31_out_capacity", "sdrhip_psk31_process",
        "sdrhip_free", "sdrhip_psk31_destroy", "sdrhip_psk31_destroy", "sdrhip_ctx_destroy"], names
    calls = {}
    for c in r.fake.calls:
        calls.setdefault(c[0], []).append(c[1:])
    assert calls["sdrhip_psk31bank_create"][0][1:3] == (0, 8000.0) and calls["sdrhip_psk31bank_create"][0][5:7] == (2, 64)
    assert calls["sdrhip_psk31_create"][0][1:4] == (1, 2000.0, 0.1) and calls["sdrhip_psk31_create"][0][5:7] == (2, 64)
    assert calls["sdrhip_psk31_plan_info"][0][1] == 64                                   # 0: a call of max_in samples
    assert calls["sdrhip_psk31_process"][0][2:4] == (16, 16) and calls["sdrhip_psk31_process"][0][5] == 4
    assert calls["sdrhip_psk31_process_dev"][0][2:4] == (16, 19) and calls["sdrhip_psk31_process_dev"][0][5] == 4 + 3   # the router's strides
    assert calls["sdrhip_psk31_process"][1][2:4] == (0, 0)
    assert calls["sdrhip_psk31_process_dev"][1][2:4] == (16, 19) and calls["sdrhip_psk31_process_dev"][1][5] == 7
    assert calls["sdrhip_psk31_set_channel"][0][1:] == (1, 0.02)
    assert calls["sdrhip_psk31_get_state"][0][-1] == 2
    from libsdr_amd import abi_psk31
    assert set(abi_psk31.SIGNATURES) <= r.fake.reached, sorted(set(abi_psk31.SIGNATURES) - r.fake.reached)


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    from libsdr_amd import psk31
    r = _run(monkeypatch)
    ctx = r.ctx()
    monkeypatch.setattr(psk31.BPSK31Bank, "_calls", psk31.BPSK31Bank._calls + " get_sttae")
    with pytest.raises(AttributeError, match="sdrhip_psk31_get_sttae"):
        psk31.BPSK31Bank(ctx, np.int16, 8000.0, [0.1])
