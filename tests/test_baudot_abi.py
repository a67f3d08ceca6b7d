"""The Baudot decoder bank's C calls (include/sdrhip_baudot.h), what can be checked without a GPU: every function of the header is
exported by libsdrhip.so and has a prototype in libsdr_amd/abi_baudot.py, and nothing else of the family is exported; the header
is registered in abi.LATER_SIDE_HEADERS and not in abi.SIDE_HEADERS; every argument rule of the two create calls answers BEFORE
the context is looked at, in the header's order; the calls on a handle refuse a NULL one; the capacity formula; the kernel
exists for gfx950 and uses no scratch; and the Python wrappers, driven against the fake library of tests/test_nodes_calls.py,
make the calls they should."""
import ctypes as C

import numpy as np
import pytest

import baudot_restatement as B
from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes
from test_nodes_calls import FakeLib, NAMES, Run, ramp

NEW = ["sdrhip_baudot_channel_state", "sdrhip_baudot_create", "sdrhip_baudot_destroy", "sdrhip_baudot_get_channels",
       "sdrhip_baudot_kernel_names", "sdrhip_baudot_out_capacity", "sdrhip_baudot_process", "sdrhip_baudot_process_dev",
       "sdrhip_baudot_reset", "sdrhip_baudot_reset_channel", "sdrhip_baudot_set_channel", "sdrhip_baudot_set_channel_state",
       "sdrhip_baudot_set_enabled", "sdrhip_baudotbank_create"]
ip = C.POINTER(C.c_int)


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_baudot
    assert_header_binding(abi_baudot, NEW, r"\b(sdrhip_baudot[a-z0-9_]*)\b")


def test_the_header_is_in_the_second_table_only():
    import libsdr_amd  # noqa: F401   (the package imports every side header's module)
    from libsdr_amd import abi_baudot
    assert "sdrhip_baudot.h" in abi.LATER_SIDE_HEADERS and "sdrhip_baudot.h" not in abi.SIDE_HEADERS
    assert len(abi.SIDE_HEADERS) == 4
    assert abi.LATER_SIDE_HEADERS["sdrhip_baudot.h"].SIGNATURES is abi_baudot.SIGNATURES
    assert not set(abi_baudot.SIGNATURES) & set(abi.SIGNATURES)           # abi.SIGNATURES stays the binding of sdrhip.h alone
    assert sorted(abi.lib()._declared) == abi.header_functions()
    for name, side in list(abi.SIDE_HEADERS.items()) + list(abi.LATER_SIDE_HEADERS.items()):
        assert name == "sdrhip_baudot.h" or not set(abi_baudot.SIGNATURES) & set(side.SIGNATURES)


def test_the_package_exports_this_modules_classes():
    import libsdr_amd
    from libsdr_amd import baudot
    assert libsdr_amd.baudot is baudot and libsdr_amd.Baudot is baudot.Baudot and libsdr_amd.BaudotBank is baudot.BaudotBank
    assert issubclass(baudot.Baudot, baudot.BaudotBank) and issubclass(baudot.BaudotBank, nodes._Node) and issubclass(nodes._Node, nodes._Handle)
    assert not hasattr(nodes, "Baudot") and not hasattr(nodes, "BaudotBank")
    assert (baudot.STOP1, baudot.STOP15, baudot.STOP2, baudot.LETTERS, baudot.FIGURES) == (0, 1, 2, 0, 1)
    assert (B.STOP1, B.STOP15, B.STOP2, B.LETTERS, B.FIGURES) == (0, 1, 2, 0, 1)


def test_out_capacity_is_the_headers_formula():
    from libsdr_amd import abi_baudot
    L = abi_baudot.lib()
    for n in (0, 1, 13, 14, 15, 27, 28, 446, 2048, 65536):
        assert L.sdrhip_baudot_out_capacity(n) == n // 14 + 1 == B.out_capacity(n)
    # the most a row can complete: a symbol at position 0 (carried in) and one every 14 half-bits behind it
    for n in (1, 14, 15, 446):
        assert len(range(0, n, 14)) <= B.out_capacity(n)


def _bank(stops=(0, 1, 2), enabled=(1, 0, 1), channels=None, max_bits=2048, null=()):
    """(code, out) of sdrhip_baudotbank_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_baudot
    st, en = np.ascontiguousarray(stops, np.intc), np.ascontiguousarray(enabled, np.intc)
    h = C.c_void_p(0x1)
    code = abi_baudot.lib().sdrhip_baudotbank_create(None, None if "stops" in null else st.ctypes.data_as(ip),
                                                     None if "enabled" in null or en.size != st.size else en.ctypes.data_as(ip),
                                                     st.size if channels is None else channels, max_bits, None if "out" in null else C.byref(h))
    return code, h.value


def _one(stop=1, channels=3, max_bits=2048, null=()):
    from libsdr_amd import abi_baudot
    h = C.c_void_p(0x1)
    code = abi_baudot.lib().sdrhip_baudot_create(None, stop, channels, max_bits, None if "out" in null else C.byref(h))
    return code, h.value


def test_create_without_a_context():
    for code, h in (_bank(), _bank(null=("enabled",)), _one(), _one(stop=0), _one(stop=2), _one(channels=1), _one(channels=8192), _one(max_bits=1),
                    _one(max_bits=65536), _bank(stops=(2,) * 8192), _bank(max_bits=1), _bank(max_bits=65536)):
        assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


ONE_RULES = [
    (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(stop=3), abi.E_INVALID, "stop"), (dict(stop=-1), abi.E_INVALID, "stop"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=-1), abi.E_INVALID, "channels"), (dict(channels=8193), abi.E_INVALID, "channels"),
    (dict(max_bits=0), abi.E_SIZE, "max_bits"), (dict(max_bits=65537), abi.E_SIZE, "max_bits"),
    # in the header's order: out, stop, channels, max_bits
    (dict(null=("out",), stop=3), abi.E_INVALID, "NULL"), (dict(stop=3, channels=0), abi.E_INVALID, "stop"),
    (dict(channels=0, max_bits=0), abi.E_INVALID, "channels"),
]
BANK_RULES = [
    (dict(null=("stops",)), abi.E_INVALID, "NULL"), (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=-1), abi.E_INVALID, "channels"),
    (dict(stops=(1,) * 8193), abi.E_INVALID, "channels"),
    (dict(max_bits=0), abi.E_SIZE, "max_bits"), (dict(max_bits=65537), abi.E_SIZE, "max_bits"),
    (dict(stops=(0, 3, 1)), abi.E_INVALID, "stops[1]"), (dict(stops=(0, 1, -1)), abi.E_INVALID, "stops[2]"),
    # in the header's order: the pointers, channels, max_bits, the settings
    (dict(null=("stops",), channels=0), abi.E_INVALID, "NULL"), (dict(null=("out",), max_bits=0), abi.E_INVALID, "NULL"),
    (dict(channels=0, max_bits=0), abi.E_INVALID, "channels"), (dict(max_bits=0, stops=(0, 3, 1)), abi.E_SIZE, "max_bits"),
]


@pytest.mark.parametrize("kw,want,text", ONE_RULES, ids=[str(i) for i in range(len(ONE_RULES))])
def test_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _one(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


@pytest.mark.parametrize("kw,want,text", BANK_RULES, ids=[str(i) for i in range(len(BANK_RULES))])
def test_bank_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _bank(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_baudot
    L = abi_baudot.lib()
    e, m, bs, bc = (C.c_int * 4)(), C.c_int(7), C.c_uint16(9), C.c_uint64(11)
    buf = C.create_string_buffer(64)
    assert L.sdrhip_baudot_process_dev(None, None, 0, None, None, 0, None, None) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_baudot_process(None, None, 0, None, None, 0, None) == abi.E_INVALID and "NULL" in last_error()
    for call in (lambda: L.sdrhip_baudot_set_channel(None, 0, 1), lambda: L.sdrhip_baudot_set_enabled(None, 0, 1),
                 lambda: L.sdrhip_baudot_get_channels(None, e, e, 4), lambda: L.sdrhip_baudot_reset(None, 0),
                 lambda: L.sdrhip_baudot_reset_channel(None, 0, 1), lambda: L.sdrhip_baudot_set_channel_state(None, 0, 0, 0, 0),
                 lambda: L.sdrhip_baudot_kernel_names(None, buf, 64)):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_baudot_channel_state(None, 0, C.byref(bs), C.byref(bc), C.byref(m)) == abi.E_INVALID
    assert (bs.value, bc.value, m.value) == (9, 11, 7)
    assert L.sdrhip_baudot_destroy(None) == abi.OK


def test_the_kernel_exists_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(baudot_[a-z0-9_]+_kernel)")
    assert seen == {"baudot_decode_kernel": 0}, seen


# ---- the Python wrappers against a fake library --------------------------------------------------------------------------------

class Fake(FakeLib):
    """sdrhip_baudot_out_capacity returns its answer, where the other calls return a code."""

    def _call(self, name, args):
        code = super()._call(name, args)
        return args[0] // 14 + 1 if name == "sdrhip_baudot_out_capacity" else code


def _process(args):
    args[4]._arr[...] = ord("R")       # text
    args[6]._arr[...] = (2, 0)         # out_counts


def _state(args):
    args[2]._obj.value, args[3]._obj.value, args[4]._obj.value = 0x6000, 1 << 40, 1


def _channels(args):
    for k in range(args[3]):
        args[1][k], args[2][k] = 2 - k, k


def _run(monkeypatch):
    from libsdr_amd import abi_baudot
    answers = {"sdrhip_baudot_out_capacity": lambda args: None, "sdrhip_baudot_process": _process, "sdrhip_baudot_channel_state": _state,
               "sdrhip_baudot_get_channels": _channels}
    return Run(monkeypatch, Fake(signatures=dict(abi.SIGNATURES, **abi_baudot.SIGNATURES), answers=answers, scalars_only=True), hook=False)


def test_wrapper_calls_against_the_fake_library(monkeypatch):
    from libsdr_amd import abi_baudot, baudot
    r = _run(monkeypatch)
    ctx = r.ctx()
    bank = baudot.BaudotBank(ctx, [baudot.STOP1, baudot.STOP2], 64, enabled=[True, False])
    assert (bank.channels, bank.max_bits) == (2, 64) and bank.kernel_names == NAMES
    assert bank.out_capacity() == 5 and bank.out_capacity(446) == 32
    text, counts = bank.process(ramp((2, 20), np.uint8, 3), [20, 7])
    assert text.shape == (2, 5) and counts.tolist() == [2, 0] and bank.text(0) == b"RR" and bank.text(1) == b""
    r.route(True)
    bank.process(ramp((2, 20), np.uint8, 3), [20, 7])   # through the router: process_dev with the router's strides
    r.route(False)
    bank.process_dev(0x1000, 23, 0x2000, 0x3000, 9, 0x4000)
    bank.process_dev(0x1000, 23, 0x2000, 0x3000, 9, 0x4000, 0x5000)
    bank.set_channel(1, baudot.STOP15)
    bank.set_enabled(1, True)
    assert bank.get_channels() == ([2, 1], [False, True])
    bank.reset()
    bank.reset(keep_mode=True)
    bank.reset_channel(1, keep_mode=True)
    assert bank.channel_state(0) == (0x6000, 1 << 40, baudot.FIGURES)
    bank.set_channel_state(1, 0xC00F, 17, baudot.FIGURES)
    one = baudot.Baudot(ctx, 3, 446)
    assert (one.channels, one.max_bits, one.stop) == (3, 446, baudot.STOP15)
    for o in (bank, bank, one, ctx):
        o.close()
    names = [c[0] for c in r.fake.calls]
    assert names == [
        "sdrhip_ctx_create", "sdrhip_baudotbank_create", "sdrhip_baudot_kernel_names", "sdrhip_baudot_out_capacity", "sdrhip_baudot_out_capacity",
        "sdrhip_baudot_out_capacity", "sdrhip_baudot_process",
        "sdrhip_baudot_out_capacity", "sdrhip_malloc", "sdrhip_memcpy_h2d", "router", "sdrhip_baudot_process_dev", "sdrhip_memcpy_d2h",
        "sdrhip_baudot_process_dev", "sdrhip_baudot_process_dev", "sdrhip_baudot_set_channel", "sdrhip_baudot_set_enabled",
        "sdrhip_baudot_get_channels", "sdrhip_baudot_reset", "sdrhip_baudot_reset", "sdrhip_baudot_reset_channel", "sdrhip_baudot_channel_state",
        "sdrhip_baudot_set_channel_state", "sdrhip_baudot_create", "sdrhip_free", "sdrhip_baudot_destroy", "sdrhip_baudot_destroy",
        "sdrhip_ctx_destroy"], names
    calls = {}
    for c in r.fake.calls:
        calls.setdefault(c[0], []).append(c[1:])
    assert calls["sdrhip_baudotbank_create"][0][3:5] == (2, 64)
    assert calls["sdrhip_baudot_create"][0][1:4] == (baudot.STOP15, 3, 446)
    assert calls["sdrhip_baudot_process"][0][2] == 20 and calls["sdrhip_baudot_process"][0][5] == 5
    assert calls["sdrhip_baudot_process_dev"][0][2] == 20 + 3 and calls["sdrhip_baudot_process_dev"][0][5] == 5 + 3   # the router's strides
    assert calls["sdrhip_baudot_process_dev"][1][2] == 23 and calls["sdrhip_baudot_process_dev"][1][5] == 9
    assert calls["sdrhip_baudot_set_channel"][0][1:] == (1, baudot.STOP15) and calls["sdrhip_baudot_set_enabled"][0][1:] == (1, 1)
    assert [c[1] for c in calls["sdrhip_baudot_reset"]] == [0, 1] and calls["sdrhip_baudot_reset_channel"][0][1:] == (1, 1)
    assert calls["sdrhip_baudot_set_channel_state"][0][1:] == (1, 0xC00F, 17, baudot.FIGURES)
    assert set(abi_baudot.SIGNATURES) <= r.fake.reached, sorted(set(abi_baudot.SIGNATURES) - r.fake.reached)


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    from libsdr_amd import baudot
    r = _run(monkeypatch)
    ctx = r.ctx()
    monkeypatch.setattr(baudot.BaudotBank, "_calls", baudot.BaudotBank._calls + " channel_sttae")
    with pytest.raises(AttributeError, match="sdrhip_baudot_channel_sttae"):
        baudot.BaudotBank(ctx, [baudot.STOP15], 64)
