"""The AX.25 deframer bank's C calls (include/sdrhip_ax25.h), what can be checked without a GPU: every function of the header is
exported by libsdrhip.so and has a prototype in libsdr_amd/abi_ax25.py, and nothing else of the family is exported; the header is
registered in abi.LATER_SIDE_HEADERS and not in abi.SIDE_HEADERS; every argument rule of the create call answers BEFORE the
context is looked at, in the header's order; the calls on a handle refuse a NULL one; the capacity formulas; the kernel exists
for gfx950 and uses no scratch; and the Python wrappers, driven against the fake library of tests/test_nodes_calls.py, make the
calls they should."""
import ctypes as C

import numpy as np
import pytest

import ax25_restatement as R
from abi_checks import assert_header_binding, kernel_scratch, last_error, no_ctx_code
from libsdr_amd import abi, nodes
from test_nodes_calls import FakeLib, NAMES, Run, ramp

NEW = ["sdrhip_ax25_bytes_capacity", "sdrhip_ax25_channel_state", "sdrhip_ax25_create", "sdrhip_ax25_destroy", "sdrhip_ax25_frames_capacity",
       "sdrhip_ax25_get_enabled", "sdrhip_ax25_kernel_names", "sdrhip_ax25_process", "sdrhip_ax25_process_dev", "sdrhip_ax25_reset",
       "sdrhip_ax25_reset_channel", "sdrhip_ax25_set_channel_state", "sdrhip_ax25_set_enabled"]
ip = C.POINTER(C.c_int)


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_ax25
    assert_header_binding(abi_ax25, NEW, r"\b(sdrhip_ax25[a-z0-9_]*)\b")


def test_the_header_is_in_the_second_table_only():
    import libsdr_amd  # noqa: F401   (the package imports every side header's module)
    from libsdr_amd import abi_ax25
    assert "sdrhip_ax25.h" in abi.LATER_SIDE_HEADERS and "sdrhip_ax25.h" not in abi.SIDE_HEADERS
    assert len(abi.SIDE_HEADERS) == 4
    assert abi.LATER_SIDE_HEADERS["sdrhip_ax25.h"].SIGNATURES is abi_ax25.SIGNATURES
    assert not set(abi_ax25.SIGNATURES) & set(abi.SIGNATURES)           # abi.SIGNATURES stays the binding of sdrhip.h alone
    assert sorted(abi.lib()._declared) == abi.header_functions()
    for name, side in list(abi.SIDE_HEADERS.items()) + list(abi.LATER_SIDE_HEADERS.items()):
        assert name == "sdrhip_ax25.h" or not set(abi_ax25.SIGNATURES) & set(side.SIGNATURES)


def test_the_package_exports_this_modules_classes():
    import libsdr_amd
    from libsdr_amd import abi_ax25, ax25, pocsag
    assert libsdr_amd.ax25 is ax25 and libsdr_amd.AX25 is ax25.AX25 and libsdr_amd.AX25Bank is ax25.AX25Bank
    assert issubclass(ax25.AX25, ax25.AX25Bank) and issubclass(ax25.AX25Bank, nodes._Node) and issubclass(nodes._Node, nodes._Handle)
    assert not hasattr(nodes, "AX25") and not hasattr(nodes, "AX25Bank")
    assert libsdr_amd.Message is pocsag.Message and ax25.Message is not pocsag.Message   # the pager's keeps the package's name
    assert abi_ax25.RXBUFFER == ax25.RXBUFFER == R.RX_MAX == 512


def test_the_capacities_are_the_headers_formulas():
    from libsdr_amd import abi_ax25
    L = abi_ax25.lib()
    for n in (0, 1, 7, 8, 24, 25, 26, 49, 50, 446, 4096, 65536):
        assert L.sdrhip_ax25_frames_capacity(n) == n // 25 + 1 == R.frames_capacity(n)
        assert L.sdrhip_ax25_bytes_capacity(n) == n // 8 + 512 == R.bytes_capacity(n)
        # the most a row can deliver: a frame at position 0 (carried in) and one every 25 positions behind it; 510 carried bytes
        # closed by the last position, a byte for every eight positions before it
        assert len(range(0, n, 25)) <= R.frames_capacity(n)
        assert R.bytes_most(n) <= R.bytes_capacity(n)


def _create(enabled=(1, 0, 1), channels=None, max_bits=2048, null=()):
    """(code, out) of sdrhip_ax25_create with a NULL context; `null` names pointer arguments passed as NULL."""
    from libsdr_amd import abi_ax25
    en = np.ascontiguousarray(enabled, np.intc)
    h = C.c_void_p(0x1)
    code = abi_ax25.lib().sdrhip_ax25_create(None, None if "enabled" in null else en.ctypes.data_as(ip), en.size if channels is None else channels,
                                             max_bits, None if "out" in null else C.byref(h))
    return code, h.value


def test_create_without_a_context():
    for code, h in (_create(), _create(null=("enabled",)), _create(channels=1), _create(null=("enabled",), channels=8192), _create(max_bits=1),
                    _create(max_bits=65536)):
        assert code == no_ctx_code() and h is None
    if nodes.device_count() == 0:
        assert "no CPU fallback" in last_error()


RULES = [
    (dict(null=("out",)), abi.E_INVALID, "NULL"),
    (dict(channels=0), abi.E_INVALID, "channels"), (dict(channels=-1), abi.E_INVALID, "channels"),
    (dict(null=("enabled",), channels=8193), abi.E_INVALID, "channels"),
    (dict(max_bits=0), abi.E_SIZE, "max_bits"), (dict(max_bits=65537), abi.E_SIZE, "max_bits"),
    # in the header's order: out, channels, max_bits
    (dict(null=("out",), channels=0), abi.E_INVALID, "NULL"), (dict(null=("out",), max_bits=0), abi.E_INVALID, "NULL"),
    (dict(channels=0, max_bits=0), abi.E_INVALID, "channels"),
]


@pytest.mark.parametrize("kw,want,text", RULES, ids=[str(i) for i in range(len(RULES))])
def test_create_argument_rules_come_before_the_context(kw, want, text):
    code, h = _create(**kw)
    assert code == want and (h is None or "out" in kw.get("null", ())), (kw, code)
    assert text in last_error(), (kw, last_error())


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_ax25
    L = abi_ax25.lib()
    e, st, ln, bs, bb = (C.c_int * 4)(), C.c_int(7), C.c_int(5), C.c_uint32(9), C.c_uint32(11)
    rx = (C.c_uint8 * 512)()
    buf = C.create_string_buffer(64)
    assert L.sdrhip_ax25_process_dev(None, None, 0, None, None, 0, None, 0, None, None) == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_ax25_process(None, None, 0, None, None, 0, None, 0, None) == abi.E_INVALID and "NULL" in last_error()
    for call in (lambda: L.sdrhip_ax25_set_enabled(None, 0, 1), lambda: L.sdrhip_ax25_get_enabled(None, e, 4), lambda: L.sdrhip_ax25_reset(None),
                 lambda: L.sdrhip_ax25_reset_channel(None, 0), lambda: L.sdrhip_ax25_set_channel_state(None, 0, 0, 0x80, 1, 0, rx),
                 lambda: L.sdrhip_ax25_kernel_names(None, buf, 64)):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert L.sdrhip_ax25_channel_state(None, 0, C.byref(bs), C.byref(bb), C.byref(st), C.byref(ln), rx) == abi.E_INVALID
    assert (bs.value, bb.value, st.value, ln.value) == (9, 11, 7, 5)
    assert L.sdrhip_ax25_destroy(None) == abi.OK


def test_the_kernel_exists_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(ax25_[a-z0-9_]+_kernel)")
    assert seen == {"ax25_deframe_kernel": 0}, seen


# ---- the Python wrappers against a fake library --------------------------------------------------------------------------------

class Fake(FakeLib):
    """The two capacity calls return their answer, where the other calls return a code."""

    def _call(self, name, args):
        code = super()._call(name, args)
        if name == "sdrhip_ax25_frames_capacity":
            return args[0] // 25 + 1
        return args[0] // 8 + 512 if name == "sdrhip_ax25_bytes_capacity" else code


def _process(args):
    args[4]._arr[0, :5] = list(b"HELLO")           # bytes
    args[6]._arr[0, :2] = [[0, 2 | 30 << 16], [2, 3 | 61 << 16]]   # events
    args[8]._arr[...] = (2, 0)                     # frame counts


def _state(args):
    args[2]._obj.value, args[3]._obj.value, args[4]._obj.value, args[5]._obj.value = 0xDEADBEEF, 0x40, 1, 3
    args[6][0], args[6][1], args[6][2] = 1, 2, 3


def _enabled(args):
    for k in range(args[2]):
        args[1][k] = k


def _run(monkeypatch):
    from libsdr_amd import abi_ax25
    answers = {"sdrhip_ax25_frames_capacity": lambda args: None, "sdrhip_ax25_bytes_capacity": lambda args: None,
               "sdrhip_ax25_process": _process, "sdrhip_ax25_channel_state": _state, "sdrhip_ax25_get_enabled": _enabled}
    return Run(monkeypatch, Fake(signatures=dict(abi.SIGNATURES, **abi_ax25.SIGNATURES), answers=answers, scalars_only=True), hook=False)


def test_wrapper_calls_against_the_fake_library(monkeypatch):
    from libsdr_amd import abi_ax25, ax25
    r = _run(monkeypatch)
    ctx = r.ctx()
    bank = ax25.AX25Bank(ctx, 2, 64, enabled=[True, False])
    assert (bank.channels, bank.max_bits) == (2, 64) and bank.kernel_names == NAMES
    assert bank.frames_capacity() == 3 and bank.frames_capacity(446) == 18 and bank.bytes_capacity() == 520 and bank.bytes_capacity(446) == 567
    data, ev, fc = bank.process(ramp((2, 20), np.uint8, 3), [20, 7])
    assert data.shape == (2, 520) and ev.shape == (2, 3, 2) and fc.tolist() == [2, 0]
    assert bank.frames(0) == [(b"HE", 30), (b"LLO", 61)] and bank.frames(1) == []
    r.route(True)
    bank.process(ramp((2, 20), np.uint8, 3), [20, 7])   # through the router: process_dev with the router's strides
    r.route(False)
    bank.process_dev(0x1000, 23, 0x2000, 0x3000, 600, 0x4000, 9, 0x5000)
    bank.process_dev(0x1000, 23, 0x2000, 0x3000, 600, 0x4000, 9, 0x5000, 0x6000)
    bank.set_enabled(1, True)
    assert bank.get_enabled() == [False, True]
    bank.reset()
    bank.reset_channel(1)
    assert bank.channel_state(0) == (0xDEADBEEF, 0x40, 1, 3, b"\x01\x02\x03")
    bank.set_channel_state(1, 0x7E, 0x80, 1, b"ab")
    one = ax25.AX25(ctx, 3, 446)
    assert (one.channels, one.max_bits) == (3, 446)
    for o in (bank, bank, one, ctx):
        o.close()
    names = [c[0] for c in r.fake.calls]
    cap2 = ["sdrhip_ax25_bytes_capacity", "sdrhip_ax25_frames_capacity"]
    assert names == [
        "sdrhip_ctx_create", "sdrhip_ax25_create", "sdrhip_ax25_kernel_names", "sdrhip_ax25_frames_capacity", "sdrhip_ax25_frames_capacity",
        "sdrhip_ax25_bytes_capacity", "sdrhip_ax25_bytes_capacity"] + cap2 + ["sdrhip_ax25_process"] + cap2 + [
        "sdrhip_malloc", "sdrhip_memcpy_h2d", "sdrhip_memcpy_h2d", "router", "sdrhip_ax25_process_dev", "sdrhip_memcpy_d2h", "sdrhip_memcpy_d2h",
        "sdrhip_ax25_process_dev", "sdrhip_ax25_process_dev", "sdrhip_ax25_set_enabled", "sdrhip_ax25_get_enabled", "sdrhip_ax25_reset",
        "sdrhip_ax25_reset_channel", "sdrhip_ax25_channel_state", "sdrhip_ax25_set_channel_state", "sdrhip_ax25_create", "sdrhip_free",
        "sdrhip_ax25_destroy", "sdrhip_ax25_destroy", "sdrhip_ctx_destroy"], names
    calls = {}
    for c in r.fake.calls:
        calls.setdefault(c[0], []).append(c[1:])
    assert calls["sdrhip_ax25_create"][0][2:4] == (2, 64) and calls["sdrhip_ax25_create"][1][1:4] == (None, 3, 446)
    assert calls["sdrhip_ax25_process"][0][2] == 20 and calls["sdrhip_ax25_process"][0][5] == 520 and calls["sdrhip_ax25_process"][0][7] == 3
    assert calls["sdrhip_ax25_process_dev"][0][2] == 20 + 3 and calls["sdrhip_ax25_process_dev"][0][5] == 520 + 3   # the router's strides
    assert calls["sdrhip_ax25_process_dev"][0][7] == 3
    assert calls["sdrhip_ax25_process_dev"][1][2] == 23 and calls["sdrhip_ax25_process_dev"][1][5] == 600 and calls["sdrhip_ax25_process_dev"][1][7] == 9
    assert calls["sdrhip_ax25_set_enabled"][0][1:] == (1, 1) and calls["sdrhip_ax25_reset_channel"][0][1:] == (1,)
    assert calls["sdrhip_ax25_set_channel_state"][0][1:6] == (1, 0x7E, 0x80, 1, 2)
    assert set(abi_ax25.SIGNATURES) <= r.fake.reached, sorted(set(abi_ax25.SIGNATURES) - r.fake.reached)


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    from libsdr_amd import ax25
    r = _run(monkeypatch)
    ctx = r.ctx()
    monkeypatch.setattr(ax25.AX25Bank, "_calls", ax25.AX25Bank._calls + " channel_sttae")
    with pytest.raises(AttributeError, match="sdrhip_ax25_channel_sttae"):
        ax25.AX25Bank(ctx, 1, 64)
