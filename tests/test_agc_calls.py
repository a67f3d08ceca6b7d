"""CPU call trace of libsdr_amd.agc, in the manner of tests/test_nodes_calls.py and with its fake library, normal form and router:
AGC and AGCBank are driven against a fake that answers the names of abi.SIGNATURES and abi_agc.SIGNATURES only, checks every
argument against its declared argtype and records every call. The recorded list is compared with the table below, so a mistyped
entry point, a wrong argument count or type, a changed call order or a changed router decision shows here, without
libsdrhip.so and without a device."""
import numpy as np

from libsdr_amd import abi, abi_agc, agc
from test_nodes_calls import A, B, FakeLib, NAMES, OUT_VP, Run, XR16, ramp

OUT_F = ("out", "c_float")
XF = ramp((2, 16), np.float32, 31)
LAM = np.array([0.5, 0.25], np.float32)
Z16, ZF = ("<i2", (2, 16), "zeros"), ("<f4", (2, 16), "zeros")
E16 = ("<i2", (2, 0), "zeros")


def _plan_info(args):
    args[2]._obj.value, args[3]._obj.value = 256, 16


def _get_state(args):
    for a, v in zip(args[1:4], (2.0, 3.0, 1)):
        a._arr[...] = v


def _run(monkeypatch):
    """The fake of test_nodes_calls.py, answering include/sdrhip_agc.h's names as well."""
    return Run(monkeypatch, FakeLib(signatures=dict(abi.SIGNATURES, **abi_agc.SIGNATURES),
                                    answers={"sdrhip_agc_plan_info": _plan_info, "sdrhip_agc_get_state": _get_state}))


def case_agc(r):
    ctx = r.ctx()
    bank = agc.AGCBank(ctx, np.int16, LAM, target=[0.0, 9000.0], enabled=[True, False], max_in=64)
    r.ret("attrs", (bank.dtype, bank.channels, bank.max_in))
    r.ret("kernel_names", bank.kernel_names)
    r.ret("plan_info", (bank.plan_info(), bank.plan_info(16)))
    bank.process_dev(0x1000, 16, 19, 0x2000, 19)
    bank.set_channel(1, 0.125)
    bank.set_channel(0, 0.125, 500.0)
    bank.set_lambda(1, 0.75)
    bank.set_enabled(1, True)
    bank.set_gain(0, 2.5)
    r.ret("get_state", bank.get_state())
    bank.reset()
    r.three("process", bank, XR16, XR16[:, :0])
    one = agc.AGC(ctx, np.float32, 8000.0, tau=0.001, channels=2, max_in=64)
    r.ret("one/attrs", (one.dtype, one.channels, one.lam, one.target, one.tau))
    r.ret("one/process", one.process(XF))
    one.set_tau(0.5, c=1)
    one.set_tau(0.25)
    r.ret("lambda", agc.design_agc_lambda(0.1, 22050.0))
    for o in (bank, bank, one, ctx):
        o.close()


EXPECT = [
    ("sdrhip_ctx_create", 0, None, OUT_VP),
    ("sdrhip_design_agc_target", 0, OUT_F),                       # a target of 0: the type's default (the fake answers 7)
    ("sdrhip_agcbank_create", "h1", 0, B(LAM), B(np.array([7.0, 9000.0], np.float32)), B(np.array([1, 0], np.intc)), 2, 64, OUT_VP),
    ("ret", "attrs", (0, 2, 64)),
    ("sdrhip_agc_kernel_names", "h2", ("buf", 256), 256),
    ("ret", "kernel_names", NAMES),
    ("sdrhip_agc_plan_info", "h2", 64, ("out", "c_int"), ("out", "c_int")),   # 0: a call of max_in samples
    ("sdrhip_agc_plan_info", "h2", 16, ("out", "c_int"), ("out", "c_int")),
    ("ret", "plan_info", ({"tile_samples": 256, "channels_per_group": 16}, {"tile_samples": 256, "channels_per_group": 16})),
    ("sdrhip_agc_process_dev", "h2", 0x1000, 16, 19, 0x2000, 19),
    ("sdrhip_design_agc_target", 0, OUT_F),
    ("sdrhip_agc_set_channel", "h2", 1, 0.125, 7.0),
    ("sdrhip_agc_set_channel", "h2", 0, 0.125, 500.0),
    ("sdrhip_agc_set_lambda", "h2", 1, 0.75),
    ("sdrhip_agc_set_enabled", "h2", 1, 1),
    ("sdrhip_agc_set_gain", "h2", 0, 2.5),
    ("sdrhip_agc_get_state", "h2", ("<f4", (2,), "zeros"), ("<f4", (2,), "zeros"), ("<i4", (2,), "zeros"), 2),
    ("ret", "get_state", (A(np.full(2, 2.0, np.float32)), A(np.full(2, 3.0, np.float32)), A(np.ones(2, bool)))),
    ("sdrhip_agc_reset", "h2"),
    ("sdrhip_agc_process", "h2", A(XR16), 16, 16, Z16, 16),
    ("ret", "process", Z16),
    ("router", "h1", A(XR16), Z16),
    ("sdrhip_agc_process_dev", "h2", 0x1000, 16, 19, 0x2000, 19),
    ("ret", "process/routed", Z16),
    ("sdrhip_agc_process", "h2", E16, 0, 0, E16, 0),              # an empty call never meets the router
    ("ret", "process/empty", E16),
    ("sdrhip_design_agc_lambda", 0.001, 8000.0, OUT_F),
    ("sdrhip_design_agc_target", 1, OUT_F),
    ("sdrhip_agc_create", "h1", 1, 7.0, 7.0, 2, 64, OUT_VP),
    ("ret", "one/attrs", (1, 2, 7.0, 7.0, 0.001)),
    ("sdrhip_agc_process", "h3", A(XF), 16, 16, ZF, 16),
    ("ret", "one/process", ZF),
    ("sdrhip_design_agc_lambda", 0.5, 8000.0, OUT_F),
    ("sdrhip_agc_set_lambda", "h3", 1, 7.0),
    ("sdrhip_design_agc_lambda", 0.25, 8000.0, OUT_F),
    ("sdrhip_agc_set_lambda", "h3", 0, 7.0),
    ("sdrhip_agc_set_lambda", "h3", 1, 7.0),
    ("sdrhip_design_agc_lambda", 0.1, 22050.0, OUT_F),
    ("ret", "lambda", 7.0),
    ("sdrhip_agc_destroy", "h2"),
    ("sdrhip_agc_destroy", "h3"),
    ("hook", "h1"),
    ("sdrhip_ctx_destroy", "h1"),
]


def test_agc_call_trace(monkeypatch):
    r = _run(monkeypatch)
    case_agc(r)
    got = r.fake.calls
    for k, (g, w) in enumerate(zip(got, EXPECT)):
        assert g == w, (k, g, w)
    assert len(got) == len(EXPECT), got[len(EXPECT):]


def test_every_wrapper_call_of_the_header_was_reached(monkeypatch):
    r = _run(monkeypatch)
    case_agc(r)
    assert set(abi_agc.SIGNATURES) <= r.fake.reached, sorted(set(abi_agc.SIGNATURES) - r.fake.reached)


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    r = _run(monkeypatch)
    ctx = r.ctx()
    monkeypatch.setattr(agc.AGCBank, "_calls", agc.AGCBank._calls + " set_gian")
    try:
        agc.AGCBank(ctx, np.int16, LAM)
    except AttributeError as e:
        assert "sdrhip_agc_set_gian" in str(e)
    else:
        raise AssertionError("a misspelt entry point was bound")
