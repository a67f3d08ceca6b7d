"""The channel group's C calls (include/sdrhip_changroup.h), what can be checked without a GPU: every function of the header is
exported by libsdrhip.so and has a prototype in libsdr_amd/abi_changroup.py, and nothing else named sdrhip_changroup* is exported;
the header is registered in abi.LATER_SIDE_HEADERS only and its names are disjoint from every other table's; the create calls'
NULL and count rules answer before anything is dereferenced, and every other entry point refuses a NULL handle; the thirteen
group kernels exist for gfx950 and use no scratch (the member pick by blockIdx.y stays in scalar registers); and the Python
wrapper, driven against tests/test_nodes_calls.py's fake library, makes the calls it should."""
import ctypes as C

import numpy as np
import pytest

from abi_checks import assert_header_binding, kernel_scratch, last_error
from libsdr_amd import abi, nodes
from test_nodes_calls import FakeLib, NAMES, Run, count, ramp

NEW = ["sdrhip_changroup_audio_create", "sdrhip_changroup_channelizer_create", "sdrhip_changroup_destroy",
       "sdrhip_changroup_kernel_names", "sdrhip_changroup_plan_info", "sdrhip_changroup_power_create",
       "sdrhip_changroup_power_process_dev", "sdrhip_changroup_process_dev"]
CREATES = ["sdrhip_changroup_channelizer_create", "sdrhip_changroup_audio_create", "sdrhip_changroup_power_create"]


def test_header_binding_and_exports_agree():
    from libsdr_amd import abi_changroup
    assert_header_binding(abi_changroup, NEW, r"\b(sdrhip_changroup[a-z0-9_]*)\b")


def test_the_header_is_in_the_second_table_only():
    import libsdr_amd  # noqa: F401   (the package imports every side header's module)
    from libsdr_amd import abi_changroup
    assert "sdrhip_changroup.h" in abi.LATER_SIDE_HEADERS and "sdrhip_changroup.h" not in abi.SIDE_HEADERS
    assert abi.LATER_SIDE_HEADERS["sdrhip_changroup.h"].SIGNATURES is abi_changroup.SIGNATURES
    assert not set(abi_changroup.SIGNATURES) & set(abi.SIGNATURES)
    for name, side in list(abi.SIDE_HEADERS.items()) + list(abi.LATER_SIDE_HEADERS.items()):
        if name != "sdrhip_changroup.h":
            assert not set(abi_changroup.SIGNATURES) & set(side.SIGNATURES), name
    assert sorted(abi.lib()._declared) == abi.header_functions()
    assert abi.LATER_SIDE_HEADERS["sdrhip_changroup.h"].header_functions() == sorted(NEW)


def test_the_package_exports_the_class():
    import libsdr_amd
    from libsdr_amd import abi_changroup, changroup
    assert libsdr_amd.ChannelGroup is changroup.ChannelGroup and abi_changroup.CHANGROUP_MAX == 8
    with open(abi_changroup.HEADER) as f:
        assert "#define SDRHIP_CHANGROUP_MAX 8" in f.read()


@pytest.mark.parametrize("create", CREATES)
def test_create_rules_that_need_no_context(create):
    """NULL out / members, then count — before any member is looked at: the member arrays here hold wild pointers — then a NULL
    member, by its index"""
    from libsdr_amd import abi_changroup
    fn = getattr(abi_changroup.lib(), create)
    wild = (C.c_void_p * 9)(*[0xDEAD0000 + 64 * k for k in range(9)])
    out = C.c_void_p(0x1)
    assert fn(wild, 2, None) == abi.E_INVALID and "NULL" in last_error()
    assert fn(None, 2, C.byref(out)) == abi.E_INVALID and "NULL" in last_error() and out.value is None
    for bad in (0, -1, 9, 1 << 20):
        out = C.c_void_p(0x1)
        assert fn(wild, bad, C.byref(out)) == abi.E_SIZE and out.value is None
        assert "count %d outside [1,8]" % bad in last_error(), last_error()
    assert fn(None, 0, C.byref(out)) == abi.E_INVALID                      # in the header's order
    # (the NULL and the duplicate rule compare pointers only, so wild ones beside them are safe here)
    for at in range(3):
        out = C.c_void_p(0x1)
        some = (C.c_void_p * 3)(*[None if k == at else 0xDEAD0000 + 64 * k for k in range(3)])
        assert fn(some, 3, C.byref(out)) == abi.E_INVALID and "member %d is NULL" % at in last_error() and out.value is None
    twice = (C.c_void_p * 3)(0xDEAD0000, 0xDEAD0040, 0xDEAD0000)
    assert fn(twice, 3, C.byref(out)) == abi.E_INVALID and "member 2 is member 0 again" in last_error() and out.value is None
    assert fn((C.c_void_p * 2)(0xDEAD0000, None), 2, C.byref(out)) == abi.E_INVALID and "member 1 is NULL" in last_error()   # NULL first


def test_calls_on_a_null_handle():
    from libsdr_amd import abi_changroup
    L = abi_changroup.lib()
    p, n, t, buf = (C.c_void_p * 2)(), (C.c_size_t * 2)(5, 5), C.c_int(7), C.create_string_buffer(64)
    got = (C.c_size_t * 2)(9, 9)
    for call in (lambda: L.sdrhip_changroup_process_dev(None, p, n, p, n, got),
                 lambda: L.sdrhip_changroup_power_process_dev(None, p, n, None, got),
                 lambda: L.sdrhip_changroup_plan_info(None, C.byref(t), None, None),
                 lambda: L.sdrhip_changroup_kernel_names(None, buf, 64)):
        assert call() == abi.E_INVALID and "NULL" in last_error()
    assert list(got) == [9, 9] and t.value == 7
    assert L.sdrhip_changroup_destroy(None) == abi.OK


def test_the_thirteen_kernels_exist_for_gfx950_without_scratch(tmp_path):
    seen = kernel_scratch(tmp_path, r"\d(group_chan[a-z0-9_]+_kernel)")
    want = ["group_%s%s_%s_kernel" % (family, real, t) for family in ("channelizer", "chanaudio", "chanpower")
            for real, types in (("", ("cs16", "cf32")), ("_real", ("s16", "f32"))) for t in types] + ["group_chanpower_finish_kernel"]
    assert len(want) == 13 and seen == {k: 0 for k in want}, seen


# ---- the wrapper against the fake library ---------------------------------------------------------------------------------
def _plan_info(args):
    for a, v in zip(args[1:], (3, 13, 66560)):
        a._obj.value = v


def _process_dev(args):
    """the fake's counts: count(n) per member, written into the call's last array"""
    for k in range(len(args[2])):
        args[-1][k] = count(args[2][k])


def _run(monkeypatch):
    from libsdr_amd import abi_chanaudio, abi_changroup, abi_channelizer, abi_chanpower
    sigs = dict(abi.SIGNATURES)
    for m in (abi_channelizer, abi_chanaudio, abi_chanpower, abi_changroup):
        sigs.update(m.SIGNATURES)
    answers = {"sdrhip_changroup_plan_info": _plan_info, "sdrhip_changroup_process_dev": _process_dev,
               "sdrhip_changroup_power_process_dev": _process_dev}
    return Run(monkeypatch, FakeLib(signatures=sigs, answers=answers), hook=False)


def _calls(r, name):
    return [c[1:] for c in r.fake.calls if c[0] == name]


def test_wrapper_calls_against_the_fake_library(monkeypatch):
    import libsdr_amd as sa
    r = _run(monkeypatch)
    ctx = r.ctx()
    taps = np.linspace(0.0, 1.0, 21)
    a, b, c = (sa.Channelizer(ctx, np.int16, M, D, taps, max_in=64) for M, D in ((8, 4), (12, 6), (8, 3)))
    g = sa.ChannelGroup([a, b, c])
    assert not g.power and g.members == [a, b, c] and g.ctx is ctx
    assert g.kernel_names == NAMES and g.plan_info() == {"members": 3, "grid_x": 13, "lds_bytes": 66560}
    # create: (the members' handles, count, out)
    assert _calls(r, "sdrhip_changroup_channelizer_create") == [(("c_void_p", [r.h(a), r.h(b), r.h(c)]), 3, ("out", "c_void_p"))]
    # the row call: every array has `count` entries
    assert g.process_dev([0x1000, 0x2000, 0x1000], [16, 0, 24], [0x5000, 0x6000, 0x7000], [0, 8, 9]) == [count(16), 0, count(24)]
    assert _calls(r, "sdrhip_changroup_process_dev") == [
        (r.h(g), ("c_void_p", [0x1000, 0x2000, 0x1000]), ("c_ulong", [16, 0, 24]), ("c_void_p", [0x5000, 0x6000, 0x7000]),
         ("c_ulong", [0, 8, 9]), ("c_ulong", [0, 0, 0]))]
    for bad in (lambda: g.process_dev([1, 2], [1, 2, 3], [1, 2, 3], [0, 0, 0]), lambda: g.process_dev([1, 2, 3], [1, 2], [1, 2, 3], [0, 0, 0]),
                lambda: g.process_dev([1, 2, 3], [1, 2, 3], [1, 2, 3, 4], [0, 0, 0]), lambda: g.process_dev([1, 2, 3], [1, 2, 3], [1, 2, 3], [0])):
        with pytest.raises(AssertionError):
            bad()
    assert len(_calls(r, "sdrhip_changroup_process_dev")) == 1
    # process(): one row per member through the group's own device rows, freed by close()
    before = r.fake.mallocs
    ys = g.process([ramp((16, 2), np.int16, 3), ramp((0, 2), np.int16, 0), ramp((24, 2), np.int16, 5)])
    assert [y.shape for y in ys] == [(8, count(16), 2), (12, 0, 2), (8, count(24), 2)] and all(y.dtype == np.float32 for y in ys)
    assert r.fake.mallocs - before == 6
    call = _calls(r, "sdrhip_changroup_process_dev")[1]
    assert call[2] == ("c_ulong", [16, 0, 24]) and call[4] == ("c_ulong", [count(16), 0, count(24)])
    assert len(set(call[1][1]) | set(call[3][1])) == 6                   # six device rows, none twice
    g.process([ramp((8, 2), np.int16, 3), ramp((0, 2), np.int16, 0), ramp((8, 2), np.int16, 3)])   # smaller rows: the buffers are kept
    assert r.fake.mallocs - before == 6
    g.close()
    g.close()
    assert len(_calls(r, "sdrhip_free")) == 6 and len(_calls(r, "sdrhip_changroup_destroy")) == 1
    assert not _calls(r, "sdrhip_channelizer_destroy")                   # the members are borrowed

    # the class check: all of one class, and a class of the family
    au = sa.AudioChannelizer(ctx, np.int16, 8, 4, taps, max_in=64)
    pw = sa.ChannelPower(ctx, np.int16, 8, 4, taps, max_in=64)
    for mixed in ([a, au], [au, a], [a, pw], [pw, au], [ctx], [a, None]):
        with pytest.raises(TypeError):
            sa.ChannelGroup(mixed)
    with pytest.raises(AssertionError):
        sa.ChannelGroup([])
    assert len(_calls(r, "sdrhip_changroup_channelizer_create")) == 1 and not _calls(r, "sdrhip_changroup_audio_create")

    ga = sa.ChannelGroup([au])
    assert not ga.power and _calls(r, "sdrhip_changroup_audio_create") == [(("c_void_p", [r.h(au)]), 1, ("out", "c_void_p"))]
    ys = ga.process([ramp((16, 2), np.int16, 3)])
    assert ys[0].shape == (8, count(16)) and ys[0].dtype == np.int16
    ga.close()

    # the power form: (ins, ns, sums), sums None or with None entries
    pw2 = sa.ChannelPower(ctx, np.int16, 12, 6, taps, max_in=64)
    gp = sa.ChannelGroup([pw, pw2])
    assert gp.power and _calls(r, "sdrhip_changroup_power_create") == [(("c_void_p", [r.h(pw), r.h(pw2)]), 2, ("out", "c_void_p"))]
    assert gp.process_dev([0x1000, 0x2000], [16, 8]) == [count(16), count(8)]
    assert gp.process_dev([0x1000, 0x2000], [16, 8], [None, 0x9000]) == [count(16), count(8)]
    assert _calls(r, "sdrhip_changroup_power_process_dev") == [
        (r.h(gp), ("c_void_p", [0x1000, 0x2000]), ("c_ulong", [16, 8]), None, ("c_ulong", [0, 0])),
        (r.h(gp), ("c_void_p", [0x1000, 0x2000]), ("c_ulong", [16, 8]), ("c_void_p", [None, 0x9000]), ("c_ulong", [0, 0]))]
    with pytest.raises(AssertionError):
        gp.process_dev([0x1000, 0x2000], [16, 8], [None, 0x9000], [0, 0])   # a power group has no strides
    sums = gp.process([ramp((16, 2), np.int16, 3), ramp((8, 2), np.int16, 4)])
    assert [s.shape for s in sums] == [(8,), (12,)] and all(s.dtype == np.float64 for s in sums)
    assert len(_calls(r, "sdrhip_changroup_process_dev")) == 4           # (the channelizer and audio groups' calls above)
    gp.close()
    from libsdr_amd import abi_changroup
    assert set(abi_changroup.SIGNATURES) <= r.fake.reached, sorted(set(abi_changroup.SIGNATURES) - r.fake.reached)
    for o in (a, b, c, au, pw, pw2, ctx):
        o.close()


def test_a_mistyped_entry_point_fails_construction(monkeypatch):
    import libsdr_amd as sa
    r = _run(monkeypatch)
    ctx = r.ctx()
    a = sa.Channelizer(ctx, np.int16, 8, 4, np.ones(8), max_in=64)
    monkeypatch.setattr(sa.ChannelGroup, "_calls", sa.ChannelGroup._calls + " plan_inf")
    with pytest.raises(AttributeError, match="sdrhip_changroup_plan_inf"):
        sa.ChannelGroup([a])
    a.close()
    ctx.close()
