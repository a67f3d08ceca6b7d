"""GPU parity of the channel group (include/sdrhip_changroup.h): ONE launch over several handles of the channelizer family must
leave every member's outputs and state BIT FOR BIT as the member's own call would. Every member has a TWIN: a second handle
created with the same arguments and given the same calls one by one (its process() runs in the red-zoned arena by this module's
name, i.e. through its own process_dev). After every group call the members' rows, counts and get_state — for the power monitor
also sums, levels(), occupied() and calls — are compared with the twins' as bit patterns.

The group's own device buffers are this module's (Guarded): filled with a pattern, a margin before and behind, row strides above
the output count; after every call the margins, the row padding and the whole input are checked.

  1  group == members alone: node type x input type, three members of different shapes (one group holds M = 4096 beside M = 8:
     the largest LDS with the smallest member; there the M = 8 member's stream is (T + 1) D samples, so in the last call it has ONE
     tile where grid.x is 3), a selection that is not the identity, mixed FM / AM / USB modes and non-unit gains, four calls with
     per-member lengths 0, D - 1, D + 1 and the rest;
  1b members of 1, 4 and 3 tiles in one launch of the small shapes: workgroups at and beyond a member's tile count, for every row
     kernel;  1c the staged process(xs) against the twins' process(x);
  2  group calls interleaved with a member's own call, set_channels and set_mode;  3  two members on one input pointer;
  4  all members' rows back to back in one buffer;  5  the power monitor under different SDRHIP_CHANPOWER_GRID values (a member's
  stride differs from grid.x), flags that open and close, sums asked for or not, a skipped finish step;  6  refusals change nothing.
The inputs are the existing parity tests' (their _taps / _signal helpers, (3 T + 1) D samples per member unless a test says
otherwise). Rig.call records every member's tile count of the call (`tiles`), so a test can assert that they differed."""
import numpy as np
import pytest

import test_gpu_parity_channelizer as PC

pytestmark = pytest.mark.gpu

FAMILIES = ["channelizer", "audio", "power"]
ITYPES = ["cs16", "cf32", "s16", "f32"]           # complex int16 / float rows, real int16 / float rows
SMALL = [(8, 3, 21), (12, 6, 30), (64, 32, 64)]
MIXED = [(4096, 2048, 4097), (8, 3, 21), (182, 77, 500)]
PAD, MARGIN, ALPHA = 5, 512, 0.375
FM, AM, USB = 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    import libsdr_amd as sa
    c = sa.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def same(a, b):
    return bits(a) == bits(b)


def _real(itype):
    return itype in ("s16", "f32")


def _np(itype):
    return np.int16 if itype in ("cs16", "s16") else np.float32


def _stream(itype, shape, seed=0, tiles=3):
    """(3 T + 1) D samples of the existing parity tests' signal; a real row is its first component"""
    M, D, n_taps = shape
    n = (tiles * PC.tile_times(M) + 1) * D
    x = PC._signal("cs16" if _np(itype) is np.int16 else "cf32", n, 17 * M + D + n_taps + seed)
    return np.ascontiguousarray(x[:, 0]) if _real(itype) else x


def _selection(K):
    """not the identity: a subset, out of order"""
    return [k for k in (K - 1, 0, K // 2, 1) if 0 <= k < K][:min(K, 4)] if K > 2 else [K - 1, 0]


def _node(ctx, family, itype, shape, max_in, sel=None):
    import libsdr_amd as sa
    M, D, n_taps = shape
    real = _real(itype)
    K = M // 2 + 1 if real else M
    taps = PC._taps(M, n_taps)
    if family == "channelizer":
        return sa.Channelizer(ctx, _np(itype), M, D, taps, channels=sel, max_in=max_in, real=real)
    if family == "audio":
        modes = [(FM, AM, USB)[k % 3] for k in range(K)]
        scale = 1.0 if _np(itype) is np.int16 else 8000.0          # (float rows are of order 1)
        gains = [scale * (0.5 + 0.25 * (k % 5)) for k in range(K)]
        return sa.AudioChannelizer(ctx, _np(itype), M, D, taps, modes=modes, gains=gains, channels=sel, max_in=max_in, real=real)
    return sa.ChannelPower(ctx, _np(itype), M, D, taps, alpha=ALPHA, max_in=max_in, real=real)


def same_state(a, b):
    sa_, sb = a.get_state(), b.get_state()
    assert sorted(sa_) == sorted(sb)
    for k in sa_:
        if isinstance(sa_[k], np.ndarray):
            assert same(sa_[k], sb[k]), k
        else:
            assert sa_[k] == sb[k], (k, sa_[k], sb[k])
    if hasattr(a, "levels"):
        (la, fa), (lb, fb) = a.levels(), b.levels()
        assert same(la, lb) and np.array_equal(fa, fb) and a.occupied() == b.occupied()
    return sa_


class Guarded:
    """a device buffer with a margin before and behind, all of it a pattern; `shadow` is what it should hold"""

    def __init__(self, ctx, nbytes, pat):
        self.ctx, self.n, self.pat = ctx, int(nbytes), pat
        self.base = ctx.malloc(self.n + 2 * MARGIN)
        self.ptr = self.base + MARGIN
        self.fill()

    def fill(self):
        self.shadow = np.full(self.n + 2 * MARGIN, self.pat, np.uint8)
        self.ctx.h2d(self.base, self.shadow)

    def put(self, arr, at=0):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert at + b.size <= self.n
        if b.size:
            self.shadow[MARGIN + at:MARGIN + at + b.size] = b
            self.ctx.h2d(self.ptr + at, b)

    def check(self, spans=()):
        """everything outside the spans (offset, bytes) is what it was -> the bytes between the margins"""
        got = np.empty_like(self.shadow)
        self.ctx.d2h(got, self.base)
        keep = np.ones(got.size, bool)
        for at, nb in spans:
            assert 0 <= at and at + nb <= self.n, (at, nb, self.n)
            keep[MARGIN + at:MARGIN + at + nb] = False
        bad = np.flatnonzero(got[keep] != self.shadow[keep])
        assert bad.size == 0, "%d bytes outside the call's rows changed (first at %d of %d)" % (bad.size, bad[0], got.size)
        return got[MARGIN:MARGIN + self.n]

    def free(self):
        self.ctx.free(self.base)


class Rig:
    """members, twins, the group and the group's device buffers. shared_input: every member reads ONE device pointer (and one
    stream); packed: every member's rows lie behind one another in ONE buffer."""

    def __init__(self, ctx, family, itype, shapes, sels=None, shared_input=False, packed=False, sums=None, make=None, tiles=3):
        import libsdr_amd as sa
        self.ctx, self.family, self.itype, self.shapes = ctx, family, itype, shapes
        self.power = family == "power"
        sels = sels or [None] * len(shapes)
        tiles = tiles if isinstance(tiles, (list, tuple)) else [tiles] * len(shapes)   # (tiles[i] T + 1) D samples for member i
        self.x = [_stream(itype, shapes[0] if shared_input else s, 0 if shared_input else i, tiles[i]) for i, s in enumerate(shapes)]
        if shared_input:
            n = min(len(_stream(itype, s)) for s in shapes)
            self.x = [self.x[0][:n]] * len(shapes)
        make = make or (lambda i, s, max_in: _node(ctx, family, itype, s, max_in, sels[i]))
        self.members = [make(i, s, len(self.x[i])) for i, s in enumerate(shapes)]
        self.twins = [make(i, s, len(self.x[i])) for i, s in enumerate(shapes)]
        self.off = [0] * len(shapes)
        self.group = sa.ChannelGroup(self.members)
        self.ob = 8 if family == "channelizer" else 2 if family == "audio" else 8
        eb = self.x[0].dtype.itemsize * (1 if _real(itype) else 2)
        self.eb = eb
        ins = [Guarded(ctx, len(self.x[0]) * eb, 0xA5)] * len(shapes) if shared_input else [Guarded(ctx, len(x) * eb, 0xA5) for x in self.x]
        self.ins = ins
        self.sums = sums if sums is not None else [True] * len(shapes)      # power: which members' sums are asked for
        caps = [m.n_channels * 8 if self.power else m.n_channels * (-(-len(x) // m.D) + PAD) * self.ob for m, x in zip(self.members, self.x)]
        if packed:
            one = Guarded(ctx, sum(caps), 0x5A)
            self.outs, self.at = [one] * len(shapes), [0] * len(shapes)     # (the offsets are the call's: back to back)
        else:
            self.outs, self.at = [Guarded(ctx, c, 0x5A) for c in caps], [0] * len(shapes)
        self.packed = packed

    def take(self, ns):
        parts = [x[o:o + n] for x, o, n in zip(self.x, self.off, ns)]
        self.off = [o + n for o, n in zip(self.off, ns)]
        return parts

    def call(self, ns):
        """one group call of ns[i] samples for member i, the twins' own calls, and every comparison"""
        parts = self.take(ns)
        for g in set(self.outs):
            g.fill()
        for g, p in zip(self.ins, parts):
            g.put(p)
        nos = [t.out_count(n) for t, n in zip(self.twins, ns)]
        # the workgroups with a tile of member i in this call (None: the member sits the call out); grid.x is their maximum
        self.tiles = [-(-no // PC.tile_times(s[0])) if n else None for no, n, s in zip(nos, ns, self.shapes)]
        if self.power:
            ptrs = [g.ptr if want else None for g, want in zip(self.outs, self.sums)]
            got = self.group.process_dev([g.ptr for g in self.ins], ns, ptrs)
        else:
            rows = [m.channels for m in self.members]
            strides = [no + PAD for no in nos]
            if self.packed:                                                 # member i + 1's first row begins where member i's last ends
                ext = [((r - 1) * s + no) * self.ob if n and no else 0 for r, s, no, n in zip(rows, strides, nos, ns)]
                self.at = [int(v) for v in np.cumsum([0] + ext)[:-1]]
            got = self.group.process_dev([g.ptr for g in self.ins], ns, [g.ptr + a for g, a in zip(self.outs, self.at)], strides)
        self.ctx.synchronize()
        assert got == [no if n else 0 for no, n in zip(nos, ns)], (got, nos)
        for g in set(self.ins):
            g.check()                                                       # margins and the input itself
        # the rows each member wrote, and nothing else
        spans = {}
        for i, (g, n, no) in enumerate(zip(self.outs, ns, nos)):
            spans.setdefault(g, [])
            if self.power:
                if n and self.sums[i]:
                    spans[g].append((0, self.members[i].n_channels * 8))
            elif n and no:
                spans[g] += [(self.at[i] + r * (no + PAD) * self.ob, no * self.ob) for r in range(self.members[i].channels)]
        inner = {g: g.check(s) for g, s in spans.items()}
        for i, (m, t, p, n, no) in enumerate(zip(self.members, self.twins, parts, ns, nos)):
            if self.power:
                if n and self.sums[i]:
                    want = t.process(p)
                    assert same(inner[self.outs[i]][:m.n_channels * 8].view(np.float64), want), i
                elif n:
                    self.twin_quiet(t, p)
            else:
                want = t.process(p)
                if n and no:
                    raw = inner[self.outs[i]][self.at[i]:self.at[i] + m.channels * (no + PAD) * self.ob]
                    if self.family == "channelizer":
                        rows_ = raw.view(np.float32).reshape(m.channels, no + PAD, 2)[:, :no]
                    else:
                        rows_ = raw.view(np.int16).reshape(m.channels, no + PAD)[:, :no]
                    assert same(rows_, want), (i, n, no)
            same_state(m, t)

    def twin_quiet(self, t, p):
        """the twin's own call with a NULL sum (its finish step is skipped where the call completes no output)"""
        d = self.ctx.malloc(max(p.nbytes, 16))
        try:
            self.ctx.h2d(d, p)
            t.process_dev(d, len(p), None)
            self.ctx.synchronize()
        finally:
            self.ctx.free(d)

    def own(self, i, n):
        """member i's own call beside the same call of its twin: the rows agree, and so does the state"""
        p = self.take([n if k == i else 0 for k in range(len(self.members))])[i]
        assert same(self.members[i].process(p), self.twins[i].process(p))
        same_state(self.members[i], self.twins[i])

    def both(self, i, f):
        f(self.members[i])
        f(self.twins[i])

    def rest(self):
        return [len(x) - o for x, o in zip(self.x, self.off)]

    def close(self):
        self.group.close()
        for o in self.members + self.twins:
            o.close()
        for g in set(self.ins) | set(self.outs):
            g.free()


def _four_calls(shapes):
    """per-member lengths of four group calls: 0, D - 1 (emits nothing) and D + 1 in an order of the member's own, then the rest"""
    heads = [[0, D - 1, D + 1][-i % 3:] + [0, D - 1, D + 1][:-i % 3] for i, (_, D, _) in enumerate(shapes)]
    return [[h[c] for h in heads] for c in range(3)]


def _kernel(family, itype):
    fam = {"channelizer": "channelizer", "audio": "chanaudio", "power": "chanpower"}[family]
    names = ["group_%s_%s%s_kernel" % (fam, "real_" if _real(itype) else "", itype)]
    return names + (["group_chanpower_finish_kernel"] if family == "power" else [])


@pytest.mark.parametrize("shapes", [SMALL, MIXED], ids=["small", "4096-beside-8"])
@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_group_equals_members_alone(ctx, family, itype, shapes):
    from redzone import RedZone
    K = [M // 2 + 1 if _real(itype) else M for M, _, _ in shapes]
    sels = None if family == "power" else [None, _selection(K[1]), None]
    before = RedZone.calls
    rig = Rig(ctx, family, itype, shapes, sels, sums=[True, False, True], tiles=[3, 1, 3] if shapes is MIXED else 3)
    try:
        assert rig.group.kernel_names == _kernel(family, itype)
        info = rig.group.plan_info()
        lds = [m.plan_info()["lds_bytes"] for m in rig.members]
        tiles = [-(-(-(-len(x) // D)) // PC.tile_times(M)) for x, (M, D, _) in zip(rig.x, shapes)]
        assert info == {"members": 3, "grid_x": max(tiles), "lds_bytes": max(lds)}, (info, tiles, lds)
        if shapes is MIXED and not _real(itype):
            assert max(lds) > 64 * 1024 and min(lds) < 32 * 1024 and max(tiles) == 4
        for ns in _four_calls(shapes):
            rig.call(ns)
        assert all(o == 2 * D for o, (_, D, _) in zip(rig.off, shapes))
        rig.call(rig.rest())
        assert rig.tiles == ([3, 1, 3] if shapes is MIXED else [3, 3, 3])   # (MIXED: grid.x = 3, the M = 8 member has one tile)
        for m, x in zip(rig.members, rig.x):
            assert m.get_state()["consumed"] == len(x)
        assert RedZone.calls > before                                       # (the twins ran in the arena)
    finally:
        rig.close()


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("family", ["channelizer", "audio"])
def test_members_with_fewer_tiles_than_the_launch(ctx, family, itype):
    """One launch in which the members have 1, 4 and 3 tiles: grid.x is 4, so member 0's row of the grid has three workgroups and
    member 2's one that find no tile and only roll their share of the tail (audio: block 0 alone copies `last`, the workgroup with
    the last output writes the FM angles). Then a launch of 3, (absent), 1 tiles."""
    shapes = SMALL
    K = [M // 2 + 1 if _real(itype) else M for M, _, _ in shapes]
    rig = Rig(ctx, family, itype, shapes, [None, _selection(K[1]), None])
    try:
        T, D = [PC.tile_times(s[0]) for s in shapes], [s[1] for s in shapes]
        rig.call([100 * D[0] + 1, len(rig.x[1]), (2 * T[2] + 2) * D[2] + 5])
        assert rig.tiles == [1, 4, 3]
        rig.call([(2 * T[0] + 7) * D[0], 0, 9 * D[2]])
        assert rig.tiles == [3, None, 1]
        rig.call(rig.rest())
    finally:
        rig.close()


@pytest.mark.parametrize("family,itype", [("channelizer", "cs16"), ("audio", "f32"), ("power", "cf32"), ("power", "s16")])
def test_the_staged_process_returns_what_the_members_own_process_would(ctx, family, itype):
    """ChannelGroup.process(xs) through the group's own device rows against the twins' process(x): a member at n = 0, one at
    n < D (no output), rows of different lengths; then the rest, which regrows the staged rows."""
    shapes = SMALL
    rig = Rig(ctx, family, itype, shapes, None if family == "power" else [None, [3, 0], None])
    try:
        D = [s[1] for s in shapes]
        for ns in ([0, D[1] - 1, 5 * D[2] + 3], [7 * D[0], 40 * D[1] + 1, 0], rig.rest):
            parts = rig.take(ns() if callable(ns) else ns)
            got = rig.group.process(parts)
            want = [t.process(p) for t, p in zip(rig.twins, parts)]
            assert len(got) == 3
            for i, (g, w) in enumerate(zip(got, want)):
                assert same(g, w), (i, g.shape, w.shape)
            for m, t in zip(rig.members, rig.twins):
                same_state(m, t)
        assert any(w.any() for w in want)
    finally:
        rig.close()


@pytest.mark.parametrize("family,itype", [("channelizer", "cs16"), ("audio", "cf32"), ("audio", "s16")])
def test_group_calls_interleaved_with_members_own_calls_and_setters(ctx, family, itype):
    shapes = SMALL
    rig = Rig(ctx, family, itype, shapes, [None, [5, 0, 3], None])
    try:
        D = [s[1] for s in shapes]
        rig.call([5 * D[0] + 1, 7 * D[1], 3 * D[2] + 2])
        rig.own(0, 4 * D[0] + 3)                                            # member 0's own process_dev between two group calls
        rig.both(1, lambda v: v.set_channels([1, 4]))
        if family == "audio":
            rig.both(2, lambda v: v.set_mode(0, AM))                        # an FM row becomes AM
            rig.both(2, lambda v: v.set_mode(1, FM))
            rig.both(0, lambda v: v.set_gain(2, 0.75))
        rig.call([2 * D[0], 9 * D[1] + 1, 4 * D[2]])
        rig.both(1, lambda v: v.set_channels(None))
        rig.own(1, D[1] + 1)
        rig.call(rig.rest())
    finally:
        rig.close()


@pytest.mark.parametrize("family,itype", [("channelizer", "s16"), ("audio", "cs16"), ("power", "cf32")])
def test_two_members_read_one_input_pointer(ctx, family, itype):
    """one antenna on two grids"""
    shapes = [(64, 32, 64), (12, 6, 30)]
    rig = Rig(ctx, family, itype, shapes, shared_input=True)
    try:
        assert rig.ins[0] is rig.ins[1]
        n = len(rig.x[0])
        for k in (97, 1, n // 2):
            rig.call([k, k])
        rig.call(rig.rest())
    finally:
        rig.close()


@pytest.mark.parametrize("family,itype", [("channelizer", "cf32"), ("audio", "f32")])
def test_rows_of_all_members_back_to_back_in_one_buffer(ctx, family, itype):
    rig = Rig(ctx, family, itype, SMALL, [None, [2, 6, 1], None], packed=True)
    try:
        D = [s[1] for s in SMALL]
        rig.call([6 * D[0], 5 * D[1], 9 * D[2]])
        assert rig.at[1] > 0 and rig.at[2] > rig.at[1]
        rig.call(rig.rest())
    finally:
        rig.close()


@pytest.mark.parametrize("itype", ["cs16", "f32"])
def test_power_members_under_different_grids(ctx, itype, monkeypatch):
    """member 0 walks four tiles with 3 workgroups, member 1 has a single tile, member 2 walks four tiles with 1 workgroup: the
    launch's grid.x is 3 and no member's stride but member 0's is. The flags all open (thresholds 0), all close (infinite), then
    follow thresholds at the median level. Member 1's sums are never asked for, and its first call completes no output: its
    finish step is skipped."""
    shapes = [(64, 32, 64), (8, 3, 21), (12, 6, 30)]
    grids = ["3", None, "1"]

    def make(i, s, max_in):
        if grids[i]:
            monkeypatch.setenv("SDRHIP_CHANPOWER_GRID", grids[i])
        else:
            monkeypatch.delenv("SDRHIP_CHANPOWER_GRID", raising=False)
        node = _node(ctx, "power", itype, s, max_in)
        monkeypatch.delenv("SDRHIP_CHANPOWER_GRID", raising=False)
        return node

    rig = Rig(ctx, "power", itype, shapes, sums=[True, False, True], make=make, tiles=5)
    try:
        assert [m.plan_info()["grid"] for m in rig.members] == [3, 6, 1] and rig.group.plan_info()["grid_x"] == 6
        T = [PC.tile_times(s[0]) for s in shapes]
        D = [s[1] for s in shapes]
        everyone = lambda f: [rig.both(i, f) for i in range(3)]
        everyone(lambda v: v.set_thresholds(0.0, 0.0))
        rig.call([3 * D[0] + 1, D[1] - 1, 2 * D[2]])                         # (member 1: no output, no sums)
        assert rig.twins[1].get_state()["calls"] == 0
        assert all(t.levels()[1].all() for t in (rig.twins[0], rig.twins[2]))
        everyone(lambda v: v.set_thresholds(np.inf, np.inf))
        rig.call([4 * T[0] * D[0], 10 * D[1] + 1, 4 * T[2] * D[2]])           # four tiles, four tiles, one tile: grid.x = 3
        assert not any(t.levels()[1].any() for t in rig.twins)
        for i in range(3):
            thr = float(np.median(rig.twins[i].levels()[0]))
            rig.both(i, lambda v: v.set_thresholds(thr, 0.5 * thr))
        rig.call([2 * D[0], 0, 5 * D[2]])                                    # (member 1 is left out of the launch)
        assert all(t.levels()[1].any() for t in (rig.twins[0], rig.twins[2])) and not rig.twins[1].levels()[1].any()
        assert [t.get_state()["calls"] for t in rig.twins] == [3, 1, 3]
    finally:
        rig.close()


def _refused(call, code, text):
    import libsdr_amd as sa
    with pytest.raises(sa.SdrHipError) as e:
        call()
    assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))


@pytest.mark.parametrize("family", ["channelizer", "audio"])
def test_refused_row_calls_change_nothing(ctx, family):
    import libsdr_amd as sa
    from libsdr_amd import abi
    shapes = SMALL
    rig = Rig(ctx, family, "cs16", shapes)
    try:
        D = [s[1] for s in shapes]
        rig.call([4 * D[0], 4 * D[1], 4 * D[2]])
        states = [same_state(m, t) for m, t in zip(rig.members, rig.twins)]
        for g in rig.outs:
            g.fill()
        ins, outs = [g.ptr for g in rig.ins], [g.ptr for g in rig.outs]
        ns = [4 * D[0], 4 * D[1], 4 * D[2]]
        ob, eb = rig.ob, rig.eb
        G = rig.group
        cases = [
            (lambda: G.process_dev(ins, [ns[0], len(rig.x[1]) + 1, ns[2]], outs, [0, 0, 0]), abi.E_SIZE, "max_in"),
            (lambda: G.process_dev(ins, ns, outs, [0, 3, 0]), abi.E_SIZE, "out_stride 3 < outputs 4"),
            (lambda: G.process_dev(ins, ns, [outs[0], outs[0] + 8 * ob, outs[2]], [0, 0, 0]), abi.E_INVALID,
             "the output range of member 0 overlaps the output range of member 1"),
            (lambda: G.process_dev(ins, ns, [outs[0], outs[1], ins[0] + 2 * eb], [0, 0, 0]), abi.E_INVALID,
             "the output range of member 2 overlaps the input range of member 0"),
            (lambda: G.process_dev(ins, ns, [outs[0], ins[1], outs[2]], [0, 0, 0]), abi.E_INVALID, "overlaps the input range"),
            (lambda: G.process_dev(ins, ns, [outs[0], None, outs[2]], [0, 0, 0]), abi.E_INVALID, "NULL buffer"),
            (lambda: sa.abi.check(G._c_power_process_dev(G._h, G._pointers(ins), G._counts(ns), None, None)), abi.E_INVALID, "not a power group"),
        ]
        for call, code, text in cases:
            _refused(call, code, text)
            self_states = [same_state(m, t) for m, t in zip(rig.members, rig.twins)]
            for a, b in zip(states, self_states):
                assert a["consumed"] == b["consumed"] and same(a["tail"], b["tail"])
            for g in rig.ins + rig.outs:
                g.check()
        rig.call(ns)                                                        # the next correct call is the twins'
        rig.call(rig.rest())
    finally:
        rig.close()


def test_refused_power_calls_and_refused_groups_change_nothing(ctx):
    import libsdr_amd as sa
    from libsdr_amd import abi
    shapes = [(12, 6, 30), (8, 3, 21)]
    rig = Rig(ctx, "power", "cs16", shapes)
    other = sa.Context(0)
    strangers = []
    try:
        D = [s[1] for s in shapes]
        rig.call([4 * D[0], 4 * D[1]])
        states = [same_state(m, t) for m, t in zip(rig.members, rig.twins)]
        for g in rig.outs:
            g.fill()
        ins, sums, ns = [g.ptr for g in rig.ins], [g.ptr for g in rig.outs], [4 * D[0], 4 * D[1]]
        G = rig.group
        cases = [
            (lambda: G.process_dev(ins, [ns[0], len(rig.x[1]) + 1], sums), abi.E_SIZE, "max_in"),
            (lambda: G.process_dev(ins, ns, [sums[0], sums[0] + 8]), abi.E_INVALID, "the output range of member 0 overlaps the output range of member 1"),
            (lambda: G.process_dev(ins, ns, [ins[1], sums[1]]), abi.E_INVALID, "the output range of member 0 overlaps the input range of member 1"),
            (lambda: G.process_dev([ins[0], None], ns, sums), abi.E_INVALID, "NULL buffer"),
            (lambda: sa.abi.check(G._c_process_dev(G._h, G._pointers(ins), G._counts(ns), G._pointers(sums), G._counts([0, 0]), None)),
             abi.E_INVALID, "a power group has no rows"),
        ]
        # groups that are refused: their members stay what they are
        a, b = rig.members
        cf = _node(ctx, "power", "cf32", shapes[0], 64)
        re = _node(ctx, "power", "s16", shapes[0], 64)
        far = _node(other, "power", "cs16", shapes[0], 64)
        plain = _node(ctx, "channelizer", "cs16", shapes[0], 64)
        strangers += [cf, re, far, plain]
        cases += [
            (lambda: sa.ChannelGroup([a, b, a]), abi.E_INVALID, "member 2 is member 0 again"),
            (lambda: sa.ChannelGroup([a, cf]), abi.E_INVALID, "member 1 has another input element type"),
            (lambda: sa.ChannelGroup([a, b, re]), abi.E_INVALID, "member 2 has another input element type"),
            (lambda: sa.ChannelGroup([a, far]), abi.E_INVALID, "member 1 is on another context"),
            (lambda: sa.ChannelGroup([a] * 9), abi.E_SIZE, "count 9 outside [1,8]"),
        ]
        for call, code, text in cases:
            _refused(call, code, text)
            now = [same_state(m, t) for m, t in zip(rig.members, rig.twins)]
            for p, q in zip(states, now):
                assert p["consumed"] == q["consumed"] and p["calls"] == q["calls"] and same(p["tail"], q["tail"])
            for g in rig.ins + rig.outs:
                g.check()
        with pytest.raises(TypeError):
            sa.ChannelGroup([a, plain])
        rig.call(ns)
        rig.call(rig.rest())
    finally:
        rig.close()
        for o in strangers:
            o.close()
        other.close()
