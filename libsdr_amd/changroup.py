"""numpy-facing wrapper over include/sdrhip_changroup.h (libsdr_amd.abi_changroup): the channel group — 1 to 8 nodes of ONE class
of the channelizer family (Channelizer, AudioChannelizer or ChannelPower; complex or real input) behind ONE launch whose second
grid dimension is the member. The group borrows its members: they stay the caller's nodes, with their own setters, state and
process calls, and must outlive the group. A group call leaves every member's outputs and state bit for bit as the member's
own process_dev would."""
import ctypes as C

import numpy as np

from . import abi_changroup
from .abi import check
from .abi_changroup import CHANGROUP_MAX
from .chanaudio import AudioChannelizer
from .channelizer import Channelizer
from .chanpower import ChannelPower
from .nodes import _Node, _text

__all__ = ["ChannelGroup", "CHANGROUP_MAX"]

_CREATE = ((AudioChannelizer, "audio"), (Channelizer, "channelizer"), (ChannelPower, "power"))   # (a subclass before its base)


def _array(ctype, values):
    return (ctype * len(values))(*values)


class ChannelGroup(_Node):
    """members: a list of 1 to 8 Channelizer, AudioChannelizer or ChannelPower nodes, all of one class, on one context and with
    one input element type; they may differ in M, D, taps and selection. process_dev(ins, ns, outs, strides) — for a power
    group process_dev(ins, ns, sums=None) — takes one device pointer and one count per member and returns the members' output
    counts; process(xs) takes one host row per member and returns what each member's own process would."""
    _prefix = "sdrhip_changroup"
    _calls = "process_dev power_process_dev plan_info kernel_names"

    def __init__(self, members):
        abi_changroup.lib()
        super().__init__()
        self.members = list(members)
        assert self.members, "a group has at least one member"
        kind = [name for cls, name in _CREATE if isinstance(self.members[0], cls)]
        if not kind or any(type(m) is not type(self.members[0]) for m in self.members):
            raise TypeError("the members of a group are Channelizer, AudioChannelizer or ChannelPower nodes, all of one class: %s"
                            % [type(m).__name__ for m in self.members])
        self.power = kind[0] == "power"
        self.ctx = self.members[0].ctx
        self._stage = {}   # member index -> [in pointer, in bytes, out pointer, out bytes]: process()'s device rows
        create = getattr(abi_changroup.lib(), "sdrhip_changroup_%s_create" % kind[0])
        check(create(_array(C.c_void_p, [m._h.value for m in self.members]), len(self.members), C.byref(self._h)))

    def _counts(self, values):
        assert len(values) == len(self.members), (len(values), len(self.members))
        return _array(C.c_size_t, [int(v) for v in values])

    def _pointers(self, values):
        assert len(values) == len(self.members), (len(values), len(self.members))
        return _array(C.c_void_p, [int(v) if v else None for v in values])

    def process_dev(self, ins, ns, outs=None, strides=None):
        """Device pointers, one per member; strides in output elements (0: the call's count). A power group takes
        (ins, ns, sums): sums None, or a list whose entries may be None. One launch (a power group: two), nothing is
        synchronised -> the outputs per row of every member."""
        got = self._counts([0] * len(self.members))
        if self.power:
            assert strides is None
            check(self._c_power_process_dev(self._h, self._pointers(ins), self._counts(ns), None if outs is None else self._pointers(outs), got))
        else:
            check(self._c_process_dev(self._h, self._pointers(ins), self._counts(ns), self._pointers(outs), self._counts(strides), got))
        return [int(v) for v in got]

    def _staged(self, i, in_bytes, out_bytes):
        """member i's device rows of at least these sizes (they only grow)"""
        s = self._stage.setdefault(i, [None, 0, None, 0])
        for k, want in ((0, in_bytes), (2, out_bytes)):
            if s[k + 1] < want:
                if s[k]:
                    self.ctx.free(s[k])
                s[k], s[k + 1] = self.ctx.malloc(want), want
        return s[0], s[2]

    def process(self, xs):
        """xs: one host row per member, as the member's own process takes it -> the list of what each member's own process
        would return. The rows are staged through device buffers the group owns."""
        assert len(xs) == len(self.members), (len(xs), len(self.members))
        rows = [m._rows(x)[0] for m, x in zip(self.members, xs)]
        ns = [int(r.shape[0]) for r in rows]
        nos = [m.out_count(n) for m, n in zip(self.members, ns)]
        outs = [np.zeros((1, m.n_channels), np.float64) if self.power else m._zeros(no) for m, no in zip(self.members, nos)]
        ins, dev = [], []
        for i, (r, o) in enumerate(zip(rows, outs)):
            a, b = self._staged(i, max(r.nbytes, 16), max(o.nbytes, 16))
            if r.nbytes:
                self.ctx.h2d(a, r)
            ins.append(a)
            dev.append(b)
        got = self.process_dev(ins, ns, dev) if self.power else self.process_dev(ins, ns, dev, nos)
        assert got == nos, (got, nos)
        for n, o, b in zip(ns, outs, dev):
            if n and o.size:
                self.ctx.d2h(o, b)
        return [o[0] if self.power else o for o in outs]

    def plan_info(self):
        """{members, grid_x, lds_bytes} of a launch (sdrhip_changroup_plan_info)"""
        v = [C.c_int(0) for _ in range(3)]
        check(self._c_plan_info(self._h, *[C.byref(c) for c in v]))
        return dict(zip(("members", "grid_x", "lds_bytes"), [c.value for c in v]))

    @property
    def kernel_names(self):
        return _text(self._c_kernel_names, self._h, size=256).split(",")

    def _release(self):
        """the group's own rows and the group; the members stay"""
        for s in self._stage.values():
            for p in (s[0], s[2]):
                if p:
                    self.ctx.free(p)
        self._stage = {}
        super()._release()
