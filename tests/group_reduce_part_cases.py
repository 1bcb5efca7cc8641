"""Deterministic table of PARTIAL REDUCTION GROUPS (SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART; tests/test_group_reduce_part_host.py,
tests/test_gpu_group_reduce_part.py).

A row is a list of members, each a reduction that keeps dims of its own (any number, none or all included), built from the pieces of
tests/reduce_fuzz_cases.py like the table of tests/group_reduce_cases.py: every input is a window of a padded parent filled with NaN
(Bool and the integers: the value that would change the result), the data make every accumulation order give the same bits, and the
expected values are computed from the integers in exact arithmetic for 1, 2 and 3 applications.  The K destinations of a row are
windows (permuted, stepped, reversed), one behind the other, of ONE padded parent whose other elements hold random bits: that whole
parent is what the tests compare, byte for byte.  One f, one op, one kind of initop and one conj flag per operand position per row
(what a group shares); beta differs from member to member under `scale`.

Every member states the lanes per destination element TR and the workgroups W = ceil(nout / (256 / TR)) the planner must give it.
Nothing here imports torch."""
import numpy as np

import group_reduce_cases as GR
import reduce_fuzz_cases as RF
import strided_jl_amd as S
from reduce_exact_cases import Operand, _index, aligned_empty
from strided_jl_amd import _lib as L
from window_cases import finite_bits, layout

FORM_PART = 5                           # smr_group_layout
REDS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511)
DT = GR.DT


def lanes_small(red):
    """TR of a member with fewer than 65536 destination elements (include/strided_hip.h, PARTIAL REDUCTION GROUPS: the general form's
    rule): the largest power of two that is at most `red`, at most 256."""
    return min(256, 1 << (int(red).bit_length() - 1))


class Spec:
    """One member: dims in the caller's order, the reduced dims, per input (perm, lo, hi, steps, broadcast dims), the destination's
    (perm, lo, hi, steps) over the kept dims, the stated TR, and whether input 2 is input 1 again."""

    def __init__(self, dims, rdims, lays, dlay, tr, dup=False):
        self.dims, self.rdims, self.lays, self.dlay, self.tr, self.dup = tuple(int(d) for d in dims), tuple(rdims), lays, dlay, int(tr), dup
        self.kept = [d for d in range(len(self.dims)) if d not in self.rdims]
        self.total = int(np.prod(self.dims))
        self.nout = int(np.prod([self.dims[d] for d in self.kept])) if self.kept else 1
        self.red = self.total // self.nout
        self.ob = 256 // self.tr
        self.W = -(-self.nout // self.ob)


def mem(dims, rdims, nin=1, perm=None, steps=None, pads=1, bcast=None, dperm=None, dsteps=None, tr=None, dup=False, perms=None):
    """dims reduced over rdims.  Input k: view dim i is parent dim perm[i] (perms[k]: per input) stepped by steps[i], with 1 along the dims
    in bcast[k]; the destination: kept dim j is parent dim dperm[j] stepped by dsteps[j]."""
    N = len(dims)
    rdims = (rdims,) if isinstance(rdims, int) else tuple(rdims)
    bcast = bcast or {}
    lays = []
    for k in range(nin):
        p = tuple(perm if perms is None else perms[k]) if (perm is not None or perms is not None) else tuple(range(N))
        lays.append((p, [(pads * (i + k)) % 3 for i in range(N)], [(pads * (i + 2 * k + 1)) % 4 for i in range(N)], list(steps or [1] * N), tuple(bcast.get(k, ()))))
    nk = N - len(rdims)
    dlay = (tuple(dperm or range(nk)), [(i + 1) % 3 for i in range(nk)], [i % 2 for i in range(nk)], list(dsteps or [1] * nk))
    sp = Spec(dims, rdims, lays, dlay, tr or 1, dup)
    if tr is None:
        assert sp.nout < 65536, "state TR for a member of 65536 outputs or more"
        sp = Spec(dims, rdims, lays, dlay, lanes_small(sp.red), dup)
    return sp


class Member:
    """A built member: its inputs (Operand), its destination's (offset, strides) in the row's parent, the expected destination
    elements (keepdims shape) after 1, 2 and 3 applications."""

    def __init__(self, dims, ins, off, dstrides, osh, initop, wants, spec):
        self.dims, self.ins, self.off, self.dstrides, self.osh, self.initop, self.wants, self.spec = dims, ins, off, dstrides, osh, initop, wants, spec


class Row(GR.Row):
    """(name, type, op, f, kind of initop, members, ...) as in tests/group_reduce_cases.py"""

    def build(self):
        """(members, destination parent): deterministic, cached (the parents are never written: tests copy them)."""
        if self._built is not None:
            return self._built
        t, op, f, cx = self.t, self.op, self.f, RF.is_cx(self.t)
        rng = np.random.default_rng([RF.SEED_OFFSET, 2560, len(self.name), sum(map(ord, self.name))])
        dlays, base = [], 1 + len(self.name) % 3
        for sp in self.specs:   # the destinations, one behind the other with a gap of one element
            plen, kstr, off = layout([sp.dims[d] for d in sp.kept], *sp.dlay) if sp.kept else (1, (), 0)
            dlays.append((base + off, kstr))
            base += plen + 1
        plen = base + 2
        parent = aligned_empty(plen, self.ddt)
        parent[...] = rng.integers(0, 2, size=plen).astype(np.bool_) if self.ddt == np.bool_ else finite_bits(rng, plen, self.ddt)
        members = []
        for i, sp in enumerate(self.specs):
            dims, N, rdims = sp.dims, len(sp.dims), sp.rdims
            initop = self.initop(i)
            osh = RF.keepshape(dims, rdims)
            shapes = [tuple(1 if d in bd else n for d, n in enumerate(dims)) for _, _, _, _, bd in sp.lays]
            if sp.dup:
                shapes[1] = shapes[0]
            seen = RF.draw_data(rng, t, op, f, "none", dims, rdims, shapes, initop, self.mixed, sp.red)
            assert seen is not None, (self.name, i, "no magnitude keeps the sums exact")
            if sp.dup:
                seen[1] = seen[0]
            if t == "bool":
                old = RF._objarr([(op == "&") if rng.integers(0, 4) else (op == "|") for _ in range(sp.nout)], osh)
            elif op == "*":
                old = RF._objarr([RF._pick(rng, (1, -1)) * (1 if RF.is_int(t) else 1.0) for _ in range(sp.nout)], osh)
            elif op in ("min", "max"):
                old = RF._objarr([(int(v) if RF.is_int(t) else float(v)) for v in rng.integers(-1200, 1201, size=sp.nout)], osh)
            elif cx:
                old = RF._objarr([complex(int(a), int(b)) for a, b in rng.integers(-4, 5, size=(sp.nout, 2))], osh)
            else:
                old = RF._objarr([int(v) for v in rng.integers(-4, 5, size=sp.nout)], osh)
            full = [tuple(np.broadcast_to(c, dims) for c in s) if cx else np.broadcast_to(s, dims) for s in seen]
            part = RF.reduce_exact(op, f, full, dims, rdims, t)
            wants = {k: RF.to_dt(w, self.ddt) for k, w in RF.applications(op, initop, old, part, t).items()}
            ins = []
            for k, ((perm, plo, phi, steps, bd), s) in enumerate(zip(sp.lays, seen)):
                if sp.dup and k == 1:
                    ins.append(ins[0])
                    continue
                e = tuple(1 if d in bd else n for d, n in enumerate(dims))
                lay = layout(e, perm, plo, phi, list(steps))
                tk = self.in_types[k]
                dt = DT[tk]
                vals = (s[0] + 1j * s[1]).astype(dt) if cx else s.astype(dt)
                assert cx or np.array_equal(vals.astype(s.dtype), s), "the input type holds the data"
                fill = np.iinfo(np.int16).max if tk == "i16" else RF.filler_for(tk, op)
                ins.append(self._input(dt, dims, lay, bd, vals, fill, self.conjs[k]))
            off, kstr = dlays[i]
            dstrides = [0] * N
            for j, d in enumerate(sp.kept):
                dstrides[d] = kstr[j]
            o = RF.to_dt(old, self.ddt)
            parent[_index(off, osh, dstrides)] = np.conj(o) if self.dconj else o
            members.append(Member(dims, ins, off, tuple(dstrides), osh, initop, wants, sp))
        self._built = (members, parent)
        return self._built

    def expected_parent(self, times=1):
        members, parent = self.build()
        out = parent.copy()
        for m in members:
            w = m.wants[times]
            out[_index(m.off, m.osh, m.dstrides)] = np.conj(w) if self.dconj else w
        return out

    def views(self, wrap=None):
        """(destination parent as wrapped, [(destination, inputs...) per member]) over copies of the parents (default: 64-byte aligned
        host copies, the alignment device allocations have); an input passed twice is wrapped once."""
        def aligned_copy(a):
            out = aligned_empty(a.size, a.dtype)
            out[...] = a
            return out
        wrap = wrap or aligned_copy
        members, parent = self.build()
        dpar = wrap(parent)
        out = []
        for m in members:
            done = {}
            dest = S.StridedView(dpar, m.dims, m.dstrides, m.off, "conj" if self.dconj else "identity")
            ins = []
            for o in m.ins:
                if id(o) not in done:
                    done[id(o)] = wrap(o.parent)
                ins.append(S.StridedView(done[id(o)], m.dims, o.strides, o.offset, "conj" if o.conj else "identity"))
            out.append((dest,) + tuple(ins))
        return dpar, out

    def group(self, views, independent=False, stream=0, reduce=True, reduce_part=True, **kw):
        ps = self.problems(views, stream)
        return L.Group([p[0] for p in ps], independent, keepalive=(ps, views), reduce=reduce, reduce_part=reduce_part, **kw)

    def layout(self):
        """what smr_group_layout must report: (form, first workgroup, W) per member"""
        out, first = [], 0
        for sp in self.specs:
            out.append((FORM_PART, first, sp.W))
            first += sp.W
        return out

    def lanes_token(self):
        """the lanes= token of describe(): the distinct TR, ascending, each with its member count"""
        trs = [sp.tr for sp in self.specs]
        return ",".join("%d:%d" % (tr, trs.count(tr)) for tr in sorted(set(trs)))


def mismatch(row, got_parent, want_parent, what):
    """None when the whole destination parent holds the expected bytes, else a message naming the members that differ."""
    g8, w8 = np.ascontiguousarray(got_parent).view(np.uint8).ravel(), np.ascontiguousarray(want_parent).view(np.uint8).ravel()
    if g8.size == w8.size and np.array_equal(g8, w8):
        return None
    if g8.size != w8.size:
        return "%s | %s: parent of %d bytes, expected %d" % (row.name, what, g8.size, w8.size)
    bad = set(int(e) for e in np.unique(np.nonzero(g8 != w8)[0] // row.ddt.itemsize))
    members, _ = row.build()
    inside, owned = [], set()
    for i, m in enumerate(members):
        idx = set(int(e) for e in _index(m.off, m.osh, m.dstrides).ravel())
        owned |= idx
        hit = sorted(idx & bad)
        if hit and len(inside) < 4:
            inside.append("member %d (dims %s reduced %s, TR %d, W %d): %d elements, first at %d got %r want %r" % (
                i, m.spec.dims, m.spec.rdims, m.spec.tr, m.spec.W, len(hit), hit[0], got_parent.ravel()[hit[0]], want_parent.ravel()[hit[0]]))
    outside = sorted(bad - owned)
    return "%s | %s: %d elements differ; %s%s" % (row.name, what, len(bad), "; ".join(inside),
                                                 ("; %d elements outside the destinations written, first %s" % (len(outside), outside[:4])) if outside else "")


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def edge(red, nin=1, reduced_first=True):
    """members of `red` reduced elements at nout = 1, 256 / TR - 1, 256 / TR, 256 / TR + 1 and with several workgroups: dead lanes and the
    last partial workgroup.  The inputs' unit-stride dim is the reduced one (reduced_first) or the kept one."""
    ob = 256 // lanes_small(red)
    out = []
    for j, nout in enumerate(sorted({1, max(1, ob - 1), ob, ob + 1, 2 * ob + 1})):
        first = reduced_first if j % 2 == 0 else not reduced_first
        out.append(mem((nout, red), 1, nin, perm=(1, 0) if first else (0, 1), dsteps=[(1, 2, -1)[j % 3]]))
    return out


def standard(nin=1, dup=False):
    """Nine members of unequal TR, rank and W: reduced dims before, between and after the kept ones, all and none reduced."""
    kw = dict(nin=nin, dup=dup)
    return [mem((5, 7), 1, **kw),
            mem((40, 33), 1, perm=(1, 0), **kw),                                      # TR 32, W 5
            mem((6, 5, 4), (0, 2), steps=(1, -1, 2), **kw),
            mem((300, 3), 1, dsteps=[2], **kw),                                        # TR 2, W 3
            mem((4, 9), (), dperm=(1, 0), **kw),                                       # no reduced dim
            mem((3, 130), 1, perm=(1, 0), dsteps=[-1], **kw),                          # TR 128: through LDS
            mem((2, 3, 4, 5), (1, 2), perm=(3, 1, 0, 2), dperm=(1, 0), **kw),
            mem((70,), 0, **kw),                                                       # one destination element
            mem((9, 2, 260), (0, 2), perm=(2, 0, 1), **kw)]                           # TR 256


def tiny(count, nin=1):
    return [mem((1 + i % 4, 1 + (5 * i) % 23), (1, 0, ())[i % 3] if i % 3 < 2 else (), nin, dsteps=None) for i in range(count)]


def order_row(t):
    """Members of TR = 1, 2, 32, 64, 128 and 256 whose reduced length is no multiple of TR and whose outputs straddle a workgroup, for the
    guarantee's test on random data: every member's single plan under "reduce_part_kind" = 0 reads form=general ... split=1 (asserted
    on the host), and the default planner gives ROW or COL forms to some."""
    f, nin, conjs = {"f32": ("abs2", 1, None), "f64": ("mul", 2, None), "c64": ("mul", 2, (True, False))}[t]
    kw = dict(nin=nin)
    specs = [mem((259, 255, 3), 2, tr=1, **kw),                                  # 66045 outputs on one lane each: 258 workgroups
             mem((129, 3), 1, **kw), mem((3, 129), 0, perm=(1, 0), **kw),        # TR 2, 128 outputs per workgroup
             mem((9, 45), 1, perm=(1, 0), **kw), mem((45, 9), 0, **kw),          # TR 32
             mem((5, 100), 1, perm=(1, 0), **kw), mem((5, 4, 25), (1, 2), **kw),  # TR 64
             mem((3, 200), 1, perm=(1, 0), **kw), mem((200, 3), 0, **kw),        # TR 128: two waves per output
             mem((3, 300), 1, perm=(1, 0), **kw), mem((2, 3, 150), (0, 2), perm=(2, 0, 1), **kw)]   # TR 256
    return Row("order/%s" % t, t, "+", f, "scale", specs, conjs=conjs)


_TABLE = None


def table():
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    rows = []
    add = lambda *a, **kw: rows.append(Row(*a, **kw))   # noqa: E731
    # reduced lengths at the edges of TR = 1 .. 256, outputs at the edges of a workgroup
    add("edges/1-33/f64", "f64", "+", "ident", "none", [m for red in (1, 2, 3, 31, 32, 33) for m in edge(red)])
    add("edges/63-127/f32", "f32", "+", "abs2", "scale", [m for red in (63, 64, 65, 127) for m in edge(red)])
    add("edges/128-255/c64", "c64", "+", "ident", "zero", [m for red in (128, 129, 255) for m in edge(red)])
    add("edges/256-511/f64", "f64", "+", "mul", "none", [m for red in (256, 257, 511) for m in edge(red, 2)])
    # 65536 outputs on one lane each, 256 workgroups: inputs unit-stride along kept dim 0
    add("wide/f32", "f32", "+", "ident", "none", [mem((3, 5), 1), mem((256, 256, 3), 2, tr=1), mem((4, 40), 1, perm=(1, 0))])
    # where the reduced dims stand in the caller's order; kept rank 1 - 3, reduced rank 1 - 3
    add("dims/rank3/f64", "f64", "+", "ident", "scale", [mem((6, 5, 4), 0), mem((6, 5, 4), 1, perm=(1, 0, 2)), mem((6, 5, 4), (0, 2), dsteps=[-1]),
                                                         mem((6, 5, 4), (1, 2), steps=(2, 1, 1)), mem((6, 5, 4), (0, 1), perm=(2, 1, 0), dsteps=[3])])
    add("dims/rank4/f32", "f32", "+", "abs2", "none", [mem((3, 4, 5, 2), 0, dperm=(2, 0, 1)), mem((3, 4, 5, 2), 1, perm=(3, 1, 0, 2), dsteps=[1, -1, 2]),
                                                      mem((3, 4, 5, 2), (0, 2), dperm=(1, 0)), mem((3, 4, 5, 2), (1, 2), steps=(-1, 1, 3, 1)),
                                                      mem((3, 4, 5, 2), (0, 1, 3)), mem((3, 4, 5, 6), (1, 2, 3), perm=(1, 2, 3, 0)), mem((7, 3, 4, 5), (0, 1, 2))])
    # permuted, stepped, reversed destinations
    add("dest/windows/f64", "f64", "+", "ident", "none", [mem((7, 6, 5), 2, dperm=(1, 0), dsteps=[2, -1]), mem((7, 6, 5), 0, dperm=(1, 0), dsteps=[-1, -2]),
                                                         mem((9, 4, 3, 2), 1, dperm=(2, 0, 1), dsteps=[-1, 1, 2]), mem((31, 9), 1, dsteps=[-3])])
    # a matrix-vector product (input 2 broadcast along the kept dim); an input broadcast along the reduced dim
    add("bcast/matvec/f64", "f64", "+", "mul", "none", [mem((32, 32), 1, 2, bcast={1: (0,)}), mem((8, 8), 1, 2, bcast={1: (0,)}), mem((33, 17), 1, 2, perm=(1, 0), bcast={1: (0,)}),
                                                       mem((5, 6, 7), (0, 2), 2, bcast={1: (1,)})])
    add("bcast/reduced/f32", "f32", "+", "mul", "zero", [mem((32, 32), 1, 2, bcast={1: (1,)}), mem((9, 70), 1, 2, perm=(1, 0), bcast={0: (1,)}), mem((4, 5, 6), (1, 2), 2, bcast={1: (1, 2)})])
    add("conj/c64", "c64", "+", "mul", "none", standard(2), conjs=(True, False), dconj=True)
    add("conj/matvec-adjoint/c64", "c64", "+", "mul", "scale", [mem((32, 32), 0, 2, bcast={1: (1,)}), mem((7, 33), 0, 2, perm=(1, 0), bcast={1: (1,)})], conjs=(True, False))
    # no reduced dim: dest[I] = op(initop(dest[I]), f(...))
    add("accumulate/f64", "f64", "+", "ident", "scale", [mem((9, 7), (), dperm=(1, 0)), mem((300,), (), dsteps=[2]), mem((4, 3, 5), (), steps=(1, 2, -1)), mem((1,), ())])
    # ops and initops
    add("ops/prod/f64", "f64", "*", "ident", "scale", standard(1))
    add("ops/prod-mul/f32", "f32", "*", "mul", "none", standard(2))
    add("ops/min/f64", "f64", "min", "ident", "const", standard(1))
    add("ops/max/f32", "f32", "max", "ident", "zero", standard(1))
    add("ops/min/i64", "i64", "min", "ident", "none", standard(1))
    add("ops/and/bool", "bool", "&", "ident", "none", standard(1))
    add("ops/or/bool", "bool", "|", "ident", "none", standard(1))
    add("ops/sum-conj/c32", "c32", "+", "ident", "conj", standard(1), conjs=(True,))
    # types
    add("types/c32", "c32", "+", "mul", "scale", standard(2), conjs=(True, False))
    add("types/i64", "i64", "+", "mul", "scale", standard(2))
    add("types/i32-wraps", "i32", "+", "abs2", "none", standard(1))
    add("types/f32-into-f64", "f32", "+", "abs2", "scale", standard(1), mixed=True)
    add("types/i16-of-f32", "f32", "+", "mul", "none", standard(2), in_types=("f32", "i16"))
    add("types/repeated/f32", "f32", "+", "mul", "none", standard(2, dup=True))
    # how f runs
    add("f/ident/f64", "f64", "+", "ident", "none", standard(1))
    add("f/abs2/c64", "c64", "+", "abs2", "const", standard(1), dconj=True)
    add("f/mul/f64", "f64", "+", "mul", "zero", standard(2))
    add("f/prog/f32", "f32", "+", "prog", "scale", standard(2), jit=0)
    add("f/prog/c64", "c64", "+", "prog", "none", standard(2), jit=1)
    add("f/amc/i64", "i64", "+", "amc", "zero", standard(3), jit=1)
    # member counts
    add("count/1", "f64", "+", "abs2", "none", [mem((40, 33), 1, perm=(1, 0))])
    add("count/2", "f32", "+", "ident", "scale", [mem((3, 5), 0), mem((300, 3), 1)])
    add("count/257", "f64", "+", "mul", "scale", tiny(257, 2))
    add("count/2049", "f32", "+", "ident", "none", tiny(2049))
    _TABLE = rows
    return rows


def row(name):
    return {r.name: r for r in table()}[name]
