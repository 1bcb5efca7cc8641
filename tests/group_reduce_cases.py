"""Deterministic table of REDUCTION GROUPS (SMR_GROUP_REDUCE; tests/test_group_reduce_host.py, tests/test_gpu_group_reduce.py).

A row is a list of members, each a complete reduction over windowed operands of its own, built from the pieces of the complete-
reduction recipes of tests/reduce_fuzz_cases.py (layouts, inputs, data, exact arithmetic): every input is a window of a padded parent
filled with NaN (Bool and the integers: the value that would change the result), the data make every accumulation order give the same
bits, and the expected values are computed from the integers in exact arithmetic for 1, 2 and 3 applications.  The K destinations of a
row are single elements, two apart, of ONE padded K-vector whose other elements hold random bits: that whole parent is what the tests
compare, byte for byte.  One f, one op, one kind of initop and one conj flag per operand position per row (what a group shares); beta
differs from member to member under `scale`.

Every member states the workgroups W = min(ceil(total / 4096), 64) and the body (vector / strided) the planner must give it.  Nothing
here imports torch."""
import numpy as np

import reduce_fuzz_cases as RF
import strided_jl_amd as S
from reduce_exact_cases import Operand, _index, aligned_empty
from strided_jl_amd import _lib as L
from window_cases import finite_bits, layout

PER_BLOCK, FOLD_MAX = 4096, 64          # include/strided_hip.h, REDUCTION GROUPS
FORM_STRIDED, FORM_VECTOR = 3, 4        # smr_group_layout
DT = dict(RF.IN_DT)
DT["i16"] = np.int16


def workgroups(total):
    return min(-(-total // PER_BLOCK), FOLD_MAX)


class Spec:
    """One member: dims (every dim is reduced), per input (perm, lo, hi, steps, broadcast dims), whether the planner must take the
    vector body, and whether input 2 is input 1 again."""

    def __init__(self, dims, lays, vec=False, dup=False):
        self.dims, self.lays, self.vec, self.dup = tuple(int(d) for d in dims), lays, vec, dup
        self.total = int(np.prod(self.dims))
        self.W = workgroups(self.total)


def lin(n, lo=0, step=1, nin=1, vec=False, los=None, bcast=(), dup=False):
    """Rank 1: input k starts lo (los[k]) elements into its parent and steps by `step`; inputs in `bcast` have stride 0."""
    lays = []
    for k in range(nin):
        l = lo if los is None else los[k]
        lays.append(((0,), [l], [(k + 2) % 4], [step], (0,) if k in bcast else ()))
    return Spec((n,), lays, vec, dup)


def box(dims, perm, steps, nin=1, pads=1, dup=False, perms=None, vec=False):
    """Rank >= 2: view dim i is parent dim perm[i] (perms[k]: per input), stepped by steps[i].  vec: only a whole parent (pads = 0, no
    permutation, no steps), which fuses into one unit-stride run."""
    N = len(dims)
    lays = []
    for k in range(nin):
        p = perm if perms is None else perms[k]
        lays.append((tuple(p), [(pads * (i + k)) % 3 for i in range(N)], [(pads * (i + 2 * k + 1)) % 4 for i in range(N)], list(steps), ()))
    return Spec(dims, lays, vec, dup)


class Member:
    """A built member: its inputs (Operand), its destination element's offset in the row's K-vector, the old value there and the
    expected value after 1, 2 and 3 applications."""

    def __init__(self, dims, ins, off, initop, wants, spec):
        self.dims, self.ins, self.off, self.initop, self.wants, self.spec = dims, ins, off, initop, wants, spec


class Row:
    def __init__(self, name, t, op, f, kind, specs, conjs=None, dconj=False, mixed=False, in_types=None, jit=None):
        self.name, self.t, self.op, self.f, self.kind, self.specs = name, t, op, f, kind, specs
        nin = RF.NIN[f]
        self.conjs = tuple(conjs) if conjs else (False,) * nin
        self.dconj, self.mixed, self.jit = dconj, mixed, jit
        self.in_types = tuple(in_types) if in_types else (t,) * nin          # "i16": an Int16 input of a float class
        self.ddt = np.dtype(np.float64 if mixed else (np.int64 if t == "i32" else DT[t]))
        # what does not run a natively compiled functor: programs, converted operands, and x * x of ONE deduplicated input
        self.needs_prog = f in ("prog", "amc") or mixed or t in ("bool", "i32") or any(x != t for x in self.in_types) or any(sp.dup for sp in specs)
        self._built = None

    def __repr__(self):
        return self.name

    def initop(self, i):
        cx = RF.is_cx(self.t)
        if self.kind == "scale":
            b = (2, -1, 3)[i % 3] if self.op != "*" else (2, -1, -2)[i % 3]
            return ("scale", complex(b, (1, -1, 0)[i % 3]) if cx and abs(b) < 3 else b)
        if self.kind == "const":
            return ("const", complex(2, -1) if cx else (2 if self.op != "*" else -1))
        return {"none": None, "zero": "zero", "conj": "conj"}[self.kind]

    # -- building ---------------------------------------------------------------------------------------------------------------
    def build(self):
        """(members, destination parent): deterministic, cached (the parents are never written: tests copy them)."""
        if self._built is not None:
            return self._built
        t, op, f, cx = self.t, self.op, self.f, RF.is_cx(self.t)
        rng = np.random.default_rng([RF.SEED_OFFSET, 4242, len(self.name), sum(map(ord, self.name))])
        K = len(self.specs)
        lo = 1 + len(self.name) % 3
        plen = lo + 2 * K + 2
        if self.ddt == np.bool_:
            parent = aligned_empty(plen, np.bool_)
            parent[...] = rng.integers(0, 2, size=plen).astype(np.bool_)
        else:
            parent = aligned_empty(plen, self.ddt)
            parent[...] = finite_bits(rng, plen, self.ddt)
        members = []
        for i, sp in enumerate(self.specs):
            dims, N = sp.dims, len(sp.dims)
            rdims = tuple(range(N))
            initop = self.initop(i)
            shapes = [tuple(1 if d in bd else n for d, n in enumerate(dims)) for _, _, _, _, bd in sp.lays]
            if sp.dup:
                shapes[1] = shapes[0]
            seen = RF.draw_data(rng, t, op, f, "none", dims, rdims, shapes, initop, self.mixed, sp.total)
            assert seen is not None, (self.name, i, "no magnitude keeps the sums exact")
            if sp.dup:
                seen[1] = seen[0]
            if t == "bool":
                old = RF._objarr([(op == "&") if rng.integers(0, 4) else (op == "|")], (1,) * N)
            elif op == "*":
                old = RF._objarr([RF._pick(rng, (1, -1)) * (1 if RF.is_int(t) else 1.0)], (1,) * N)
            elif op in ("min", "max"):
                v = int(rng.integers(-1200, 1201))
                old = RF._objarr([v if RF.is_int(t) else float(v)], (1,) * N)
            elif cx:
                old = RF._objarr([complex(int(rng.integers(-4, 5)), int(rng.integers(-4, 5)))], (1,) * N)
            else:
                old = RF._objarr([int(rng.integers(-4, 5))], (1,) * N)
            full = [tuple(np.broadcast_to(c, dims) for c in s) if cx else np.broadcast_to(s, dims) for s in seen]
            part = RF.reduce_exact(op, f, full, dims, rdims, t)
            wants = {k: RF.to_dt(w, self.ddt).reshape(()) for k, w in RF.applications(op, initop, old, part, t).items()}
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
            off = lo + 2 * i
            o = RF.to_dt(old, self.ddt).reshape(())
            parent[off] = np.conj(o) if self.dconj else o
            members.append(Member(dims, ins, off, initop, wants, sp))
        self._built = (members, parent)
        return self._built

    @staticmethod
    def _input(dt, dims, lay, bdims, seen, fill, conj):
        """RF.make_input for any input dtype"""
        plen, strides, off = lay
        e = tuple(1 if i in bdims else n for i, n in enumerate(dims))
        parent = aligned_empty(plen, dt)
        parent[...] = fill
        parent[_index(off, e, strides)] = np.conj(seen) if conj else seen
        return Operand(dt, plen, off, tuple(0 if i in bdims else s for i, s in enumerate(strides)), conj=conj, parent=parent)

    def expected_parent(self, times=1):
        members, parent = self.build()
        out = parent.copy()
        for m in members:
            w = m.wants[times]
            out[m.off] = np.conj(w) if self.dconj else w
        return out

    # -- views, problems, groups --------------------------------------------------------------------------------------------------
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
            N = len(m.dims)
            dest = S.StridedView(dpar, m.dims, (0,) * N, m.off, "conj" if self.dconj else "identity")
            ins = []
            for o in m.ins:
                if id(o) not in done:
                    done[id(o)] = wrap(o.parent)
                ins.append(S.StridedView(done[id(o)], m.dims, o.strides, o.offset, "conj" if o.conj else "identity"))
            out.append((dest,) + tuple(ins))
        return dpar, out

    def fn(self):
        return RF.F[self.f]

    def problems(self, views, stream=0):
        members, _ = self.build()
        return [S.build_problem(self.fn(), self.op, m.initop, m.dims, v, stream=stream) for m, v in zip(members, views)]

    def group(self, views, independent=False, stream=0, reduce=True, **kw):
        ps = self.problems(views, stream)
        return L.Group([p[0] for p in ps], independent, keepalive=(ps, views), reduce=reduce, **kw)

    def layout(self):
        """what smr_group_layout must report: (form, first workgroup, W, canonical rank is not stated) per member"""
        out, first = [], 0
        for sp in self.specs:
            out.append((FORM_VECTOR if sp.vec else FORM_STRIDED, first, sp.W))
            first += sp.W
        return out


def mismatch(row, got_parent, want_parent, what):
    """None when the whole destination parent holds the expected bytes, else a message naming the members that differ."""
    g8, w8 = np.ascontiguousarray(got_parent).view(np.uint8).ravel(), np.ascontiguousarray(want_parent).view(np.uint8).ravel()
    if g8.size == w8.size and np.array_equal(g8, w8):
        return None
    if g8.size != w8.size:
        return "%s | %s: parent of %d bytes, expected %d" % (row.name, what, g8.size, w8.size)
    es = row.ddt.itemsize
    bad = np.unique(np.nonzero(g8 != w8)[0] // es)
    members, _ = row.build()
    at = {m.off: i for i, m in enumerate(members)}
    inside = ["member %d (total %d, W %d): got %r want %r" % (at[e], members[at[e]].spec.total, members[at[e]].spec.W, got_parent.ravel()[e], want_parent.ravel()[e])
              for e in bad[:64] if int(e) in at][:4]
    outside = [int(e) for e in bad if int(e) not in at]
    return "%s | %s: %d elements differ; %s%s" % (row.name, what, len(bad), "; ".join(inside),
                                                 ("; %d elements outside the destinations written, first %s" % (len(outside), outside[:4])) if outside else "")


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def standard(nin=1, V=4, dup=False):
    """Seven members mixing W = 1, 2 and 3, both bodies and ranks 1 to 3."""
    return [lin(5, lo=1, nin=nin, dup=dup),
            lin(4096 + 2 * V, nin=nin, vec=V > 1, dup=dup),                       # W = 2, vector
            box((7, 5), (1, 0), (1, 2), nin=nin, dup=dup),
            lin(4097, lo=1, step=2, nin=nin, dup=dup),                            # W = 2, strided
            box((6, 5, 4), (2, 0, 1), (1, -1, 2), nin=nin, dup=dup),
            lin(8192 + 1, nin=nin, dup=dup),                                      # W = 3, strided
            lin(300, step=-1, nin=nin, dup=dup)]


def tiny(count, nin=1):
    return [lin(1 + (5 * i) % 23, lo=i % 3, step=(1, 2, -1)[i % 3], nin=nin) for i in range(count)]


_TABLE = None


def table():
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    V = RF.VMAX
    rows = []
    add = lambda *a, **kw: rows.append(Row(*a, **kw))   # noqa: E731
    # member totals at the planning edges; members of unequal W in one group
    add("edges/small/f64", "f64", "+", "ident", "none", [lin(n, lo=n % 2, step=1 + n % 2) for n in (1, 63, 64, 65, 255, 256, 257)])
    add("edges/block/f32", "f32", "+", "abs2", "scale", [lin(4095), lin(4096, vec=True), lin(4097), lin(8192, vec=True), lin(8193)])
    add("edges/block/c64", "c64", "+", "ident", "zero", [lin(4095, lo=1), lin(4096), lin(4097, step=2), lin(8192), lin(8193, lo=2)])
    add("edges/cap/f64", "f64", "+", "ident", "none", [lin(262144, vec=True), lin(7), lin(262145), lin(262144, lo=1)])
    # vector against strided
    add("bodies/f32", "f32", "+", "ident", "zero", [lin(4096, vec=True), lin(4100, vec=True), lin(4096, lo=1), lin(4100, lo=1), lin(4098), lin(4092),
                                                   lin(4096, lo=4, vec=True), lin(4096, step=2),
                                                   lin(4096, step=-1, vec=True)])   # (a reversed reduced dim is canonicalised to unit stride from its lowest address)
    add("bodies/f64", "f64", "+", "abs2", "none", [lin(4098, vec=True), lin(4098, lo=1), lin(4099), lin(4092), lin(4098, lo=2, vec=True),
                                                  box((64, 65), (0, 1), (1, 1), pads=0, vec=True), box((64, 65), (0, 1), (1, 1))])   # a whole parent fuses to rank 1; a window does not
    add("bodies/bcast/f32", "f32", "+", "mul", "none", [lin(4096, nin=2, bcast=(1,), vec=True), lin(4096, nin=2, vec=True), lin(4096, nin=2, los=(0, 1)),
                                                      lin(4096, nin=2, bcast=(0,), los=(0, 4), vec=True), lin(12, nin=2, bcast=(1,))])
    # ranks 2 - 4: permuted, stepped, reversed; one, two (conj), three inputs; a repeated input
    boxes = lambda nin, dup=False: [box((7, 5), (0, 1), (1, 1), nin, dup=dup), box((7, 5), (1, 0), (2, 1), nin, dup=dup), box((6, 5, 4), (2, 0, 1), (1, -1, 2), nin, dup=dup),  # noqa: E731
                                    box((3, 4, 5, 2), (3, 1, 0, 2), (-1, 1, 3, 1), nin, dup=dup), box((71, 59), (0, 1), (1, 1), nin, pads=0, dup=dup),
                                    box((33, 9, 17), (1, 2, 0), (2, 1, -1), nin, dup=dup), box((4, 3, 2, 5), (0, 1, 2, 3), (1, 1, 1, 1), nin, pads=0, dup=dup)]
    add("ranks/one/f32", "f32", "+", "ident", "scale", boxes(1))
    add("ranks/two-conj/c64", "c64", "+", "mul", "none", boxes(2), conjs=(True, False), dconj=True)
    add("ranks/two-perms/f64", "f64", "+", "mul", "zero", [box((7, 5), None, (1, 1), 2, perms=((0, 1), (1, 0))), box((6, 5, 4), None, (1, 2, 1), 2, perms=((2, 0, 1), (0, 1, 2))),
                                                        box((71, 59), None, (1, 1), 2, perms=((1, 0), (0, 1)))])
    add("ranks/three/f64", "f64", "+", "amc", "const", boxes(3), jit=1)
    add("ranks/repeated/f32", "f32", "+", "mul", "none", boxes(2, dup=True) + [lin(4096, nin=2, dup=True, vec=True)])
    # ops and initops
    add("ops/prod/f64", "f64", "*", "ident", "scale", standard(1, V["f64"]))
    add("ops/prod-mul/f32", "f32", "*", "mul", "none", standard(2, V["f32"]))
    add("ops/min/f64", "f64", "min", "ident", "const", standard(1, V["f64"]))
    add("ops/max/f32", "f32", "max", "ident", "zero", standard(1, V["f32"]))
    add("ops/min/i64", "i64", "min", "ident", "none", standard(1, V["i64"]))
    add("ops/and/bool", "bool", "&", "ident", "none", standard(1, 1))
    add("ops/or/bool", "bool", "|", "ident", "none", standard(1, 1))
    add("ops/sum-conj/c32", "c32", "+", "ident", "conj", standard(1, V["c32"]), conjs=(True,))
    add("ops/sum-const/c64", "c64", "+", "abs2", "const", standard(1, 1), dconj=True)
    # types
    add("types/f32", "f32", "+", "ident", "none", standard(1, V["f32"]))
    add("types/f64", "f64", "+", "ident", "scale", standard(1, V["f64"]))
    add("types/c32", "c32", "+", "mul", "scale", standard(2, V["c32"]), conjs=(True, False))
    add("types/c64", "c64", "+", "mul", "zero", standard(2, 1), conjs=(False, True))
    add("types/i64", "i64", "+", "mul", "scale", standard(2, V["i64"]))
    add("types/i32-wraps", "i32", "+", "abs2", "none", standard(1, 1))
    add("types/i64-prod", "i64", "*", "ident", "const", standard(1, V["i64"]))
    add("types/f32-into-f64", "f32", "+", "abs2", "scale", standard(1, 1), mixed=True)
    add("types/i16-of-f32", "f32", "+", "mul", "none", standard(2, 1), in_types=("f32", "i16"))
    # how f runs: the recognised functors, an interpreted program, a runtime-compiled one (the GPU test runs program rows both ways)
    add("f/ident/c32", "c32", "+", "ident", "none", standard(1, V["c32"]))
    add("f/abs2/f64", "f64", "+", "abs2", "zero", standard(1, V["f64"]))
    add("f/mul/f64", "f64", "+", "mul", "none", standard(2, V["f64"]))
    add("f/prog/f32", "f32", "+", "prog", "scale", standard(2, V["f32"]), jit=0)
    add("f/prog/c64", "c64", "+", "prog", "none", standard(2, 1), jit=1)
    add("f/amc/i64", "i64", "+", "amc", "zero", standard(3, V["i64"]), jit=1)
    # member counts
    add("count/1", "f64", "+", "abs2", "none", [lin(4097)])
    add("count/2", "f32", "+", "ident", "scale", [lin(3), lin(4096, vec=True)])
    add("count/257", "f64", "+", "mul", "scale", tiny(257, 2))
    add("count/2049", "f32", "+", "ident", "none", tiny(2049))
    _TABLE = rows
    return rows


def row(name):
    return {r.name: r for r in table()}[name]
