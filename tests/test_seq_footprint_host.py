"""CPU: the byte ranges the replay scheduler is fed (footprint() in csrc/smr_api.cpp over operand_span() in csrc/smr_group.h), on the
plans of the case tables: window_cases (TILED, STREAM, FLAT, ORBIT, GENERIC), reduce_fuzz_cases (REDUCE_ALL, REDUCE_PART),
contract_cases and contract_split_cases (CONTRACT).  Host plans over NumPy parents and Sequence.components(), as in
tests/test_seq_components.py; nothing here needs a device.

For every operand of a row the lowest and the highest parent element it touches are taken from window_cases.element_index, and a probe
-- a one-element copy plan recorded after the row's plan -- must behave as follows:
  * writing that element joins the row's component, whatever the operand;
  * reading it joins the component when the row writes it (the destination, or an input that lies inside the destination's range);
  * reading it stays apart for a pure input;
  * touching the element just below the lowest / just above the highest, where that element is inside the parent and outside every
    operand's byte range, stays apart: the ranges are tight, which is what lets disjoint column blocks of one parent overlap.
The operands met include reversed, stepped, broadcast (stride 0), conjugated views, dropped size-1 dims and inputs that repeat one
parent (asserted below from the operands themselves).  Left out: the partials of a reduction (plan.scratch) -- a host plan is never
prepared, so it has none; tests/test_gpu_seq_program.py asserts them on the device."""
import collections

import numpy as np
import contract_cases as CC
import contract_split_cases as CS
import reduce_fuzz_cases as R
import strided_jl_amd as S
import window_cases as W

MIN_ROWS = 24


def one(parent, e):
    return S.StridedView(parent, (1,), (1,), int(e))


def probe_write(parent, e):
    return S.make_plan(lambda x: x, None, None, (1,), (one(parent, e), one(np.zeros(1, dtype=parent.dtype), 0)))


def probe_read(parent, e):
    return S.make_plan(lambda x: x, None, None, (1,), (one(np.zeros(1, dtype=parent.dtype), 0), one(parent, e)))


def joined(plan, probe, bases=None):
    q = S.Sequence().add(plan, bases=bases).add(probe)
    c = q.components()
    assert c in ([0, 0], [0, 1]), c
    return c == [0, 0]


def byte_range(parent, lo, hi):
    a = parent.ctypes.data
    return (a + lo * parent.itemsize, a + (hi + 1) * parent.itemsize)


def extremes(v):
    idx = W.element_index(v)
    return int(idx.min()), int(idx.max())


def kinds(ops, dims):
    out = set()
    for k, v in enumerate(ops):
        moving = [abs(s) for n, s in zip(v.size, v.strides) if n > 1 and s != 0]
        if any(s < 0 and n > 1 for n, s in zip(v.size, v.strides)):
            out.add("reversed")
        if moving and min(moving) > 1:
            out.add("stepped")
        if any(s == 0 and n > 1 for n, s in zip(v.size, v.strides)) or any(n == 1 and d > 1 for n, d in zip(v.size, dims)):
            out.add("broadcast")
        if any(n == 1 for n in v.size):
            out.add("size-1 dim")
        if v.op == "conj":
            out.add("conj")
        if k and any(v.parent is w.parent for w in ops[1:k]):
            out.add("repeated input")
    out.add("%d operands" % len(ops))
    return out


def check_row(name, plan, ops):
    """Returns what went wrong with the probes of one row (a list of strings) and how many probes ran."""
    bad, ran = [], 0
    spans = [byte_range(v.parent, *extremes(v)) for v in ops]
    dest = spans[0]
    for k, v in enumerate(ops):
        lo, hi = extremes(v)
        p = v.parent
        for e in (lo, hi):
            ran += 2
            if not joined(plan, probe_write(p, e)):
                bad.append("%s: writing element %d of operand %d stays apart" % (name, e, k))
            b = byte_range(p, e, e)
            written = b[0] < dest[1] and dest[0] < b[1]
            if joined(plan, probe_read(p, e)) != written:
                bad.append("%s: reading element %d of operand %d %s" % (name, e, k, "stays apart" if written else "joins"))
        for e in (lo - 1, hi + 1):
            if not 0 <= e < p.size:
                continue
            b = byte_range(p, e, e)
            if any(b[0] < s[1] and s[0] < b[1] for s in spans):
                continue
            ran += 2
            if joined(plan, probe_write(p, e)) or joined(plan, probe_read(p, e)):
                bad.append("%s: element %d next to operand %d [%d, %d] joins" % (name, e, k, lo, hi))
    return bad, ran


class Tally:
    def __init__(self):
        self.families, self.kinds, self.bad, self.probes, self.outside = collections.Counter(), collections.Counter(), [], 0, 0

    def row(self, name, plan, ops, dims):
        self.families[W.family(plan.describe())] += 1
        self.kinds.update(kinds(ops, dims))
        bad, ran = check_row(name, plan, ops)
        self.bad += bad
        self.probes += ran
        self.outside += ran - 4 * len(ops)
        plan.close()

    def done(self, families, need):
        assert not self.bad, "%d probes of %d: %s" % (len(self.bad), self.probes, self.bad[:8])
        short = {f: self.families[f] for f in families if self.families[f] < MIN_ROWS}
        assert not short, "families met too rarely: %s of %s" % (short, dict(self.families))
        missing = {k: self.kinds[k] for k in need if self.kinds[k] < 8}
        assert not missing, "operand kinds met too rarely: %s of %s" % (missing, dict(self.kinds))
        assert self.outside >= 4 * MIN_ROWS, "only %d probes next to a range" % self.outside


def test_map_families_of_the_window_table():
    t = Tally()
    for recipe in sorted(W.RECIPES):
        types = W.RECIPES[recipe]
        for seed in range(W.MORE_SEEDS.get(recipe, W.SEEDS)):
            # every type and every pad mode of a recipe (half of the GENERIC draws go to another family: one more type there)
            for dt in [types[(seed + j) % len(types)] for j in ((0, 1, 3) if recipe == "generic" else (0, 3))]:
                c = W.build(recipe, seed, dt)
                t.row(c.name, c.plan(), c.arrays, c.dims)
    t.done(("tiled", "stream", "flat", "orbit", "generic"),
           ("reversed", "stepped", "conj", "repeated input", "2 operands", "3 operands", "4 operands", "5 operands"))


def test_reduction_families_of_the_reduce_table():
    t = Tally()
    for recipe, ty in R.GROUPS:
        if recipe == "negzero":
            continue
        for seed in list(R.seeds(recipe, ty))[:4 if recipe in ("all", "all_box") else 2]:   # (REDUCE_ALL comes from two recipes only)
            c = R.build(recipe, seed, ty)
            ops = R.views(c, S)
            plan = R.with_options(c, lambda: S.make_plan(R.F[c.f], c.op, c.initop, c.dims, ops))
            t.row("%s/%s/%d" % (recipe, ty, seed), plan, ops, c.dims)
    t.done(("reduce_all", "reduce_part"), ("reversed", "stepped", "broadcast", "conj", "2 operands", "3 operands", "4 operands"))


def test_contract_family_whole_and_split():
    t = Tally()
    layouts = collections.Counter()
    for c in CC.table():
        ops = c.build()
        with CC.option("contract", 2):
            plan = c.plan(ops, "zero" if c.op else None)
        layouts.update(c.layouts)
        t.row(c.name, plan, ops, c.dims)
    whole = t.families["contract"]
    for c in CS.table():
        ops = c.build()
        with c.options():
            plan = c.plan(ops)
        assert "kparts=" in plan.describe(), plan.describe()
        layouts.update(c.layouts)
        t.row(c.name, plan, ops, c.dims)
    assert whole >= MIN_ROWS and t.families["contract"] - whole >= MIN_ROWS, dict(t.families)
    assert all(layouts[lay] >= 8 for lay in CC.LAYOUTS), dict(layouts)
    t.done(("contract",), ("reversed", "stepped", "broadcast", "size-1 dim", "conj", "3 operands"))


def test_rebound_bases_follow_the_original_operand_order():
    """One plan whose two inputs are the left and the right column block of ONE parent, recorded with every operand rebound to a
    parent of its own: the ranges are those of the rebound pointers, each with its own operand's offset and extent (the canonical
    operand k is the original operand c.orig[k]), and the planned parents are not touched at all."""
    n = 64
    P, D = np.zeros((n, n), order="F"), np.zeros((n, n // 2), order="F")
    X, Y, D2 = np.zeros_like(P), np.zeros_like(P), np.zeros_like(D)
    Pv = S.StridedView(P)
    left, right = Pv.sview(slice(None), slice(0, n // 2)), Pv.sview(slice(None), slice(n // 2, n))
    for f, ins in ((lambda a, b: a - 2 * b, (left, right)), (lambda a, b: a - 2 * b, (right, left)), (lambda a, b, c: a + b * c, (right, left, right))):
        plan = S.make_plan(f, None, None, (n, n // 2), (S.StridedView(D),) + ins)
        targets = [X if v is left else Y for v in ins]      # left blocks go to X, right blocks to Y
        bases = [D2.ctypes.data] + [t.ctypes.data for t in targets]
        flat = lambda a: a.reshape(-1, order="F")  # noqa: E731
        lo_left, hi_left, lo_right, hi_right = 0, n * n // 2 - 1, n * n // 2, n * n - 1
        for parent, inside, outside in ((X, (lo_left, hi_left), (lo_right, hi_right)), (Y, (lo_right, hi_right), (lo_left, hi_left))):
            for e in inside:
                assert joined(plan, probe_write(flat(parent), e), bases), (parent is X, e)
                assert not joined(plan, probe_read(flat(parent), e), bases), (parent is X, e)
            assert not joined(plan, probe_write(flat(parent), outside[0] if outside[0] else outside[1]), bases)
            assert not joined(plan, probe_write(flat(parent), inside[1] + 1 if inside[1] + 1 < n * n else inside[0] - 1), bases)
        for e in (0, D.size - 1):
            assert joined(plan, probe_write(flat(D2), e), bases) and joined(plan, probe_read(flat(D2), e), bases)
            assert not joined(plan, probe_write(flat(D), e), bases) and not joined(plan, probe_read(flat(D), e), bases)
        for e in (0, n * n - 1):
            assert not joined(plan, probe_write(flat(P), e), bases)          # the planned parent: not touched by this execution
            assert joined(plan, probe_write(flat(P), e))                      # ... but by one recorded without bases
        plan.close()


def test_an_accumulating_contraction_group_reads_its_destinations():
    """C = C + A B' as a group of one: recorded behind a plan that writes C, its packet must acquire (it reads what the sequence
    wrote); with initop zero the old C is not read and nothing acquires.  A single plan's reduction always counts as reading."""
    from strided_jl_amd import _lib as L
    c = CC.Case("acc", (20, 24, 9), CC.MM, CC.TYPES["f64"], CC.CONTRACT)
    ops = c.build()
    Cv = S.StridedView(ops[0].parent, (20, 24), ops[0].strides[:2], ops[0].offset)
    writer = S.make_plan(lambda x: x, None, None, (20, 24), (Cv, S.StridedView(np.zeros((20, 24), order="F"))))
    for initop, want in ((None, [0, 1]), (("scale", 2.0), [0, 1]), ("zero", [0, 0]), (("const", 1.0), [0, 0])):
        built = [S.build_problem(c.f, c.op, initop, c.dims, S.promoteshape(c.dims, *ops), stream=0)]
        g = L.Group([b[0] for b in built], keepalive=built)
        q = S.Sequence().add(writer).add_group(g)
        assert q.components() == [0, 0] and q.fences()[0] == want, (initop, q.fences())
        with CC.option("contract", 2):
            plan = c.plan(ops, initop)
        assert S.Sequence().add(writer).add(plan).fences()[0] == [0, 1], initop
        plan.close()
