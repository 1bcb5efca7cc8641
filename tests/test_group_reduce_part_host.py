"""Partial reduction groups (SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART), host side (no device): what smr_group_create accepts and
refuses with the flag and without it, the lanes per destination element and the workgroups of every member of the table of
tests/group_reduce_part_cases.py against what the table states and against the single planner's general form, describe(), the
footprint of a recorded group, the `with S.group(reduce=True, reduce_part=True):` front with the launcher stubbed, and the table's own
expected values against the CPU oracle run member by member."""
import ctypes as C

import numpy as np
import pytest

import contract_cases as CC
import group_reduce_part_cases as GP
import oraclelib
import reduce_fuzz_cases as RF
import strided_jl_amd as S
from strided_jl_amd import _lib as L

ROWS = GP.table()
IDS = [r.name for r in ROWS]
FNAME = {"ident": "ident", "abs2": "abs2", "mul": "mul2"}
R, RP = 8, 8 | 256


def create(problems, flags=0):
    """(status, message) of smr_group_create on a list of (problem, keepalive)."""
    lib = L.load()
    arr = (L.smr_problem * max(1, len(problems)))()
    for i, (p, _) in enumerate(problems):
        C.memmove(C.byref(arr[i]), C.byref(p), C.sizeof(L.smr_problem))
    h = C.c_void_p()
    rc = lib.smr_group_create(arr, len(problems), flags, C.byref(h))
    msg = lib.smr_last_error().decode() if rc else ""
    if rc == 0:
        lib.smr_group_destroy(h)
    return rc, msg


def rowsum(a, out, lo=0, f=lambda v: v, op="+", initop=None):
    """(problem, keepalive): out[lo + i] = op(initop(out[lo + i]), op over j of f(a[i, j])) for a column-major n x m matrix `a`"""
    n, m = a.shape
    dest = S.StridedView(out, (n, m), (1, 0), lo)
    return S.build_problem(f, op, initop, (n, m), (dest, S.StridedView(a)), stream=0)


def mat(n=6, m=5, dtype=np.float64):
    return np.zeros((n, m), dtype=dtype, order="F")


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def test_flag_256_makes_a_partial_reduction_group_and_is_valid_only_with_flag_8():
    a, out = mat(), np.zeros(16)
    p = [rowsum(a, out)]
    assert L.SMR_GROUP_REDUCE_PART == 256 and L.SMR_GROUP_REDUCE == 8
    for flags in (RP, RP | 1):
        assert create(p, flags) == (0, ""), flags
    rc, msg = create(p, 256)
    assert rc == L.SMR_EUNSUPPORTED and "SMR_GROUP_REDUCE_PART" in msg and "SMR_GROUP_REDUCE" in msg, msg
    rc, msg = create(p, 256 | 1)
    assert rc == L.SMR_EUNSUPPORTED and "SMR_GROUP_REDUCE_PART" in msg, msg
    rc, msg = create(p, RP | 2)
    assert rc == L.SMR_EUNSUPPORTED and "SMR_GROUP_MEMBER_SCALARS" in msg and "reduction group" in msg, msg
    rc, msg = create(p, RP | 64)
    assert rc == L.SMR_EUNSUPPORTED and "SMR_GROUP_CONTRACT_SCALARS" in msg and "reduction group" in msg, msg
    for flags in (4, 16, 32, 128, 512, RP | 4, RP | 16, RP | 32, RP | 128, RP | 512):
        rc, msg = create(p, flags)
        assert rc == L.SMR_EINVAL and "unknown flag" in msg, (flags, msg)
    # flag 8 alone: a kept dim is refused as before
    rc, msg = create(p, R)
    assert rc == L.SMR_EUNSUPPORTED and "member 0" in msg and "complete" in msg and "keeps a dim" in msg, msg
    rc, msg = create(p, 0)
    assert rc == L.SMR_EUNSUPPORTED and "is a reduction, but not of the contraction shape" in msg, msg


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_member():
    a, b, out = mat(), mat(), np.zeros(64)
    ok = lambda i, **kw: rowsum(a, out, 8 * i, **kw)   # noqa: E731
    av = S.StridedView(a)
    amap = S.build_problem(lambda v: v, None, None, av.size, (av.similar(), av), stream=0)
    rc, msg = create([ok(0), ok(1), amap], RP)
    assert rc == L.SMR_EUNSUPPORTED and "member 2" in msg and "map" in msg and "SMR_GROUP_REDUCE_PART" in msg, msg
    rc, msg = create([amap], RP)
    assert rc == L.SMR_EUNSUPPORTED and "member 0" in msg and "map" in msg, msg
    rc, msg = create([ok(0), ok(1), ok(2, op="max")], RP)
    assert rc == L.SMR_EUNSUPPORTED and "member 2" in msg and "op" in msg, msg
    rc, msg = create([ok(0, initop=("scale", 2)), ok(1, initop="zero")], RP)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "initop" in msg, msg
    assert create([ok(0, initop=("scale", 2)), ok(1, initop=("scale", -3))], RP) == (0, "")      # beta is the member's own
    rc, msg = create([ok(0), ok(1, f=lambda v: v * 2)], RP)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "f" in msg, msg
    rc, msg = create([ok(0, f=lambda v: v * 2), ok(1, f=lambda v: v * 3)], RP)                    # the constants belong to the program
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "constants" in msg, msg
    dest = S.StridedView(out, (6, 5), (1, 0), 24)
    two = S.build_problem(lambda u, v: u * v, "+", None, (6, 5), (dest, S.StridedView(a), S.StridedView(b)), stream=0)
    rc, msg = create([ok(0), two], RP)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "operands" in msg, msg
    rc, msg = create([ok(0), rowsum(mat(dtype=np.float32), np.zeros(8, dtype=np.float32))], RP)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg, msg
    # which dims are kept is the member's own: a column sum, a complete reduction and an accumulating map next to a row sum
    colsum = S.build_problem(lambda v: v, "+", None, (6, 5), (S.StridedView(out, (6, 5), (0, 1), 16), S.StridedView(a)), stream=0)
    total = S.build_problem(lambda v: v, "+", None, (6, 5), (S.StridedView(out, (6, 5), (0, 0), 30), S.StridedView(a)), stream=0)
    accum = S.build_problem(lambda v: v, "+", None, (6, 5), (S.StridedView(out, (6, 5), (1, 6), 32), S.StridedView(a)), stream=0)
    assert create([ok(0), colsum, total, accum], RP) == (0, "")
    # overlapping destinations: the same window twice; interleaved windows (bounding ranges meet); a destination inside an input
    rc, msg = create([ok(0), ok(0)], RP)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "SMR_GROUP_INDEPENDENT" in msg, msg
    assert create([ok(0), ok(0)], RP | 1) == (0, "")
    even = S.build_problem(lambda v: v, "+", None, (6, 5), (S.StridedView(out, (6, 5), (2, 0), 40), S.StridedView(a)), stream=0)
    odd = S.build_problem(lambda v: v, "+", None, (6, 5), (S.StridedView(out, (6, 5), (2, 0), 41), S.StridedView(a)), stream=0)
    rc, msg = create([even, odd], RP)
    assert rc == L.SMR_EUNSUPPORTED and "meets a byte range" in msg and "SMR_GROUP_INDEPENDENT" in msg, msg
    assert create([even, odd], RP | 1) == (0, "")
    inside = S.build_problem(lambda v: v, "+", None, (6, 5), (S.StridedView(a.reshape(-1, order="F"), (6, 5), (1, 0), 0), S.StridedView(b)), stream=0)
    rc, msg = create([ok(0), inside], RP)
    assert rc == L.SMR_EUNSUPPORTED and "meets a byte range" in msg, msg
    assert create([ok(i) for i in range(8)], RP) == (0, "")
    rc, msg = create([ok(0)] * 65536, RP)
    assert rc == L.SMR_EINVAL and "count" in msg, msg


# ---- acceptance, layout, describe ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_every_row_is_accepted_with_the_lanes_and_the_workgroups_the_table_states(row):
    _, views = row.views()
    with CC.option("jit", 1 if row.jit is None else row.jit):
        g = row.group(views)
        d = g.describe()
    lay, lanes = g.layout(), g.lanes()
    want = row.layout()
    assert len(lay) == len(want) == len(lanes) == len(row.specs)
    for i, ((form, first, wgs, rank), (wform, wfirst, ww), tr, sp) in enumerate(zip(lay, want, lanes, row.specs)):
        assert (form, first, wgs, tr) == (wform, wfirst, ww, sp.tr), (row.name, i, sp.dims, sp.rdims, (form, first, wgs, tr), (wform, wfirst, ww, sp.tr), d)
        assert 1 <= rank <= len(sp.dims), (row.name, i, rank)
        assert ww == -(-sp.nout // (256 // sp.tr)) and sp.tr in (1, 2, 4, 8, 16, 32, 64, 128, 256)
    grid = sum(sp.W for sp in row.specs)
    assert d.startswith("family=group kind=reduce_part members=%d grid=%d lanes=%s f=" % (len(row.specs), grid, row.lanes_token())), d
    assert CC.field(d, "f") == ("prog" if row.needs_prog else FNAME[row.f]) and CC.field(d, "op") == row.op, d
    assert CC.field(d, "jit") == ("1" if row.needs_prog and (row.jit is None or row.jit) else "0"), d
    assert int(CC.field(d, "bytes")) == g.algorithmic_bytes > 0, d
    assert all(tok not in d for tok in ("independent=", "tile=", "linear=", "partials=", "scratch=", "vec=")), d
    gi = row.group(views, independent=True)
    assert gi.describe().endswith(" independent=asserted") and gi.layout() == lay and gi.lanes() == lanes


@pytest.mark.parametrize("row", ROWS[::6], ids=IDS[::6])
def test_without_flag_256_the_same_members_are_refused_as_before(row):
    _, views = row.views()
    with pytest.raises(L.UnsupportedOnDevice) as e:
        row.group(views, reduce=False, reduce_part=False)
    assert "member 0" in str(e.value) and "is a reduction, but not of the contraction shape" in str(e.value), str(e.value)
    if any(sp.nout > 1 for sp in row.specs):
        with pytest.raises(L.UnsupportedOnDevice) as e:
            row.group(views, reduce=True, reduce_part=False)
        assert "complete" in str(e.value), str(e.value)


def covered_by_the_guarantee(row, m, view):
    """the single plan's description of member m under reduce_part_kind = 0 when it reads form=general ... split=1, else None"""
    with CC.option("reduce_part_kind", 0), CC.option("jit", 1 if row.jit is None else row.jit):
        p = S.make_plan(row.fn(), row.op, m.initop, m.dims, view)
        d = p.describe()
        p.close()
    if d.startswith("family=reduce_part ") and CC.field(d, "form") == "general" and CC.field(d, "split") == "1":
        return d
    return None


def test_lanes_and_workgroups_are_the_single_plans_general_form():
    covered = left_out = 0
    reasons = set()
    for row in ROWS:
        if len(row.specs) > 300:
            continue
        members, _ = row.build()
        _, views = row.views()
        lanes = row.group(views).lanes()
        for m, v, tr in zip(members, views, lanes):
            d = covered_by_the_guarantee(row, m, v)
            if d is None:   # the three cases without an identity claim: one destination element, no reduced dim, a split single plan
                left_out += 1
                reasons.add("one element" if m.spec.nout == 1 else ("no reduced dim" if m.spec.red == 1 else "split"))
                assert m.spec.nout == 1 or m.spec.red == 1 or m.spec.red >= 256 * m.spec.tr, (row.name, m.spec.dims, m.spec.rdims)
                continue
            covered += 1
            assert int(CC.field(d, "lanes_per_out")) == tr == m.spec.tr and int(CC.field(d, "nout")) == m.spec.nout, (row.name, m.spec.dims, d, tr)
    # (a member with no reduced dim reads form=general ... split=1 in a single call as well: it is compared like the others)
    assert covered >= 300 and "one element" in reasons and "split" not in reasons, (covered, left_out, reasons)


@pytest.mark.parametrize("t", ["f32", "f64", "c64"])
def test_the_guarantee_covers_every_member_of_the_order_rows(t):
    """tests/test_gpu_group_reduce_part.py compares these members bit for bit with the single calls: none may be left out."""
    row = GP.order_row(t)
    members, _ = row.build()
    _, views = row.views()
    g = row.group(views)
    assert g.lanes() == [sp.tr for sp in row.specs] and [r[2] for r in g.layout()] == [sp.W for sp in row.specs]
    assert {sp.tr for sp in row.specs} == {1, 2, 32, 64, 128, 256} and all(sp.red % sp.tr for sp in row.specs if sp.tr > 1)
    assert all(sp.W > 1 and (sp.ob == 1 or sp.nout % sp.ob) for sp in row.specs)   # the last workgroup has dead lanes
    forms = set()
    for m, v in zip(members, views):
        d = covered_by_the_guarantee(row, m, v)
        assert d is not None and int(CC.field(d, "lanes_per_out")) == m.spec.tr, (m.spec.dims, m.spec.rdims, d)
        p = S.make_plan(row.fn(), row.op, m.initop, m.dims, v)
        forms.add(CC.field(p.describe(), "form"))
        p.close()
    assert forms & {"row", "col"}, forms   # the default planner takes other forms: the GPU test's control


def test_the_table_covers_what_it_must():
    specs = [sp for r in ROWS for sp in r.specs]
    assert {sp.red for sp in specs} >= set(GP.REDS)
    assert {sp.tr for sp in specs} == {1, 2, 4, 8, 16, 32, 64, 128, 256}
    assert any(sp.red % sp.tr for sp in specs if sp.tr > 1)
    for red in GP.REDS:   # per reduced length: one output, a workgroup less one, exactly one, one more, several workgroups
        ob = 256 // GP.lanes_small(red)
        assert {sp.nout for sp in specs if sp.red == red} >= {1, max(1, ob - 1), ob, ob + 1, 2 * ob + 1}, red
    wide = [sp for sp in specs if sp.dims == (256, 256, 3) and sp.rdims == (2,)]
    assert wide and (wide[0].nout, wide[0].tr, wide[0].W) == (65536, 1, 256) and wide[0].lays[0][0][0] == 0
    assert {len(sp.kept) for sp in specs} >= {0, 1, 2, 3} and {len(sp.rdims) for sp in specs} >= {0, 1, 2, 3}
    for N, rd in ((3, (0,)), (3, (1,)), (3, (0, 2)), (3, (1, 2)), (4, (0,)), (4, (1,)), (4, (0, 2)), (4, (1, 2))):   # dims=1, 2, (1,3), (2,3) in Julia's counting
        assert any(len(sp.dims) == N and sp.rdims == rd for sp in specs), (N, rd)
    dl = [sp.dlay for sp in specs if sp.kept]
    assert any(tuple(p) != tuple(range(len(p))) for p, _, _, _ in dl) and any(any(s > 1 for s in st) for _, _, _, st in dl) and any(any(s < 0 for s in st) for _, _, _, st in dl)
    assert any(sp.kept and set(bd) & set(sp.kept) for sp in specs for _, _, _, _, bd in sp.lays), "an input broadcast along a kept dim"
    assert any(set(bd) & set(sp.rdims) for sp in specs for _, _, _, _, bd in sp.lays), "an input broadcast along a reduced dim"
    assert any(r.conjs[0] for r in ROWS) and any(r.dconj for r in ROWS) and any(sp.dup for sp in specs)
    assert any(not sp.rdims for sp in specs) and any(not sp.kept for sp in specs)
    assert {len(r.specs) for r in ROWS} >= {1, 2, 257, 2049}
    assert any(len({sp.tr for sp in r.specs}) >= 4 and len({len(sp.dims) for sp in r.specs}) >= 3 and len({sp.W for sp in r.specs}) >= 3 for r in ROWS)
    assert {r.op for r in ROWS} == {"+", "*", "min", "max", "&", "|"}
    assert {r.kind for r in ROWS} == {"none", "zero", "scale", "const", "conj"}
    assert {r.t for r in ROWS} >= {"f32", "f64", "c32", "c64", "i32", "i64", "bool"} and any(r.mixed for r in ROWS) and any("i16" in r.in_types for r in ROWS)
    assert {r.f for r in ROWS} == {"ident", "abs2", "mul", "prog", "amc"} and {r.jit for r in ROWS} == {None, 0, 1}
    assert 30 <= len(ROWS) <= 40


# ---- the footprint of a recorded group ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("initop,reads", [(None, True), (("scale", 2), True), ("conj", True), ("zero", False), (("const", 3), False)])
def test_the_footprint_is_the_bounding_ranges_and_the_destination_is_read_unless_the_initop_replaces_it(initop, reads):
    a, b, out, src = mat(), mat(), np.zeros(64), np.zeros(64)
    # member 0 writes out[8:19:2] (6 elements, stepped), member 1 out[30:36]: bounding ranges [8, 19) and [30, 36)
    p0 = S.build_problem(lambda v: v, "+", initop, (6, 5), (S.StridedView(out, (6, 5), (2, 0), 8), S.StridedView(a)), stream=0)
    p1 = S.build_problem(lambda v: v, "+", initop, (6, 5), (S.StridedView(out, (6, 5), (1, 0), 30), S.StridedView(b)), stream=0)
    g = L.Group([p0[0], p1[0]], keepalive=(p0, p1), reduce=True, reduce_part=True)
    q = S.Sequence().add_group(g)
    assert q.components() == [0]
    acq, fp, resident = q.fences()
    assert acq == [1 if reads else 0] and fp == 2 * 30 * 8 + (11 + 6) * 8
    vec = lambda arr, lo, n: S.StridedView(arr, (n,), (1,), lo)   # noqa: E731
    copy = lambda dst, lo, n: S.make_plan(lambda v: v, None, None, (n,), (vec(dst, lo, n), vec(src, 0, n)))   # noqa: E731
    # probes that write one element at and next to the lowest and the highest destination element: inside the bounding range the probe
    # joins the group's component, outside they are independent; the group acquires only when it reads its destination (an accumulating
    # item reads what its own earlier replay wrote, whatever the probe did)
    for lo, meets in ((7, False), (8, True), (9, True), (18, True), (19, False), (29, False), (30, True), (35, True), (36, False)):
        q = S.Sequence().add(copy(out, lo, 1)).add_group(g)
        assert q.components() == ([0, 0] if meets else [0, 1]), (lo, q.components())
        assert q.fences()[0][1] == (1 if reads else 0), (lo, q.fences())
    # ... of the inputs: whatever the initop, the group acquires what a probe wrote inside an input
    fa = a.reshape(-1, order="F")
    for arr, lo, meets in ((fa, 0, True), (fa, 29, True), (out, 0, False)):
        q = S.Sequence().add(copy(arr, lo, 1)).add_group(g)
        assert q.fences()[0][1] == (1 if meets or reads else 0), (lo, q.fences())
        assert q.components() == ([0, 0] if meets else [0, 1]), (lo, q.components())
    # a reader of a destination element joins the group
    reader = S.make_plan(lambda v: v, None, None, (1,), (vec(src, 0, 1), vec(out, 18, 1)))
    assert S.Sequence().add_group(g).add(reader).components() == [0, 0]
    outside = S.make_plan(lambda v: v, None, None, (1,), (vec(src, 0, 1), vec(out, 19, 1)))
    assert S.Sequence().add_group(g).add(outside).components() == [0, 1]


# ---- the front -------------------------------------------------------------------------------------------------------------------------
class Recorder(S.group):
    """`S.group` with the launcher stubbed out (tests/test_group_front_model.py): records the deferred calls of every launch."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.launches = []

    def _launch(self, calls, stream):
        self.launches.append(list(calls))


def test_reduce_part_needs_reduce():
    with pytest.raises(ValueError):
        S.group(reduce_part=True)
    with pytest.raises(L.UnsupportedOnDevice):
        a, out = mat(), np.zeros(8)
        p = rowsum(a, out)
        L.Group([p[0]], keepalive=[p], reduce_part=True)
    g = S.group(reduce=True, reduce_part=True)
    assert g.reduce and g.reduce_part and not S.group(reduce=True).reduce_part


def test_front_buckets_by_op_initop_kind_and_constants():
    K = 6
    mats = [mat(4 + i, 5) for i in range(K)]
    out = np.zeros(16 * K)
    arr = lambda i: (S.StridedView(out, mats[i].shape, (1, 0), 16 * i), S.StridedView(mats[i]))   # noqa: E731
    ident = lambda v: v          # noqa: E731
    g = Recorder(reduce=True, reduce_part=True)
    assert g.defer(ident, mats[0].shape, arr(0), "+", None, part=True)
    assert g.defer(ident, mats[1].shape, arr(1), "+", None, part=True)
    assert g.defer(ident, mats[2].shape, arr(2), "max", None, part=True)                    # another op
    assert g.defer(ident, mats[3].shape, arr(3), "+", ("scale", 2), part=True)              # another kind of initop
    assert g.defer(ident, mats[4].shape, arr(4), "+", ("scale", 5), part=True)              # beta is per member
    assert g.defer(lambda v: v * 2, mats[5].shape, arr(5), "+", None, part=True)            # another f
    g.flush()
    assert [len(x) for x in g.launches] == [2, 1, 2, 1]
    assert all(c.kind == "reduce_part" and c.bucket[-3] == "reduce_part" for launch in g.launches for c in launch)
    # constants always belong to the key, whatever member_scalars says
    g = Recorder(reduce=True, reduce_part=True, member_scalars=True)
    assert g.defer(lambda v: v * 2, mats[0].shape, arr(0), "+", None, part=True)
    assert g.defer(lambda v: v * 3, mats[1].shape, arr(1), "+", None, part=True)
    assert g.defer(lambda v: v * 2, mats[2].shape, arr(2), "+", None, part=True)
    g.flush()
    assert [len(x) for x in g.launches] == [2, 1]
    # every bucket the front forms is a group the library accepts
    for launch in g.launches:
        built = [S.build_problem(c.f, c.op, c.initop, c.dims, c.arrays, stream=0) for c in launch]
        grp = L.Group([b[0] for b in built], keepalive=built, reduce=True, reduce_part=True)
        assert "kind=reduce_part members=%d " % len(launch) in grp.describe()


def test_front_defers_within_group_max_bytes_and_flushes_on_a_conflict():
    a, out = mat(), np.zeros(32)
    av = S.StridedView(a)
    g = Recorder(reduce=True, reduce_part=True)
    ident = lambda v: v   # noqa: E731
    assert g.defer(ident, (6, 5), (S.StridedView(out, (6, 5), (1, 0), 0), av), "+", None, part=True)       # row sums
    assert g.defer(ident, (6, 5), (S.StridedView(out, (6, 5), (0, 1), 8), av), "+", None, part=True)       # column sums
    assert g.defer(ident, (6, 5), (S.StridedView(out, (6, 5), (0, 0), 14), av), "+", None, part=True)      # one element: a member as well
    with CC.option("group_max_bytes", 64):
        assert not g.defer(ident, (6, 5), (S.StridedView(out, (6, 5), (1, 0), 16), av), "+", None, part=True)
    assert len(g.pending) == 3
    # a conflicting call flushes first: the same destination window again
    assert g.defer(ident, (6, 5), (S.StridedView(out, (6, 5), (1, 0), 0), av), "+", None, part=True)
    assert [len(z) for z in g.launches] == [3] and len(g.pending) == 1
    # interleaved destinations (bounding ranges meet) flush unless the block is independent
    for independent, launches in ((False, [1]), (True, [])):
        g = Recorder(reduce=True, reduce_part=True, independent=independent)
        assert g.defer(ident, (6, 5), (S.StridedView(out, (6, 5), (2, 0), 0), av), "+", None, part=True)
        assert g.defer(ident, (6, 5), (S.StridedView(out, (6, 5), (2, 0), 1), av), "+", None, part=True)
        assert [len(z) for z in g.launches] == launches


def test_the_funnel_routes_by_the_flags_and_complete_reductions_keep_their_bucket(monkeypatch):
    import sys
    MR = sys.modules["strided_jl_amd.mapreduce"]
    a, out = mat(), np.zeros(32)
    ran = []

    class FakeView:
        """forwards to a host view and claims to be on the device (nothing is launched: smr_mapreduce is stubbed)"""

        def __init__(self, v):
            self._v = v

        on_device = True

        def __getattr__(self, k):
            return getattr(self._v, k)

    monkeypatch.setattr(MR, "_SMR_MAPREDUCE", lambda p: ran.append(1) or 0)
    partial = lambda: tuple(FakeView(v) for v in (S.StridedView(out, (6, 5), (1, 0), 0), S.StridedView(a)))        # noqa: E731
    complete = lambda: tuple(FakeView(v) for v in (S.StridedView(out, (6, 5), (0, 0), 20), S.StridedView(a)))      # noqa: E731
    ident = lambda v: v   # noqa: E731
    for kw, pdef, cdef in (({}, False, False), ({"contract": True}, False, False), ({"reduce": True}, False, True),
                           ({"reduce": True, "reduce_part": True}, True, True), ({"reduce": True, "reduce_part": True, "contract": True}, True, True)):
        g = Recorder(**kw)
        with g:
            del ran[:]
            MR._mapreduce_fuse_(ident, "+", None, (6, 5), complete())
            assert (not ran and len(g.pending) == 1) if cdef else (ran == [1] and not g.pending), kw
            del ran[:]
            MR._mapreduce_fuse_(ident, "+", None, (6, 5), partial())
            if pdef:
                assert not ran and len(g.pending) == 2 and not g.launches, kw
            else:   # reduce=True alone defers no partial reduction: it flushes what is pending and runs alone, as before
                assert ran == [1] and not g.pending, kw
        kinds = [[c.kind for c in launch] for launch in g.launches]
        assert kinds == ([["reduce"], ["reduce_part"]] if pdef else ([["reduce"]] if cdef else [])), (kw, kinds)


# ---- the table's expected values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_the_expected_values_are_the_oracles_member_by_member(row):
    members, parent = row.build()
    assert parent.ctypes.data % 64 == 0 and all(o.parent.ctypes.data % 64 == 0 for m in members for o in m.ins)
    for nthreads, times in ((1, 1), (4, RF.APPLICATIONS)) if len(members) <= 300 else ((1, 1),):
        dpar, views = row.views()
        ps = row.problems(views)
        for _ in range(times):
            for p, _keep in ps:
                oraclelib.mapreduce(p, nthreads)
        err = GP.mismatch(row, dpar, row.expected_parent(times), "oracle, %d threads, %d applications" % (nthreads, times))
        assert err is None, err
