"""Reduction groups (SMR_GROUP_REDUCE), host side (no device): what smr_group_create accepts and refuses with the flag and without it,
the workgroups and the body of every member of the table of tests/group_reduce_cases.py against what the table states, describe(),
the footprint of a recorded reduction group, the `with S.group(reduce=True):` front with the launcher stubbed, and the table's own
expected values against the CPU oracle run member by member."""
import ctypes as C

import numpy as np
import pytest

import contract_cases as CC
import group_reduce_cases as GR
import oraclelib
import reduce_fuzz_cases as RF
import strided_jl_amd as S
from strided_jl_amd import _lib as L

ROWS = GR.table()
IDS = [r.name for r in ROWS]
FNAME = {"ident": "ident", "abs2": "abs2", "mul": "mul2"}
OLD_REFUSAL = "is a reduction, but not of the contraction shape"


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


def vec(a, lo, n, step=1):
    return S.StridedView(a, (n,), (step,), lo)


def elem(a, i, rank=1):
    """element i of `a` as the destination of a complete reduction of that rank"""
    return S.StridedView(a, (1,) * rank, (0,) * rank, i)


def red(x, out, i=0, f=lambda v: v, op="+", initop=None):
    """(problem, keepalive): out[i] = op(initop(out[i]), op over x of f)"""
    dest = elem(out, i, len(x.size))
    return S.build_problem(f, op, initop, x.size, S.promoteshape(x.size, dest, x), stream=0)


# ---- acceptance, layout, describe ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_every_row_is_accepted_with_the_workgroups_and_the_body_the_table_states(row):
    _, views = row.views()
    with CC.option("jit", 1 if row.jit is None else row.jit):
        g = row.group(views)
        d = g.describe()
    lay = g.layout()
    want = row.layout()
    assert len(lay) == len(want) == len(row.specs)
    for i, ((form, first, wgs, rank), (wform, wfirst, ww), sp) in enumerate(zip(lay, want, row.specs)):
        assert (form, first, wgs) == (wform, wfirst, ww), (row.name, i, sp.dims, (form, first, wgs), (wform, wfirst, ww), d)
        assert 1 <= rank <= len(sp.dims), (row.name, i, rank)
        assert ww == min(-(-sp.total // 4096), 64)
    grid = sum(sp.W for sp in row.specs)
    nvec = sum(sp.vec for sp in row.specs)
    parts = [sp.W for sp in row.specs if sp.W > 1]
    members, _ = row.build()   # the compute class's element size, from what the single planner says of member 0
    p0 = S.make_plan(row.fn(), row.op, members[0].initop, members[0].dims, views[0])
    es = {"f32": 4, "f64": 8, "c32": 8, "c64": 16, "i64": 8}[CC.field(p0.describe(), "ct").split("(")[0]]
    p0.close()
    assert d.startswith("family=group kind=reduce members=%d grid=%d vec=%d strided=%d " % (len(row.specs), grid, nvec, len(row.specs) - nvec)), d
    assert CC.field(d, "f") == ("prog" if row.needs_prog else FNAME[row.f]) and CC.field(d, "op") == row.op, d
    assert CC.field(d, "jit") == ("1" if row.needs_prog and (row.jit is None or row.jit) else "0"), d
    assert int(CC.field(d, "partials")) == len(parts) and int(CC.field(d, "scratch")) == sum(parts) * es + 4 * len(parts), d
    assert int(CC.field(d, "bytes")) == g.algorithmic_bytes > 0 and "independent=" not in d and "tile=" not in d and "linear=" not in d, d
    gi = row.group(views, independent=True)
    assert gi.describe().endswith(" independent=asserted") and gi.layout() == lay


@pytest.mark.parametrize("row", ROWS[::5], ids=IDS[::5])
def test_without_the_flag_the_same_members_are_refused_as_before(row):
    _, views = row.views()
    with pytest.raises(L.UnsupportedOnDevice) as e:
        row.group(views, reduce=False)
    assert "member 0" in str(e.value) and OLD_REFUSAL in str(e.value), str(e.value)


def test_the_table_covers_what_it_must():
    totals = {sp.total for r in ROWS for sp in r.specs}
    assert totals >= {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 262144, 262145, 4100, 4098, 4092}
    assert {sp.W for r in ROWS for sp in r.specs} >= {1, 2, 3, 64}
    assert any(len({sp.W for sp in r.specs}) >= 3 for r in ROWS)                      # members of unequal W in one group
    assert {len(r.specs) for r in ROWS} >= {1, 2, 257, 2049}
    assert {r.op for r in ROWS} == {"+", "*", "min", "max", "&", "|"}
    assert {r.kind for r in ROWS} == {"none", "zero", "scale", "const", "conj"}
    assert {r.t for r in ROWS} >= {"f32", "f64", "c32", "c64", "i32", "i64", "bool"} and any(r.mixed for r in ROWS) and any("i16" in r.in_types for r in ROWS)
    assert {r.f for r in ROWS} == {"ident", "abs2", "mul", "prog", "amc"} and {r.jit for r in ROWS} == {None, 0, 1}
    assert {len(sp.dims) for r in ROWS for sp in r.specs} == {1, 2, 3, 4}
    assert any(sp.dup for r in ROWS for sp in r.specs) and any(r.conjs[0] for r in ROWS) and any(r.dconj for r in ROWS)
    for t in ("f32", "f64"):   # both bodies, per type, at and above the vector threshold
        assert {sp.vec for r in ROWS if r.t == t and not r.mixed for sp in r.specs if sp.total >= 4096} == {True, False}


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def test_flag_four_is_still_unknown_and_eight_is_the_reduction_group():
    x, out = np.zeros(50), np.zeros(4)
    p = [red(vec(x, 0, 50), out)]
    assert L.SMR_GROUP_REDUCE == 8
    for flags in (4, 4 | 8, 16, 8 | 32):
        rc, msg = create(p, flags)
        assert rc == L.SMR_EINVAL and "unknown flag" in msg, (flags, msg)
    for flags in (8, 8 | 1):
        assert create(p, flags) == (0, "")
    rc, msg = create(p, 0)
    assert rc == L.SMR_EUNSUPPORTED and OLD_REFUSAL in msg, msg
    rc, msg = create(p, 8 | 2)
    assert rc == L.SMR_EUNSUPPORTED and "SMR_GROUP_MEMBER_SCALARS" in msg and "reduction group" in msg, msg


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_member():
    x, y, out = np.zeros(60), np.zeros(60), np.zeros(8)
    ok = lambda i, **kw: red(vec(x, 0, 50), out, i, **kw)   # noqa: E731
    a = S.StridedView(np.zeros((6, 5), order="F"))
    amap = S.build_problem(lambda v: v, None, None, a.size, (a.similar(), a), stream=0)
    rc, msg = create([ok(0), ok(1), amap], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 2" in msg and "map" in msg and "complete" in msg, msg
    rc, msg = create([amap], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 0" in msg and "complete" in msg, msg
    # a kept dim of extent > 1: sum over the rows of a 6 x 5 matrix into 5 elements
    col = S.StridedView(np.zeros(5), (6, 5), (0, 1), 0)
    kept = S.build_problem(lambda v: v, "+", None, a.size, (col, a), stream=0)
    rc, msg = create([ok(0), kept], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "complete" in msg, msg
    rc, msg = create([kept], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 0" in msg and "complete" in msg, msg
    # ... of extent 1 is no kept dim
    one = S.StridedView(np.zeros(5), (6, 1), (0, 1), 2)
    a1 = S.StridedView(np.zeros((6, 1), order="F"))
    assert create([S.build_problem(lambda v: v, "+", None, a1.size, (one, a1), stream=0)], 8) == (0, "")
    rc, msg = create([ok(0), ok(1), ok(2, op="max")], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 2" in msg and "op" in msg, msg
    rc, msg = create([ok(0, initop=("scale", 2)), ok(1, initop="zero")], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "initop" in msg, msg
    assert create([ok(0, initop=("scale", 2)), ok(1, initop=("scale", -3))], 8) == (0, "")      # beta is the member's own
    rc, msg = create([ok(0), ok(1, f=lambda v: v * 2)], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "f" in msg, msg
    rc, msg = create([ok(0, f=lambda v: v * 2), ok(1, f=lambda v: v * 3)], 8)                    # the constants belong to the program
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "constants" in msg, msg
    two = S.build_problem(lambda u, v: u * v, "+", None, (50,), S.promoteshape((50,), elem(out, 3), vec(x, 0, 50), vec(y, 0, 50)), stream=0)
    rc, msg = create([ok(0), two], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg, msg
    x32 = np.zeros(60, dtype=np.float32)
    rc, msg = create([ok(0), red(vec(x32, 0, 50), np.zeros(4, dtype=np.float32))], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg, msg
    # overlapping destinations: the same element twice; a destination inside another member's input
    rc, msg = create([ok(0), ok(0)], 8)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "SMR_GROUP_INDEPENDENT" in msg, msg
    assert create([ok(0), ok(0)], 8 | 1) == (0, "")
    rc, msg = create([ok(0), red(vec(out, 0, 1), out, 5)], 8)
    assert rc == L.SMR_EUNSUPPORTED and "meets a byte range" in msg, msg
    assert create([ok(i) for i in range(8)], 8) == (0, "")
    rc, msg = create([ok(0)] * 65536, 8)
    assert rc == L.SMR_EINVAL and "count" in msg, msg


# ---- the footprint of a recorded reduction group ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("initop,reads", [(None, True), (("scale", 2), True), ("conj", True), ("zero", False), (("const", 3), False)])
def test_the_destination_is_read_unless_the_initop_replaces_it(initop, reads):
    x, out, src = np.zeros(100), np.zeros(4), np.zeros(4)
    ps = [red(vec(x, 50 * i, 50), out, i, initop=initop) for i in range(2)]
    g = L.Group([p[0] for p in ps], keepalive=ps, reduce=True)
    q = S.Sequence().add_group(g)
    assert q.components() == [0]
    acq, fp, resident = q.fences()
    assert acq == [1 if reads else 0] and fp == 100 * 8 + 2 * 8     # (an accumulating item reads what its own earlier replay wrote)
    # a plan that writes the destinations first: the group acquires only when it reads them
    writer = S.make_plan(lambda v: v, None, None, (4,), (vec(out, 0, 4), vec(src, 0, 4)))
    q = S.Sequence().add(writer).add_group(g)
    assert q.components() == [0, 0]
    assert q.fences()[0][1] == (1 if reads else 0)
    # one that writes an input: the group acquires whatever the initop
    wx = S.make_plan(lambda v: v, None, None, (4,), (vec(x, 10, 4), vec(src, 0, 4)))
    assert S.Sequence().add(wx).add_group(g).fences()[0] == [0, 1]
    # a reader of a destination joins the group
    reader = S.make_plan(lambda v: v, None, None, (1,), (vec(src, 0, 1), vec(out, 1, 1)))
    assert S.Sequence().add_group(g).add(reader).components() == [0, 0]
    assert S.Sequence().add_group(g).add(reader).fences()[0] == [1 if reads else 0, 1]


# ---- the front -------------------------------------------------------------------------------------------------------------------------
class Recorder(S.group):
    """`S.group` with the launcher stubbed out (tests/test_group_front_model.py): records the deferred calls of every launch."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.launches = []

    def _launch(self, calls, stream):
        self.launches.append(list(calls))


def test_front_buckets_by_op_initop_kind_and_constants():
    K = 6
    xs = [np.zeros(30 + i) for i in range(K)]
    out = np.zeros(K)
    arr = lambda i: S.promoteshape((xs[i].size,), elem(out, i), vec(xs[i], 0, xs[i].size))   # noqa: E731
    ident = lambda v: v          # noqa: E731
    g = Recorder(reduce=True)
    assert g.reduce and not g.contract
    assert g.defer(ident, (xs[0].size,), arr(0), "+", None, complete=True)
    assert g.defer(ident, (xs[1].size,), arr(1), "+", None, complete=True)
    assert g.defer(ident, (xs[2].size,), arr(2), "max", None, complete=True)                    # another op
    assert g.defer(ident, (xs[3].size,), arr(3), "+", ("scale", 2), complete=True)              # another kind of initop
    assert g.defer(ident, (xs[4].size,), arr(4), "+", ("scale", 5), complete=True)              # beta is per member
    assert g.defer(lambda v: v * 2, (xs[5].size,), arr(5), "+", None, complete=True)            # another f
    g.flush()
    assert [len(x) for x in g.launches] == [2, 1, 2, 1]
    assert all(c.kind == "reduce" for launch in g.launches for c in launch)
    # constants always belong to the key, whatever member_scalars says
    g = Recorder(reduce=True, member_scalars=True)
    assert g.defer(lambda v: v * 2, (xs[0].size,), arr(0), "+", None, complete=True)
    assert g.defer(lambda v: v * 3, (xs[1].size,), arr(1), "+", None, complete=True)
    assert g.defer(lambda v: v * 2, (xs[2].size,), arr(2), "+", None, complete=True)
    g.flush()
    assert [len(x) for x in g.launches] == [2, 1]
    # every bucket the front forms is a group the library accepts
    for launch in g.launches:
        built = [S.build_problem(c.f, c.op, c.initop, c.dims, c.arrays, stream=0) for c in launch]
        grp = L.Group([b[0] for b in built], keepalive=built, reduce=True)
        assert "kind=reduce members=%d " % len(launch) in grp.describe()


def test_front_defers_complete_reductions_only():
    x, out = np.zeros((6, 5), order="F"), np.zeros(8)
    xv = S.StridedView(x)
    g = Recorder(reduce=True)
    ident = lambda v: v   # noqa: E731
    # a destination of one element: every stride 0 or extent 1
    assert g.defer(ident, (6, 5), (elem(out, 0, 2), xv), "+", None, complete=True)
    assert g.defer(ident, (6, 1), (S.StridedView(out, (6, 1), (0, 1), 1), S.StridedView(x, (6, 1), (1, 6), 0)), "+", None, complete=True)
    # a kept dim: not deferred
    assert not g.defer(ident, (6, 5), (S.StridedView(out, (6, 5), (0, 1), 0), xv), "+", None, complete=True)
    # above group_max_bytes: not deferred
    with CC.option("group_max_bytes", 64):
        assert not g.defer(ident, (6, 5), (elem(out, 2, 2), xv), "+", None, complete=True)
    assert len(g.pending) == 2
    # a conflicting call flushes first: the same destination element again
    assert g.defer(ident, (6, 5), (elem(out, 0, 2), xv), "+", None, complete=True)
    assert [len(z) for z in g.launches] == [2] and len(g.pending) == 1


def test_reduce_false_still_flushes_and_the_funnel_routes_by_the_flags(monkeypatch):
    import sys
    MR = sys.modules["strided_jl_amd.mapreduce"]
    x, out = np.zeros(40), np.zeros(4)
    ran = []

    class FakeView:
        """forwards to a host view and claims to be on the device (nothing is launched: smr_mapreduce is stubbed)"""

        def __init__(self, v):
            self._v = v

        on_device = True

        def __getattr__(self, k):
            return getattr(self._v, k)

    monkeypatch.setattr(MR, "_SMR_MAPREDUCE", lambda p: ran.append(1) or 0)
    arrays = lambda i: tuple(FakeView(v) for v in S.promoteshape((40,), elem(out, i), vec(x, 0, 40)))   # noqa: E731
    ident = lambda v: v   # noqa: E731
    for kw, deferred in (({}, False), ({"contract": True}, False), ({"reduce": True}, True), ({"reduce": True, "contract": True}, True)):
        g = Recorder(**kw)
        with g:
            pend = S.StridedView(np.zeros(8))
            assert g.defer(ident, (8,), (pend.similar(), pend))       # a pending map
            del ran[:]
            MR._mapreduce_fuse_(ident, "+", None, (40,), arrays(0))
            if deferred:
                assert not ran and len(g.pending) == 2 and not g.launches
            else:
                assert ran == [1] and not g.pending and [len(z) for z in g.launches] == [1]   # flushed what was pending, then ran alone
        kinds = [[c.kind for c in launch] for launch in g.launches]
        assert kinds == ([["map"], ["reduce"]] if deferred else [["map"]]), (kw, kinds)


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
        err = GR.mismatch(row, dpar, row.expected_parent(times), "oracle, %d threads, %d applications" % (nthreads, times))
        assert err is None, err
