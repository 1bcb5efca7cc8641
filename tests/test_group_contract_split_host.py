"""Split contraction groups, host side (no device): option "group_contract_split" -- its validation, that 0 leaves every plan of
tests/group_contract_cases.py as it is, the layout of every row of tests/group_contract_split_cases.py against the slice arithmetic
recomputed here, the clamp and the refusal above 2^31 bytes of partials, known answers of the group rule, the front's cache key
(launcher stubbed) and the footprint of a split group in a recorded sequence."""
import ctypes as C
import sys

import numpy as np
import pytest

import contract_cases as CC
import group_contract_cases as GC
import group_contract_split_cases as GS
import strided_jl_amd as S
from strided_jl_amd import _lib as L

MR = sys.modules["strided_jl_amd.mapreduce"]
ROWS = GS.table()
MUL = lambda a, b: a * b  # noqa: E731


def fresh(shape, dtype=np.float64):
    return S.StridedView(np.zeros(shape, dtype=dtype, order="F"))


def mul_problem(m, n, k, dt=np.float64, initop="zero"):
    """The generic product box over fresh host operands: C (m, n) = A (m, k) B (k, n)."""
    Cv, A, B = fresh((m, n), dt), fresh((m, k), dt), fresh((k, n), dt)
    A2 = S.StridedView(A.parent, (m, 1, k), (A.strides[0], 0, A.strides[1]), A.offset, A.op)
    B2 = S.StridedView(B.parent, (1, n, k), (0, B.strides[1], B.strides[0]), B.offset, B.op)
    C2 = S.StridedView(Cv.parent, (m, n, 1), (Cv.strides[0], Cv.strides[1], 0), Cv.offset, Cv.op)
    return S.build_problem(MUL, "+", initop, (m, n, k), S.promoteshape((m, n, k), C2, A2, B2), stream=0)


def group_of(problems, split, tile=0):
    with CC.option("group_contract_tile", tile), GS.split_option(split):
        return L.Group([p[0] for p in problems], keepalive=problems)


def create_status(problems, split, tile=0):
    lib = L.load()
    arr = (L.smr_problem * len(problems))()
    for i, (p, _) in enumerate(problems):
        C.memmove(C.byref(arr[i]), C.byref(p), C.sizeof(L.smr_problem))
    h = C.c_void_p()
    with CC.option("group_contract_tile", tile), GS.split_option(split):
        rc = lib.smr_group_create(arr, len(problems), 0, C.byref(h))
    msg = lib.smr_last_error().decode() if rc else ""
    if rc == 0:
        lib.smr_group_destroy(h)
    return rc, msg


# ---- the option ----------------------------------------------------------------------------------------------------------------------
def test_option_values():
    assert S.get_option("group_contract_split") == 0
    for v in (1, 2, 64, 1000, 2 ** 31 - 1, 0):
        S.set_option("group_contract_split", v)
        assert S.get_option("group_contract_split") == v
    lib = L.load()
    for v in (-1, -64, 2 ** 31, 2 ** 40):
        assert lib.smr_set_option(b"group_contract_split", v) == L.SMR_EINVAL
        assert "group_contract_split" in lib.smr_last_error().decode()
        assert S.get_option("group_contract_split") == 0


def test_setting_the_option_keeps_the_plan_cache_and_single_plans():
    """Read by smr_group_create only: a single call's plan does not change with it."""
    c = GS.row("f64/t16/n1_2tk_s2_vec").members[0]
    ops = c.build()
    with CC.option("contract", 2):
        p = c.plan(ops)
        d0 = p.describe()
        p.close()
        with GS.split_option(8):
            p = c.plan(ops)
            assert p.describe() == d0 and "kparts" not in d0
            p.close()


@pytest.mark.parametrize("row", GC.table(), ids=[r.name for r in GC.table()])
def test_with_the_option_at_zero_every_unsplit_row_plans_as_before(row):
    built = row.build()
    g = row.group(built)
    before = (g.describe(), g.layout())
    assert "split=" not in before[0] and g.split_layout() == []
    S.set_option("group_contract_split", 7)
    S.set_option("group_contract_split", 0)
    g0 = row.group(built)
    assert (g0.describe(), g0.layout()) == before and g0.split_layout() == []


def test_a_map_group_has_no_split_layout_and_ignores_the_option():
    a, b = fresh((40, 50)), fresh((40, 50))
    p = S.build_problem(lambda x: x, None, None, a.size, (a, b), stream=0)
    g = L.Group([p[0]], keepalive=[p])
    with GS.split_option(4):
        g4 = L.Group([p[0]], keepalive=[p])
    assert g4.describe() == g.describe() and g4.layout() == g.layout() and g4.split_layout() == []


# ---- the table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_layout_of_every_row_is_the_slice_arithmetic(row):
    built = row.build()
    g = row.group(built)
    unsplit = row.group(built, S=0)
    d, lay, sl = g.describe(), g.layout(), g.split_layout()
    assert int(CC.field(d, "tile")) == row.tile and len(lay) == len(sl) == len(row.members), d
    rb2 = (row.tile // 16) ** 2
    es = np.dtype({"bool": np.int64, "i32_i64": np.int64}.get(row.tn, row.dts[0])).itemsize
    first = fold_first = scratch = nsplit = 0
    for (form, f0, wgs, rank), (Si, cps, ff, fw), (nchunks, tiles), (_, _, uw, _) in zip(lay, sl, row.chunks(built), unsplit.layout()):
        want_s, want_cps = GS.cut(nchunks, row.S)
        assert (Si, cps) == (want_s, want_cps), (row.name, nchunks, Si, cps)
        assert uw == tiles and form == 2 and f0 == first and wgs == tiles * Si
        assert (Si - 1) * cps < nchunks <= Si * cps          # no slice is empty
        assert ff == fold_first and fw == (rb2 * tiles if Si >= 2 else 0)
        first += wgs
        fold_first += fw
        if Si >= 2:
            nsplit += 1
            scratch += tiles * Si * row.tile * row.tile * es
    assert nsplit >= 1 and any(s[0] == 1 for s in sl) == any(n == 1 for n, _ in row.chunks(built))
    assert int(CC.field(d, "grid")) == first and int(CC.field(d, "split")) == nsplit and int(CC.field(d, "kparts")) == max(s[0] for s in sl)
    assert CC.field(d, "fold") == "second-launch" and int(CC.field(d, "fold_grid")) == fold_first and int(CC.field(d, "scratch")) == scratch
    # everything in front of the split form's fields is the unsplit group's string, but for the grid
    ud = unsplit.describe()
    assert "split=" not in ud and unsplit.split_layout() == []
    head = d.split(" split=")[0]
    assert head.replace("grid=%d " % first, "grid=%s " % CC.field(ud, "grid")) == ud
    assert g.algorithmic_bytes == unsplit.algorithmic_bytes


def test_the_table_reaches_what_it_is_for():
    names = [r.name for r in ROWS]
    assert len(set(names)) == len(names)
    assert {len(r.members) for r in ROWS} >= {1, 3, 17, 257}
    assert {r.S for r in ROWS} >= {2, 3, 4, 64} and {r.tile for r in ROWS} == {16, 32}
    assert {r.kind for r in ROWS} >= {"zero", "none", "scale", "const", "conj"}
    assert {r.op for r in ROWS} >= {"+", "*", "min", "max", "&", "|"} and {r.fname for r in ROWS} >= {"mul", "dist", "and", "asym"}
    assert {r.tn for r in ROWS} >= {"f32", "f64", "c32", "c64", "i64", "i32_i64", "bool"}
    assert any(len({len(c.dims) for c in r.members}) > 1 for r in ROWS)          # members of different rank in one group
    assert any(any(c.conjs) for r in ROWS for c in r.members)
    mixed = GS.row("f64/t32/n17_mixed_s3")
    s = [x[0] for x in mixed.group(mixed.build()).split_layout()]
    assert s[0] == 1 and s[-1] == 1 and 1 in s[1:-1] and s[1] == 3               # unsplit members first, last and in between


def test_an_independent_group_keeps_its_tag_last():
    r = GS.row("f64/t16/n4_two_s2")
    d = r.group(r.build(), independent=True).describe()
    assert d.endswith(" independent=asserted") and " scratch=" in d and d.index(" split=") > d.index(" bytes=")


# ---- clamp and limits ----------------------------------------------------------------------------------------------------------------
def test_forced_slices_clamp_to_the_chunks():
    tk = GC.tk_of("f64")
    ps = [mul_problem(20, 24, 3 * tk + 1), mul_problem(20, 24, tk), mul_problem(20, 24, 2 * tk)]
    for S_, want in ((1000, [(4, 1), (1, 1), (2, 1)]), (3, [(2, 2), (1, 1), (2, 1)]), (2, [(2, 2), (1, 1), (2, 1)])):
        sl = group_of(ps, S_, 16).split_layout()
        assert [(s, c) for s, c, _, _ in sl] == want, (S_, sl)
    # nobody can take two slices: the unsplit group, whatever is forced
    g = group_of([mul_problem(20, 24, tk), mul_problem(17, 5, 3)], 64, 16)
    assert g.split_layout() == [] and "split=" not in g.describe()


def test_partials_above_two_gib_are_refused_when_forced():
    """ComplexF64 on 32 x 32 tiles: 16 KiB per (tile, slice); 16 members of (512, 512, K) have 4096 tiles, so 32 slices each are
    exactly 2^31 bytes (accepted) and 33 are beyond (refused when forced; the rule would leave such a group unsplit)."""
    tk = GC.tk_of("c64")
    ps = [mul_problem(512, 512, 32 * tk, np.complex128) for _ in range(16)]
    g = group_of(ps, 32, 32)
    assert int(CC.field(g.describe(), "scratch")) == 2 ** 31 and int(CC.field(g.describe(), "kparts")) == 32
    ps = [mul_problem(512, 512, 33 * tk, np.complex128) for _ in range(16)]
    assert int(CC.field(group_of(ps, 32, 32).describe(), "kparts")) == 17
    rc, msg = create_status(ps, 33, 32)
    assert rc == L.SMR_EUNSUPPORTED and "2^31 bytes" in msg, msg


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def test_rule_splits_sixteen_long_blocks():
    """16 x (32, 32, 4096) Float64: unsplit 64 workgroups of 16 x 16; the rule takes 32 x 32 tiles (16 tiles, up to 64 slices each)
    and ceil(512 / 16) = 32 slices per member."""
    ps = [mul_problem(32, 32, 4096) for _ in range(16)]
    assert CC.field(group_of(ps, 0).describe(), "grid") == "64"
    g = group_of(ps, 1)
    d = g.describe()
    assert CC.field(d, "tile") == "32" and CC.field(d, "grid") == "512" and CC.field(d, "split") == "16" and CC.field(d, "kparts") == "32", d
    assert [s[:2] for s in g.split_layout()] == [(32, 4)] * 16


def test_rule_leaves_many_small_blocks_and_full_devices_alone():
    small = [mul_problem(32, 32, 32) for _ in range(1024)]
    assert group_of(small, 1).describe() == group_of(small, 0).describe()
    # 256 unsplit workgroups and more: not looked at, however long the members
    long256 = [mul_problem(32, 32, 1024) for _ in range(64)]
    d0 = group_of(long256, 0).describe()
    assert int(CC.field(d0, "grid")) >= 256 and group_of(long256, 1).describe() == d0
    # single-chunk members only: nobody can take two slices
    tk = GC.tk_of("f64")
    few = [mul_problem(32, 32, tk) for _ in range(4)]
    assert group_of(few, 1).describe() == group_of(few, 0).describe()


def test_rule_splits_only_the_long_members_of_a_mixed_group():
    ps = [mul_problem(32, 32, 32) for _ in range(10)] + [mul_problem(32, 32, 16384) for _ in range(2)]
    g = group_of(ps, 1)
    sl = g.split_layout()
    assert [s[0] for s in sl[:10]] == [1] * 10 and all(s[0] >= 2 for s in sl[10:]), sl
    assert CC.field(g.describe(), "split") == "2"
    # a forced tile stays
    for tile in (16, 32):
        assert CC.field(group_of(ps, 1, tile).describe(), "tile") == str(tile)


def test_rule_honours_max_lds_bytes():
    ps = [mul_problem(32, 32, 4096) for _ in range(16)]
    lds16 = int(CC.field(group_of(ps, 0, 16).describe(), "lds"))
    with CC.option("max_lds_bytes", lds16):
        d = group_of(ps, 1).describe()
    assert CC.field(d, "tile") == "16" and "split=" in d, d


# ---- the front, with the launcher stubbed --------------------------------------------------------------------------------------------
@pytest.fixture
def host_front(monkeypatch):
    monkeypatch.setattr(S.StridedView, "on_device", property(lambda self: True))
    monkeypatch.setattr(MR, "_SMR_MAPREDUCE", lambda pp: 0)
    monkeypatch.setattr(MR, "_PROBLEM_CACHE", type(MR._PROBLEM_CACHE)())
    monkeypatch.setattr(MR, "_GROUP_CACHE", type(MR._GROUP_CACHE)())
    monkeypatch.setattr(L.Group, "execute", lambda self, stream=None: None)


def test_front_reads_the_option_into_the_buckets_cache_key(host_front):
    tk = GC.tk_of("f64")
    ms = [(fresh((20, 24)), fresh((20, 3 * tk + 1)), fresh((3 * tk + 1, 24))) for _ in range(3)]

    def block():
        with S.group(contract=True) as g:
            for i, (Cm, A, B) in enumerate(ms):
                S.mul_(Cm, A, B, 1, 2 + i)
        (grp,) = g.groups
        return grp

    g0 = block()
    assert "split=" not in g0.describe() and len(MR._GROUP_CACHE) == 1
    with GS.split_option(2):
        g2 = block()
        assert g2 is not g0 and CC.field(g2.describe(), "kparts") == "2" and len(MR._GROUP_CACHE) == 2
        assert block() is g2
    assert block() is g0 and len(MR._GROUP_CACHE) == 2
    keys = list(MR._GROUP_CACHE)
    assert keys[0][:-1] == keys[1][:-1] and {k[-1] for k in keys} == {(0, 0), (0, 2)}


# ---- a recorded sequence -------------------------------------------------------------------------------------------------------------
def test_the_footprint_of_a_split_group_is_the_unsplit_groups():
    tk = GC.tk_of("f64")
    ps = [mul_problem(16, 16, 2 * tk) for _ in range(3)]
    out = []
    for split in (0, 2):
        g = group_of(ps, split, 16)
        q = S.Sequence().add_group(g)
        out.append((q.components(), q.fences()))
        assert ("split=3" in g.describe()) == (split == 2)
    assert out[0] == out[1] and out[0][1][1] == 3 * (16 * 16 + 2 * 16 * 2 * tk) * 8


# ---- the scheduler: block ranges of a two-launch item whose second launch folds the first -------------------------------------------------
def test_schedule_cuts_a_fold_after_item_into_ranges_on_one_queue_with_the_fold_behind():
    import test_seq_schedule as TQ
    A, B, Cd = TQ.span(0), TQ.span(1), TQ.span(2)

    def item(fold_after=True, grid=300, nlaunch=2):
        e = TQ.ex([A, B, Cd], [Cd], nlaunch=nlaunch, grid=grid)
        e["sliceable"] = 3 if fold_after else 1   # smr_debug_seq_schedule: bit 0 sliceable, bit 1 fold_after
        return e

    for queues in (1, 4):
        r = TQ.sched([item()], max_queues=queues, slices=3)
        assert r["nq"] == 1 and r["nsliced"] == 1 and r["nslices"] == [3]
        (rows,) = r["queues"].values()
        per = ((300 + 2) // 3 + 7) & ~7
        # (exec, launch, slice, lo, hi, barrier, acquire): three ranges that tile [0, 300), the first ordered, the others free, then the fold
        assert [x[:5] for x in rows[:3]] == [(0, 0, k, per * k, min(300, per * (k + 1))) for k in range(3)]
        assert [x[5] for x in rows] == [1, 0, 0, 1] and rows[3][:3] == (0, 1, 0) and rows[3][5:] == (1, 1)
        assert all(x[6] == 1 for x in rows)                       # (it accumulates into its destination: every range acquires)
    # never automatically, not below 64 workgroups per range, not without the flag (a split plan's two launches stay whole)
    for kw, e in ((dict(slices=-1), item()), (dict(slices=1), item()), (dict(slices=3), item(grid=191)), (dict(slices=3), item(fold_after=False))):
        r = TQ.sched([e], **kw)
        (rows,) = r["queues"].values()
        assert r["nsliced"] == 0 and [x[1] for x in rows] == [0, 1] and [x[5] for x in rows] == [1, 1], (kw, rows)
    # every packet ordered on request; an unrelated single-launch item is still cut over queues of its own
    (rows,) = TQ.sched([item()], slices=3, all_ordered=True)["queues"].values()
    assert [x[5] for x in rows] == [1, 1, 1, 1]
    other = TQ.ex([TQ.span(5)], [TQ.span(6)], grid=4096)
    r = TQ.sched([item(), other], slices=2)
    assert r["nslices"] == [2, 2] and r["nq"] == 3 and sorted(len(v) for v in r["queues"].values()) == [1, 1, 3]
