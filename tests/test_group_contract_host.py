"""Contraction groups, host side (no device): what smr_group_create accepts and refuses when member 0 is a reduction, the workgroup
layout against the members' single plans, the paths the table of tests/group_contract_cases.py reaches, the host mirror of the shape
rule (`_contract_shaped`), the `with S.group(contract=True):` front with the launcher stubbed, and a recorded sequence's footprint.
Map groups are pinned by describe() / layout() strings recorded from the commit before contraction groups existed."""
import ctypes as C
import sys

import numpy as np
import pytest

import contract_cases as CC
import group_contract_cases as GC
import strided_jl_amd as S
from strided_jl_amd import _lib as L

MR = sys.modules["strided_jl_amd.mapreduce"]
ROWS = GC.table()
MUL = lambda a, b: a * b  # noqa: E731


def fresh(shape, dtype=np.float64):
    return S.StridedView(np.zeros(shape, dtype=dtype, order="F"))


def mul_ops(m, n, k, dt=np.float64, Cv=None, A=None, B=None):
    """(C2, A2, B2): the box operands of linalg._matmul_ for C (m, n), A (m, k), B (k, n)."""
    Cv = fresh((m, n), dt) if Cv is None else Cv
    A = fresh((m, k), dt) if A is None else A
    B = fresh((k, n), dt) if B is None else B
    A2 = S.StridedView(A.parent, (m, 1, k), (A.strides[0], 0, A.strides[1]), A.offset, A.op)
    B2 = S.StridedView(B.parent, (1, n, k), (0, B.strides[1], B.strides[0]), B.offset, B.op)
    C2 = S.StridedView(Cv.parent, (m, n, 1), (Cv.strides[0], Cv.strides[1], 0), Cv.offset, Cv.op)
    return S.promoteshape((m, n, k), C2, A2, B2)


def mul_problem(m=20, n=24, k=9, dt=np.float64, f=MUL, op="+", initop="zero", **kw):
    return S.build_problem(f, op, initop, (m, n, k), mul_ops(m, n, k, dt, **kw), stream=0)


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


def member_geometry(case, d, tile):
    """(workgroups, ragged?, vec) of a member on `tile` x `tile` tiles, from its single plan's describe() under contract = 2."""
    di, _, dj, _, _ = CC.tile_of(d)
    cdims = [int(x) for x in CC.field(d, "dims").split("x")]
    nk = len(cdims) - len([r for r in case.rdims if case.dims[r] > 1])
    rest = int(np.prod([cdims[x] for x in range(nk) if x not in (di, dj)]))
    wgs = -(-cdims[di] // tile) * -(-cdims[dj] // tile) * rest
    return wgs, bool(cdims[di] % tile or cdims[dj] % tile), int(CC.field(d, "vec"))


# ---- acceptance and layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_row_is_accepted_and_tiles_the_grid_like_the_single_plans(row):
    built = row.build()
    g = row.group(built)
    d = g.describe()
    lay = g.layout()
    tile = int(CC.field(d, "tile"))
    assert d.startswith("family=group kind=contract members=%d " % len(row.members)), d
    assert tile in (16, 32) and (row.tile == 0 or tile == row.tile), d
    key = "i64" if row.tn == "bool" else row.tn
    assert int(CC.field(d, "k")) == CC.tile_numbers(key, tile)[2], d
    assert CC.field(d, "op") == row.op and CC.field(d, "f") == ("prog" if row.needs_prog else "mul2"), d
    assert CC.field(d, "jit") == ("1" if row.needs_prog else "0") and int(CC.field(d, "lds")) <= 65536, d
    assert "linear=" not in d and "independent=" not in d
    singles = row.single_descs(built)
    nxt = 0
    for (form, first, wgs, rank), case, sd in zip(lay, row.members, singles):
        assert CC.family(sd) == "contract", sd
        assert form == 2 and first == nxt and wgs >= 1 and 3 <= rank <= 8
        want = member_geometry(case, sd, tile)[0]
        assert wgs == want, (case.name, sd, d)
        if CC.tile_of(sd)[1] == tile:  # the single call picked the same tile: its grid, as printed
            assert wgs == int(CC.field(sd, "grid")), (case.name, sd)
        nxt += wgs
    assert len(lay) == len(row.members) and nxt == int(CC.field(d, "grid")), d
    assert g.algorithmic_bytes == int(CC.field(d, "bytes")) == sum(int(CC.field(s, "algbytes")) for s in singles)
    if len(row.members) >= 3:   # the first and the last member have a single workgroup, one in the middle has many
        assert lay[0][2] == 1 and lay[-1][2] == 1 and max(x[2] for x in lay[1:-1]) >= 12


def test_the_table_reaches_both_tiles_and_every_copy_of_the_body():
    """Per tile and type: ragged members (the clamped copy), whole members without vector loads (the bounds-free copy) and -- where
    the type has a vector at all -- whole members with them, read from the members' single-plan describe() (vec=)."""
    seen = {}
    for row in ROWS:
        built = row.build()
        g = row.group(built)
        tile = int(CC.field(g.describe(), "tile"))
        for case, sd in zip(row.members, row.single_descs(built)):
            _, ragged, vec = member_geometry(case, sd, tile)
            seen.setdefault((tile, row.tn), set()).add("ragged" if ragged else ("vector" if vec > 1 else "whole"))
    for tn in GC.TYPES:
        for tile in (16, 32):
            want = {"ragged", "whole"} | ({"vector"} if tn in ("f32", "f64", "c32", "i64") else set())
            assert seen.get((tile, tn), set()) >= want, (tile, tn, seen.get((tile, tn)))
    assert {t for t, _ in seen} == {16, 32}
    # the rule itself reaches both tiles
    rule = {int(CC.field(r.group(r.build()).describe(), "tile")) for r in ROWS if r.tile == 0}
    assert rule == {16, 32}, rule


def test_counts_of_the_table():
    assert {len(r.members) for r in ROWS} >= {1, 2, 3, 37, 300}
    assert {r.kind for r in ROWS} == {"zero", "none", "const", "scale"}
    assert {(r.fname, r.op) for r in ROWS} == {("mul", "+"), ("dist", "+"), ("asym", "+"), ("plus", "min"), ("and", "|")}


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_member():
    ok = mul_problem
    a = fresh((6, 5))
    amap = S.build_problem(lambda x: x, None, None, a.size, (a.similar(), a), stream=0)
    rc, msg = create([ok(), ok(), amap])
    assert rc == L.SMR_EUNSUPPORTED and "member 2" in msg and "map" in msg, msg
    x, o = fresh((8, 8)), fresh((1, 1))
    plain = S.build_problem(lambda v: v, "+", None, x.size, S.promoteshape(x.size, o, x), stream=0)
    rc, msg = create([plain])
    assert rc == L.SMR_EUNSUPPORTED and "member 0" in msg and "contraction" in msg, msg
    rc, msg = create([ok(), plain])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "contraction" in msg, msg
    rc, msg = create([ok(), ok(m=1)])       # the size-1 dim is dropped: one input left varying along a kept dim
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "contraction" in msg, msg
    rc, msg = create([ok(), ok(), ok(op="max")])
    assert rc == L.SMR_EUNSUPPORTED and "member 2" in msg and "op" in msg, msg
    rc, msg = create([ok(initop=("scale", 2)), ok(initop="zero")])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "initop" in msg, msg
    rc, msg = create([ok(f=lambda p, q: p * q * 2), ok(f=lambda p, q: p * q * 3)])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg, msg
    rc, msg = create([ok(), ok(dt=np.float32)])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg, msg
    # an input on the destination's buffer: C[:, 0:4] = C[:, 4:8] * B
    P = fresh((8, 8))
    rc, msg = create([ok(), ok(m=8, n=4, k=4, Cv=P.sview(slice(None), slice(0, 4)), A=P.sview(slice(None), slice(4, 8)))])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "contraction" in msg, msg
    rc, msg = create([ok(), ok()], L.SMR_GROUP_MEMBER_SCALARS)
    assert rc == L.SMR_EUNSUPPORTED and "SMR_GROUP_MEMBER_SCALARS" in msg, msg
    assert create([ok(), ok()], 4)[0] == L.SMR_EINVAL
    # a reduction after a map: as before
    rc, msg = create([amap, ok()])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "reduction" in msg, msg


def test_beta_may_differ_and_interleaved_blocks_need_the_flag():
    assert create([mul_problem(initop=("scale", b)) for b in (2, 3, -0.5, 7)])[0] == L.SMR_OK
    assert create([mul_problem(initop=("const", b)) for b in (2, 3)])[0] == L.SMR_OK
    P = fresh((16, 16))   # even and odd columns of one parent: the byte ranges overlap, the elements do not
    ms = [mul_problem(m=16, n=8, k=5, Cv=P.sview(slice(None), slice(j, None, 2))) for j in (0, 1)]
    rc, msg = create(ms)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "SMR_GROUP_INDEPENDENT" in msg
    assert create(ms, L.SMR_GROUP_INDEPENDENT)[0] == L.SMR_OK
    built = [mul_problem(m=16, n=8, k=5, Cv=P.sview(slice(None), slice(j, None, 2))) for j in (0, 1)]
    g = L.Group([b[0] for b in built], True, keepalive=built)
    assert g.describe().endswith(" independent=asserted")


def test_the_tile_rule_and_the_forced_tile():
    def tile(ms, forced=0, lds=None):
        with CC.option("group_contract_tile", forced):
            if lds is None:
                g = L.Group([m[0] for m in ms], keepalive=ms)
            else:
                with CC.option("max_lds_bytes", lds):
                    g = L.Group([m[0] for m in ms], keepalive=ms)
        return int(CC.field(g.describe(), "tile")), int(CC.field(g.describe(), "grid"))

    few = [mul_problem(32, 32, 32) for _ in range(255)]
    assert tile(few) == (16, 4 * 255)                       # 255 tiles of 32 x 32: under a workgroup per CU
    assert tile(few + [mul_problem(32, 32, 32)]) == (32, 256)
    assert tile([mul_problem(17, 17, 8) for _ in range(300)]) == (16, 4 * 300)   # 289 of 1024 outputs per tile: under half full
    assert tile([mul_problem(24, 24, 8) for _ in range(300)]) == (32, 300)       # 576 of 1024
    assert tile(few, 32) == (32, 255) and tile(few + [mul_problem(32, 32, 32)], 16) == (16, 4 * 256)
    # Float64, 32 x 32: 34816 bytes of LDS; 16 x 16: 18432
    assert tile(few, 32, lds=20000)[0] == 16
    with CC.option("max_lds_bytes", 1000):
        rc, msg = create(few[:2])
    assert rc == L.SMR_EUNSUPPORTED and "max_lds_bytes" in msg
    with pytest.raises(L.StridedHIPError):
        S.set_option("group_contract_tile", 64)
    assert S.get_option("group_contract_tile") == 0


# ---- map groups are what they were --------------------------------------------------------------------------------------------------
def _map_groups():
    ident = lambda x: x  # noqa: E731
    shapes = [(1,), (5, 7), (31, 33), (33, 31), (64, 1, 3), (4,) * 8, (1024,), (1025,), (40, 40, 3)]
    one = []
    for i, shp in enumerate(shapes):
        a = fresh(shp)
        perm = tuple(reversed(range(len(shp)))) if i % 2 else tuple(range(len(shp)))
        one.append(S.build_problem(ident, None, None, tuple(shp[j] for j in perm), (fresh(tuple(shp[j] for j in perm)), a.permutedims(perm)), stream=0))
    two = []
    for shp in ((17, 5), (40, 33), (3, 3, 3)):
        x, y = fresh(shp, np.float32), fresh(tuple(reversed(shp)), np.float32)
        two.append(S.build_problem(lambda p, q: p * q - p / 3, None, None, shp, (fresh(shp, np.float32), x, y.permutedims(tuple(reversed(range(len(shp)))))), stream=0))
    three = []
    for i, shp in enumerate(((6, 5), (33, 40), (12,))):
        x, y = fresh(shp), fresh(shp)
        three.append(S.build_problem((lambda a_, b_: (lambda p, q: a_ * p + b_ * q))(2 + i, 5 - i), None, None, shp, (y, x, y), stream=0))
    return [(one, False, False), (two, True, False), (three, False, True)]


MAP_GROUPS_BEFORE = [  # describe() and layout() of _map_groups() at the commit before contraction groups
    ('family=group members=9 grid=78 linear=8 transposing=1 f=ident jit=0 bytes=1194544',
     [(0, 0, 1, 1), (0, 1, 1, 2), (0, 2, 1, 1), (1, 3, 2, 2), (0, 5, 1, 1), (0, 6, 64, 8), (0, 70, 1, 1), (0, 71, 2, 1), (0, 73, 5, 1)]),
    ('family=group members=3 grid=6 linear=2 transposing=1 f=prog jit=1 bytes=17184 independent=asserted',
     [(0, 0, 1, 2), (1, 1, 4, 2), (0, 5, 1, 3)]),
    ('family=group members=3 grid=4 linear=3 transposing=0 f=axpby jit=0 bytes=21792 scalars=member',
     [(0, 0, 1, 1), (0, 1, 2, 1), (0, 3, 1, 1)]),
]


def test_map_groups_describe_and_layout_are_unchanged():
    got = []
    for ms, independent, scalars in _map_groups():
        g = L.Group([m[0] for m in ms], independent, keepalive=ms, member_scalars=scalars)
        got.append((g.describe(), g.layout()))
    assert got == MAP_GROUPS_BEFORE


# ---- the host mirror of the shape rule ----------------------------------------------------------------------------------------------
def library_accepts(f, dims, arrays):
    p = S.build_problem(f, "+", "zero", dims, arrays, stream=0)
    return create([p])[0] == L.SMR_OK


def test_contract_shaped_agrees_with_the_library_on_the_table():
    n = 0
    for row in ROWS:
        if len(row.members) > 40:
            continue
        for case, ops in zip(row.members, row.build()):
            arrays = S.promoteshape(case.dims, *ops)
            assert MR._contract_shaped(case.dims, arrays) is True, case.name
            n += 1
    assert n > 500
    for case in CC.table():   # and on what contract_cases.py lists as refused, the m == 1 and k == 1 rows included
        if case.op is None or len(case.axes) != 3:
            continue
        arrays = S.promoteshape(case.dims, *case.build())
        with CC.option("group_max_bytes", 1 << 40):   # (the shape alone: some rows are larger than the front defers)
                assert MR._contract_shaped(case.dims, arrays) == (case.family == CC.CONTRACT) == library_accepts(case.f, case.dims, arrays), case.name


def random_reduction(rng):
    """A three-operand reduction with random broadcast patterns, dim orders, steps and (sometimes) an input inside the destination's
    parent."""
    N = int(rng.integers(2, 5))
    dims = tuple(int(rng.choice([1, 2, 3, 5, 6])) for _ in range(N))
    patterns = [[bool(rng.integers(0, 3)) for _ in range(N)] for _ in range(3)]
    if rng.integers(0, 4):   # mostly a matrix-product-like pattern with the roles shuffled
        N = max(N, 3)
        dims = tuple(int(rng.choice([1, 2, 3, 5, 6, 7])) for _ in range(N))
        roles = list(rng.permutation(["i", "j", "k", "b"][:N]))
        table = {"i": (1, 1, 0), "j": (1, 0, 1), "k": (0, 1, 1), "b": (1, 1, 1)}
        patterns = [[bool(table[r][o]) for r in roles] for o in range(3)]
        if rng.integers(0, 4) == 0:
            patterns[int(rng.integers(0, 3))][int(rng.integers(0, N))] ^= True
    share = rng.integers(0, 6) == 0
    pool = np.zeros(4096)
    arrays = []
    for o in range(3):
        parent = pool if (o == 0 or (o == 1 and share)) else np.zeros(1024)
        order = rng.permutation(N)
        strides, s = [0] * N, int(rng.integers(1, 3))
        for d in order:
            if patterns[o][d]:
                strides[d] = s * (-1 if rng.integers(0, 5) == 0 else 1)
                s *= dims[d] + int(rng.integers(0, 2))
        off = 512 if o == 0 else 1536
        arrays.append(S.StridedView(parent, dims, tuple(strides), off))
    return dims, tuple(arrays)


def test_contract_shaped_agrees_with_the_library_on_random_reductions():
    rng = np.random.default_rng(20261020)
    yes = 0
    for i in range(200):
        dims, arrays = random_reduction(rng)
        want = library_accepts(MUL, dims, arrays)
        assert MR._contract_shaped(dims, arrays) == want, (i, dims, [a.strides for a in arrays])
        yes += want
    assert 30 <= yes <= 170, yes   # both answers occur
    # the byte limit is the front's alone
    dims, arrays = (20, 24, 9), mul_ops(20, 24, 9)
    assert MR._contract_shaped(dims, arrays)
    with CC.option("group_max_bytes", 100):
        assert not MR._contract_shaped(dims, arrays) and library_accepts(MUL, dims, arrays)


# ---- the front, with the launcher stubbed -------------------------------------------------------------------------------------------
class Recorder(S.group):
    """`S.group` with the launcher stubbed out: records the deferred calls of every launch."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.launches = []

    def _launch(self, calls, stream):
        self.launches.append(list(calls))


@pytest.fixture
def host_front(monkeypatch):
    """Host views pass for device views and smr_mapreduce is a stub that records the problems it is handed (redop, initop, beta)."""
    singles = []

    def fake(pp):
        p = C.cast(pp, C.POINTER(L.smr_problem)).contents
        singles.append((p.redop, p.initop, p.initarg[0]))
        return 0

    monkeypatch.setattr(S.StridedView, "on_device", property(lambda self: True))
    monkeypatch.setattr(MR, "_SMR_MAPREDUCE", fake)
    monkeypatch.setattr(MR, "_PROBLEM_CACHE", type(MR._PROBLEM_CACHE)())
    return singles


def mats(K, m=12, n=10, k=7):
    return [(fresh((m, n)), fresh((m, k)), fresh((k, n))) for _ in range(K)]


def test_front_default_group_flushes_at_a_mul_and_defers_none(host_front):
    ms = mats(3)
    x = fresh((12, 7))
    with Recorder() as g:
        S.copy_(ms[0][1], x)
        for Cm, A, B in ms:
            S.mul_(Cm, A, B, 1, 2)
            assert g.pending == []
    assert [len(x) for x in g.launches] == [1] and g.launches[0][0].op is None
    assert host_front == [(L.SMR_RED_ADD, L.SMR_INIT_SCALE, 2.0)] * 3


def test_front_contract_buckets_by_alpha_and_kind_not_by_beta(host_front):
    ms = mats(6)
    with Recorder(contract=True) as g:
        for i, (Cm, A, B) in enumerate(ms):
            S.mul_(Cm, A, B, 1, 2 + i)
        assert len(g.pending) == 6 and len({c.bucket for c in g.pending}) == 1
    assert [len(x) for x in g.launches] == [6] and host_front == []
    assert [c.initop for c in g.launches[0]] == [("scale", 2 + i) for i in range(6)] and {c.op for c in g.launches[0]} == {"+"}
    with Recorder(contract=True, member_scalars=True) as g:   # another alpha is another f: a bucket of its own, also under member_scalars
        for i, (Cm, A, B) in enumerate(ms):
            S.mul_(Cm, A, B, 1 if i < 3 else 3, 2)
        S.mul_(ms[0][0].similar(), ms[0][1], ms[0][2], 3, 0)   # beta = 0: another kind of initop
        S.mul_(ms[1][0].similar(), ms[1][1], ms[1][2], 4, 2)
    assert sorted(len(x) for x in g.launches) == [1, 1, 3, 3]
    # scalar forms and alpha == 0 take the map path
    with Recorder(contract=True) as g:
        S.mul_(ms[0][0], ms[0][1], ms[0][2], 0, 2)
        S.mul_(ms[1][1], ms[2][1], 3)
        assert [c.op for c in g.pending] == [None, None]


def test_front_contract_flushes_before_a_mul_that_reads_a_pending_destination(host_front):
    (C0, A0, B0), (C1, A1, B1) = mats(2)
    x = fresh((7, 12))
    with Recorder(contract=True) as g:
        S.permutedims_(A0, x, (1, 0))
        S.mul_(C1, A1, B1, 1, 2)        # unrelated: stays pending next to the map
        assert g.launches == [] and len(g.pending) == 2
        S.mul_(C0, A0, B0, 1, 2)        # reads what the pending permutedims_ writes
        assert [len(l) for l in g.launches] == [1, 1] and len(g.pending) == 1
        S.copy_(fresh((12, 10)), C0)    # reads a pending contraction's destination
        assert [len(l) for l in g.launches] == [1, 1, 1]
        S.mul_(C0, A1, B1, 1, 2)
        S.mul_(C0, A0, B0, 1, 2)        # writes (and reads) a pending destination
        assert [len(l) for l in g.launches] == [1, 1, 1, 1, 1]
    assert host_front == []


def test_front_a_refused_bucket_runs_call_by_call_with_op_and_initop(host_front, monkeypatch):
    def refuse(*a, **kw):
        raise L.UnsupportedOnDevice(L.SMR_EUNSUPPORTED, "refused")

    monkeypatch.setattr(L, "Group", refuse)
    ms = mats(3)
    with S.group(contract=True) as g:
        for i, (Cm, A, B) in enumerate(ms):
            S.mul_(Cm, A, B, 1, 2 + i)
    assert g.singles == 3 and g.groups == []
    assert host_front == [(L.SMR_RED_ADD, L.SMR_INIT_SCALE, 2.0 + i) for i in range(3)]


def test_front_buckets_are_groups_the_library_accepts(host_front):
    ms = mats(5)
    with Recorder(contract=True) as g:
        for i, (Cm, A, B) in enumerate(ms):
            S.mul_(Cm, A, B, 2, 2 + i)
    (launch,) = g.launches
    built = [S.build_problem(c.f, c.op, c.initop, c.dims, c.arrays, stream=0) for c in launch]
    grp = L.Group([b[0] for b in built], keepalive=built)
    assert "kind=contract members=5" in grp.describe() and "f=prog" in grp.describe()


# ---- a recorded sequence --------------------------------------------------------------------------------------------------------------
def test_a_sequence_of_one_contraction_group_is_one_component_with_the_members_footprint():
    built = [mul_problem(16, 16, 8) for _ in range(3)]
    g = L.Group([b[0] for b in built], keepalive=built)
    q = S.Sequence().add_group(g)
    assert q.components() == [0]
    acq, fp, resident = q.fences()
    assert acq == [0] and resident and fp == 3 * (16 * 16 + 16 * 8 + 8 * 16) * 8
    arr = (C.c_int32 * 1)()
    assert L.load().smr_seq_components(q._h, arr, 1) == 1
    # a plan that reads a member's destination joins it
    Cm = fresh((16, 16))
    b2 = [mul_problem(16, 16, 8, Cv=Cm)]
    g2 = L.Group([b2[0][0]], keepalive=b2)
    reader = S.make_plan(lambda v: v, None, None, Cm.size, (Cm.similar(), Cm))
    assert S.Sequence().add_group(g2).add(reader).components() == [0, 0]
