"""Contraction groups with per-member constants of f (SMR_GROUP_CONTRACT_SCALARS), host side (no device): what smr_group_create
accepts and refuses under the new flag, that nothing changes without it, describe() / layout() of every row of
tests/group_contract_scalar_cases.py against the unflagged group of the same members, what the table reaches, the
`with S.group(contract=True, contract_scalars=True):` front with the launcher stubbed, and the table's NumPy model against a plain loop."""
import ctypes as C
import sys

import numpy as np
import pytest

import contract_cases as CC
import group_contract_scalar_cases as GS
import strided_jl_amd as S
import window_cases as W
from strided_jl_amd import _lib as L

MR = sys.modules["strided_jl_amd.mapreduce"]
ROWS = GS.table()
FLAG = 64
NAME = "SMR_GROUP_CONTRACT_SCALARS"


def fresh(shape, dtype=np.float64):
    return S.StridedView(np.zeros(shape, dtype=dtype, order="F"))


def mul_ops(m, n, k, dt=np.float64):
    Cv, A, B = fresh((m, n), dt), fresh((m, k), dt), fresh((k, n), dt)
    A2 = S.StridedView(A.parent, (m, 1, k), (A.strides[0], 0, A.strides[1]), A.offset, A.op)
    B2 = S.StridedView(B.parent, (1, n, k), (0, B.strides[1], B.strides[0]), B.offset, B.op)
    C2 = S.StridedView(Cv.parent, (m, n, 1), (Cv.strides[0], Cv.strides[1], 0), Cv.offset, Cv.op)
    return S.promoteshape((m, n, k), C2, A2, B2)


def mul_problem(alpha, m=20, n=24, k=9, dt=np.float64, initop="zero"):
    f = (lambda x, y: x * y) if alpha is None else (lambda x, y: x * y * alpha)
    return S.build_problem(f, "+", initop, (m, n, k), mul_ops(m, n, k, dt), stream=0)


def create(problems, flags=0):
    """(status, message, describe()) of smr_group_create on a list of (problem, keepalive)."""
    lib = L.load()
    arr = (L.smr_problem * max(1, len(problems)))()
    for i, (p, _) in enumerate(problems):
        C.memmove(C.byref(arr[i]), C.byref(p), C.sizeof(L.smr_problem))
    h = C.c_void_p()
    rc = lib.smr_group_create(arr, len(problems), flags, C.byref(h))
    msg = lib.smr_last_error().decode() if rc else ""
    desc = ""
    if rc == 0:
        buf = C.create_string_buffer(1024)
        lib.smr_group_describe(h, buf, 1024)
        desc = buf.value.decode()
        lib.smr_group_destroy(h)
    return rc, msg, desc


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_the_flag_is_64_and_a_contraction_group_takes_it():
    assert L.SMR_GROUP_CONTRACT_SCALARS == FLAG
    ps = [mul_problem(2.0), mul_problem(3.0), mul_problem(-0.25)]
    rc, msg, d = create(ps, FLAG)
    assert rc == L.SMR_OK, msg
    assert d.startswith("family=group kind=contract members=3 ") and " f=mul2scale " in d and " jit=0 " in d and d.endswith(" scalars=member"), d
    rc, msg, d = create(ps, FLAG | L.SMR_GROUP_INDEPENDENT)
    assert rc == L.SMR_OK and d.endswith(" independent=asserted scalars=member"), (msg, d)
    # equal constants: the plan without the flag, tagged
    same = [mul_problem(2.0) for _ in range(3)]
    rc, msg, d = create(same, FLAG)
    rc0, _, d0 = create(same)
    assert rc == rc0 == L.SMR_OK and d == d0 + " scalars=shared" and " f=prog " in d, (d, d0)
    # the plain product has no constants: shared
    rc, msg, d = create([mul_problem(None), mul_problem(None)], FLAG)
    assert rc == L.SMR_OK and " f=mul2 " in d and d.endswith(" scalars=shared"), (msg, d)


def test_refusals_name_the_flag_and_flag_two_keeps_its_text():
    ps = [mul_problem(2.0), mul_problem(3.0)]
    x, y = fresh((20, 24)), fresh((20, 24))
    maps = [S.build_problem(lambda a: a * 2.0, None, None, (20, 24), (y, x), stream=0)]
    out = S.StridedView(np.zeros(1), (50,), (0,), 0)
    red = [S.build_problem(lambda a: a * 2.0, "+", "zero", (50,), (out, fresh((50,))), stream=0)]
    for problems, flags in ((red, FLAG | L.SMR_GROUP_REDUCE), (maps, FLAG), (ps, FLAG | L.SMR_GROUP_MEMBER_SCALARS), (maps, FLAG | L.SMR_GROUP_MEMBER_SCALARS)):
        rc, msg, _ = create(problems, flags)
        assert rc == L.SMR_EUNSUPPORTED and NAME in msg, (flags, msg)
    rc, msg, _ = create(ps, L.SMR_GROUP_MEMBER_SCALARS)
    assert rc == L.SMR_EUNSUPPORTED and "SMR_GROUP_MEMBER_SCALARS with a contraction group" in msg and NAME not in msg, msg
    for flags in (4, 16, 32, FLAG | 4, 128, FLAG | 128):
        rc, msg, _ = create(ps, flags)
        assert rc == L.SMR_EINVAL and "unknown flag" in msg, (flags, msg)


def test_without_the_flag_another_alpha_is_refused_as_before():
    rc, msg, _ = create([mul_problem(2.0), mul_problem(3.0)])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "has another f (program or constants) than member 0" in msg, msg
    rc, msg, d = create([mul_problem(2.0), mul_problem(2.0)])
    assert rc == L.SMR_OK and " f=prog " in d and "scalars=" not in d, (msg, d)


def test_under_the_flag_only_the_values_of_the_constants_may_differ():
    a2 = mul_problem(2.0)
    for other, what in ((mul_problem(None), "another f-program"),                                     # x * y: another program
                        (mul_problem(2.0, initop=("scale", 3.0)), "another kind of initop"),
                        (mul_problem(2.0 + 1j), "another class"),                                       # a complex alpha among real arrays
                        (mul_problem(np.float32(2.0), dt=np.float32), "another class")):
        rc, msg, _ = create([a2, other], FLAG)
        assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and what in msg, (what, msg)
    dist = S.build_problem(lambda x, y: (x - y) * (x - y) * 2.0 + 3.0, "+", "zero", (20, 24, 9), mul_ops(20, 24, 9), stream=0)
    rc, msg, _ = create([a2, dist], FLAG)
    assert rc == L.SMR_EUNSUPPORTED and "another f-program" in msg, msg


# ---- every row -------------------------------------------------------------------------------------------------------------------------
def split_part(d):
    return [tok for tok in d.split() if tok.split("=")[0] in ("split", "kparts", "fold", "fold_grid", "scratch")]


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_row_describes_its_scalars_and_is_laid_out_like_the_unflagged_group(row):
    built = row.build()
    g = row.group(built)
    u = row.group(built, flag=False, member0=True)   # the same members, member 0's constants everywhere, no flag
    d, du = g.describe(), u.describe()
    assert d.endswith(" scalars=shared" if row.shared else " scalars=member"), d
    assert "scalars=" not in du, du
    assert CC.field(d, "f") == row.f_tag and CC.field(du, "f") == "prog", (d, du)
    assert CC.field(d, "jit") == ("0" if row.f_tag == "mul2scale" else "1"), d
    for key in ("members", "grid", "tile", "k", "lds", "op", "bytes"):
        assert CC.field(d, key) == CC.field(du, key), (key, d, du)
    assert split_part(d) == split_part(du), (d, du)
    assert g.layout() == u.layout() and g.split_layout() == u.split_layout()
    assert bool(row.split) <= bool(split_part(d)) if row.split >= 2 else True, d
    assert row.tile == 0 or int(CC.field(d, "tile")) == row.tile, d
    if row.shared:   # the plan without the flag, with no table
        assert d == row.group(built, flag=False).describe() + " scalars=shared"


def test_the_table_reaches_what_it_is_meant_to():
    seen = {"tile": set(), "class": set(), "W": set(), "counts": set(), "kind": set(), "f": set(), "wg": set()}
    mixed_split = 0
    for row in ROWS:
        built = row.build()
        g = row.group(built)
        d = g.describe()
        tile = int(CC.field(d, "tile"))
        if not row.shared:
            seen["tile"].add(tile)
            seen["class"].add(row.tn)
            seen["W"].add(row.W)
            seen["counts"].add(len(row.members))
            seen["kind"].add(row.kind)
            seen["f"].add(CC.field(d, "f"))
        sl = g.split_layout()
        if sl and not row.shared:
            S_ = [s[0] for s in sl]
            mixed_split += int(min(S_) == 1 and max(S_) >= 2)
        if tile == 16 and not row.shared:
            for c, (_, _, wgs, _) in zip(row.members, g.layout()):
                m, n = c.dims[0], c.dims[1]
                if wgs > 1 and (m % 16 or n % 16):
                    seen["wg"].add("ragged")
                if wgs > 1 and m % 16 == 0 and n % 16 == 0:
                    seen["wg"].add("whole")
                if wgs > 1 and c.layouts[0].startswith("whole") and m % 8 == 0:
                    seen["wg"].add("vector")
    assert seen["tile"] == {16, 32} and seen["class"] == {"f32", "f64", "c32", "c64", "i64", "mixed"}, seen
    assert seen["W"] == {2, 4} and {2, 3, 37, 300, 2049} <= seen["counts"], seen
    assert seen["kind"] == {"zero", "none", "scale", "const"} and seen["f"] == {"mul2scale", "prog"}, seen
    assert seen["wg"] == {"ragged", "whole", "vector"}, seen
    assert mixed_split >= 3, mixed_split       # split and unsplit members in one group: the two forced rows and the rule's
    assert sum(r.shared for r in ROWS) == 1
    # every member of a `distinct` row has constants of its own; an `ends` row differs in the first and the last member only
    for row in ROWS:
        if row.pattern == "distinct":
            assert len({repr(cs) for cs in row.consts}) == len(row.members), row
        if row.pattern == "ends":
            assert len({repr(cs) for cs in row.consts[1:-1]}) == 1 and len({repr(cs) for cs in row.consts}) == 3, row


# ---- the front, with the launcher stubbed ----------------------------------------------------------------------------------------------
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


ALPHAS = (2.5, -1.5, 3.25, 0.5, -0.25, 4.75)   # (none integer-valued: that is part of the bucket key, as for maps under member_scalars)


def test_front_six_alphas_are_one_bucket_the_library_accepts(host_front):
    ms = mats(6)
    with Recorder(contract=True, contract_scalars=True) as g:
        for i, (Cm, A, B) in enumerate(ms):
            S.mul_(Cm, A, B, ALPHAS[i], 2 + i)
        assert len(g.pending) == 6 and len({c.bucket for c in g.pending}) == 1
    assert [len(x) for x in g.launches] == [6] and host_front == []
    built = [S.build_problem(c.f, c.op, c.initop, c.dims, c.arrays, stream=0) for c in g.launches[0]]
    grp = L.Group([b[0] for b in built], keepalive=built, contract_scalars=True)
    d = grp.describe()
    assert "kind=contract members=6" in d and " f=mul2scale " in d and d.endswith(" scalars=member"), d
    # without the keyword: a bucket per alpha, as before
    with Recorder(contract=True) as g:
        for i, (Cm, A, B) in enumerate(ms):
            S.mul_(Cm, A, B, ALPHAS[i], 2 + i)
    assert sorted(len(x) for x in g.launches) == [1] * 6
    with Recorder(contract=True, member_scalars=True) as g:
        for i, (Cm, A, B) in enumerate(ms):
            S.mul_(Cm, A, B, ALPHAS[i], 2 + i)
    assert sorted(len(x) for x in g.launches) == [1] * 6


def test_front_alpha_one_beta_zero_and_a_complex_alpha_are_buckets_of_their_own(host_front):
    ms = mats(9)
    with Recorder(contract=True, contract_scalars=True) as g:
        for i in range(4):
            S.mul_(*ms[i], ALPHAS[i], 2)
        S.mul_(*ms[4], 1, 2)            # alpha = 1: x * y, another program
        S.mul_(*ms[5], 1, 3)
        S.mul_(*ms[6], 3.5, 0)          # beta = 0: another kind of initop
        S.mul_(*ms[7], 2.5 + 1j, 2)     # a complex alpha on real arrays: another compute class
        S.mul_(*ms[8], 0, 2)            # alpha = 0: a map
        assert [c.op for c in g.pending].count(None) == 1
    assert sorted(len(x) for x in g.launches) == [1, 1, 1, 2, 4] and host_front == []


def test_front_passes_the_flag_for_contraction_buckets_only(host_front, monkeypatch):
    made = []

    class FakeGroup:
        def __init__(self, problems, independent=False, keepalive=(), member_scalars=False, **kw):
            made.append((len(problems), member_scalars, kw))

        def execute(self, stream=None):
            pass

    monkeypatch.setattr(L, "Group", FakeGroup)
    monkeypatch.setattr(MR, "_GROUP_CACHE", type(MR._GROUP_CACHE)())
    ms = mats(3)
    x = [fresh((12, 10)) for _ in range(2)]
    with S.group(contract=True, contract_scalars=True):
        for i, (Cm, A, B) in enumerate(ms):
            S.mul_(Cm, A, B, ALPHAS[i], 2)
        S.copy_(x[0], x[1])
    assert sorted(made, key=lambda t: t[0]) == [(1, False, {}), (3, False, {"contract_scalars": True})]
    del made[:]
    with S.group(contract=True):
        S.mul_(*ms[0], 2.5, 2)
    assert made == [(1, False, {})]
    # the setting is part of the cached group's key
    keys = list(MR._GROUP_CACHE)
    assert len(keys) == 3 and sorted(str(k[2]) for k in keys if k[4] != 0) == ["False", "contract_scalars"]


def test_contract_scalars_needs_contract():
    with pytest.raises(ValueError):
        S.group(contract_scalars=True)
    with pytest.raises(ValueError):
        S.group(member_scalars=True, contract_scalars=True)
    S.group(contract=True, contract_scalars=True)


# ---- the checker is checked --------------------------------------------------------------------------------------------------------------
def loop_model(row, i, ops):
    """The destination's elements of member i by a plain loop over the box, in Python numbers."""
    c = row.members[i]
    arrs = [a.toarray() for a in ops]
    pick = lambda a, idx: a[tuple(x if a.shape[d] > 1 else 0 for d, x in enumerate(idx))]  # noqa: E731
    acc = {}
    for idx in np.ndindex(*c.dims):
        out = tuple(x if arrs[0].shape[d] > 1 else 0 for d, x in enumerate(idx))
        v = c.npf(pick(arrs[1], idx).item(), pick(arrs[2], idx).item())
        acc[out] = acc.get(out, 0) + v
    init = row.initop(i)
    want = np.empty(arrs[0].shape, dtype=arrs[0].dtype)
    for out, v in acc.items():
        old = arrs[0][out].item()
        first = 0 if init == "zero" else (old if init is None else (old * init[1] if init[0] == "scale" else init[1]))
        want[out] = first + v
    return want


@pytest.mark.parametrize("name", ["f64/mula/n2/t0/distinct", "c32/mula/n3/t32/ends", "i64/dist2/n3/t16/ends"])
def test_the_numpy_model_agrees_with_a_plain_loop(name):
    row = GS.row(name)
    built = row.build()
    want = row.expected(built)
    for i, ops in enumerate(built):
        dest = ops[0]
        idx = W.element_index(dest)
        assert np.array_equal(want[i][idx], loop_model(row, i, ops)), (name, i)
        rest = np.ones(want[i].size, dtype=bool)
        rest[idx.ravel()] = False
        assert np.array_equal(want[i][rest].view(np.uint8), dest.parent[rest].view(np.uint8))   # nothing outside the window
