"""Grouped launches, host side (no device): what smr_group_create accepts and refuses, the workgroup layout of a planned
group, the body chosen per member, and the conflict-flush rule of `with S.group():` (checked with a stubbed launcher)."""
import ctypes as C

import numpy as np
import pytest

import strided_jl_amd as S
from strided_jl_amd import _lib as L


def ident(x):
    return x


def fresh(shape, dtype=np.float64):
    return S.StridedView(np.zeros(shape, dtype=dtype, order="F"))


def problem(f, dst, *ins, op=None):
    p, keep = S.build_problem(f, op, None, dst.size, (dst,) + ins, stream=0)
    return p, keep


def create(problems, flags=0):
    """(status, message, handle) of smr_group_create on a list of (problem, keepalive)."""
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


def copy_member(shape=(6, 5), dtype=np.float64):
    a = fresh(shape, dtype)
    return problem(ident, a.similar(), a)


def test_refuses_a_reduction_member():
    a = fresh((8, 8))
    o = fresh((1, 1))
    red = S.build_problem(ident, "+", None, a.size, S.promoteshape(a.size, o, a), stream=0)
    rc, msg = create([copy_member(), red])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "reduction" in msg


def test_refuses_a_dtype_mismatch():
    rc, msg = create([copy_member(), copy_member(), copy_member(dtype=np.float32)])
    assert rc == L.SMR_EUNSUPPORTED and "member 2" in msg


def test_refuses_an_f_mismatch():
    a, b = fresh((4, 4)), fresh((4, 4))
    m0 = problem(lambda x: x * 2, a.similar(), a)
    m1 = problem(lambda x: x * 3, b.similar(), b)  # same program, another constant
    m2 = problem(lambda x: x + 2, b.similar(), b)
    rc, msg = create([m0, m1])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "f" in msg
    rc, msg = create([m0, m2])
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg
    assert create([m0, problem(lambda x: x * 2, b.similar(), b)])[0] == L.SMR_OK


def test_count_zero_and_null_are_malformed():
    lib = L.load()
    h = C.c_void_p()
    arr = (L.smr_problem * 1)()
    assert lib.smr_group_create(arr, 0, 0, C.byref(h)) == L.SMR_EINVAL
    assert "count" in lib.smr_last_error().decode()
    assert lib.smr_group_create(None, 1, 0, C.byref(h)) == L.SMR_EINVAL
    assert lib.smr_group_create(arr, 70000, 0, C.byref(h)) == L.SMR_EINVAL
    bad = copy_member()
    bad[0].dims[0] = 0  # a malformed member keeps its status and is named
    rc, msg = create([copy_member(), bad])
    assert rc == L.SMR_EINVAL and "member 1" in msg


def interleaved_members():
    """Even and odd columns of one parent copied into even and odd columns of another: the byte ranges overlap, the elements do not."""
    src, dst = fresh((8, 8)), fresh((8, 8))
    return [problem(ident, dst.sview(slice(None), slice(k, None, 2)), src.sview(slice(None), slice(k, None, 2))) for k in (0, 1)]


def test_range_conflict_is_refused_without_the_flag_and_accepted_with_it():
    ms = interleaved_members()
    rc, msg = create(ms)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "SMR_GROUP_INDEPENDENT" in msg
    assert create(ms, L.SMR_GROUP_INDEPENDENT)[0] == L.SMR_OK
    # a member that reads what another one writes
    a, b, c = fresh((4, 4)), fresh((4, 4)), fresh((4, 4))
    chain = [problem(ident, b, a), problem(ident, c, b)]
    rc, msg = create(chain)
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg
    # shared inputs and an in-place member are fine
    d = fresh((4, 4))
    assert create([problem(ident, b, a), problem(ident, c, a), problem(ident, d, d)])[0] == L.SMR_OK


def test_layout_tiles_the_grid_in_member_order():
    shapes = [(1,), (5, 7), (31, 33), (33, 31), (64, 1, 3), (4,) * 8, (1024,), (1025,), (40, 40, 3)]
    members, forms = [], []
    for i, shp in enumerate(shapes):
        a = fresh(shp)
        perm = tuple(reversed(range(len(shp)))) if i % 2 else tuple(range(len(shp)))
        members.append(problem(ident, fresh(tuple(shp[j] for j in perm)), a.permutedims(perm)))
    g = L.Group([m[0] for m in members], keepalive=members)
    lay = g.layout()
    assert len(lay) == len(shapes)
    nxt = 0
    for form, first, wgs, rank in lay:
        assert first == nxt and wgs >= 1 and form in (0, 1) and 1 <= rank <= 8
        nxt = first + wgs
    d = g.describe()
    assert "family=group" in d and "members=%d" % len(shapes) in d and "grid=%d " % nxt in d and "jit=0" in d and "f=ident" in d
    assert "linear=%d" % sum(1 for r in lay if r[0] == 0) in d and "transposing=%d" % sum(1 for r in lay if r[0] == 1) in d
    # 1024 contiguous elements are one chunk of 256 lanes x 4, one more element takes a second workgroup
    assert lay[6][2] == 1 and lay[7][2] == 2
    assert g.algorithmic_bytes == sum(2 * 8 * int(np.prod(s)) for s in shapes)


def test_body_chosen_per_member():
    a = fresh((33, 31))
    same = problem(ident, a.similar(), a)
    tr = problem(ident, fresh((31, 33)), a.permutedims((1, 0)))
    x = fresh((20, 24, 28))
    two = problem(lambda p, q: p + q, fresh((24, 28, 20)), x.permutedims((1, 2, 0)), fresh((28, 20, 24)).permutedims((2, 0, 1)))
    assert L.Group([same[0]], keepalive=same).layout()[0][0] == 0
    form, first, wgs, rank = L.Group([tr[0]], keepalive=tr).layout()[0]
    assert (form, first, wgs, rank) == (1, 0, 2 * 1, 2)  # 31 -> one tile along dim 0, 33 -> two along the input's unit dim
    assert L.Group([two[0]], keepalive=two).layout()[0][0] == 0


def test_group_max_bytes_option():
    old = S.get_option("group_max_bytes")
    assert old > 0
    S.set_option("group_max_bytes", 12345)
    try:
        assert S.get_option("group_max_bytes") == 12345
    finally:
        S.set_option("group_max_bytes", old)


class Recorder(S.group):
    """`S.group` with the launcher stubbed out: records which calls every launch would hold."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.launches = []

    def _launch(self, calls, stream):
        self.launches.append([c.arrays[0] for c in calls])


def test_front_flushes_pending_calls_before_a_conflicting_one():
    a, b, c = fresh((4, 4)), fresh((4, 4)), fresh((4, 4))
    da, db, dc = a.similar(), b.similar(), c.similar()
    g = Recorder()
    assert g.defer(ident, a.size, (da, a))          # A
    assert g.defer(ident, a.size, (db, b))          # B
    assert g.launches == []
    assert g.defer(ident, a.size, (dc, da))         # C reads A's destination
    assert g.launches == [[da, db]]
    g.flush()
    assert g.launches == [[da, db], [dc]]
    g.flush()
    assert len(g.launches) == 2
    # writing what a pending call reads, or writes, flushes too
    g = Recorder()
    g.defer(ident, a.size, (da, a))
    g.defer(ident, a.size, (a, b))
    assert g.launches == [[da]]
    g.defer(ident, a.size, (a, c))
    assert g.launches == [[da], [a]]


def test_front_buckets_by_f_and_respects_independent():
    a, b = fresh((4, 4)), fresh((4, 4))
    da, db = a.similar(), b.similar()
    g = Recorder()
    g.defer(lambda x: x * 2, a.size, (da, a))
    g.defer(lambda x: x * 3, a.size, (db, b))
    g.flush()
    assert g.launches == [[da], [db]]
    # interleaved blocks: the ranges conflict, the views differ
    src, dst = fresh((8, 8)), fresh((8, 8))
    ev = [(dst.sview(slice(None), slice(k, None, 2)), src.sview(slice(None), slice(k, None, 2))) for k in (0, 1)]
    g = Recorder()
    for d, s in ev:
        g.defer(ident, d.size, (d, s))
    assert len(g.launches) == 1  # flushed before the second call
    g = Recorder(independent=True)
    for d, s in ev:
        g.defer(ident, d.size, (d, s))
    assert g.launches == []
    g.defer(ident, ev[0][0].size, (src.sview(slice(None), slice(0, None, 2)).similar(), ev[0][0]))  # reads exactly a pending destination
    assert len(g.launches) == 1 and len(g.launches[0]) == 2


def test_front_leaves_large_members_to_the_normal_path():
    a = fresh((64, 64))
    g = Recorder()
    old = S.get_option("group_max_bytes")
    S.set_option("group_max_bytes", 2 * 64 * 64 * 8 - 1)
    try:
        assert not g.defer(ident, a.size, (a.similar(), a))
        S.set_option("group_max_bytes", 2 * 64 * 64 * 8)
        assert g.defer(ident, a.size, (a.similar(), a))
    finally:
        S.set_option("group_max_bytes", old)
