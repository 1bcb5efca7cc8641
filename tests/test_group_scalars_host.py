"""Grouped launches with per-member scalars (SMR_GROUP_MEMBER_SCALARS), host side (no device): what smr_group_create accepts and
refuses under the flag, what describe() / layout() report, the buckets of `with S.group(member_scalars=True):` (stubbed launcher)
and the sequence analyses of a flagged group.  Member i's scalars are a function of i throughout."""
import numpy as np

import strided_jl_amd as S
from strided_jl_amd import _lib as L
from test_group_host import Recorder, create, fresh, ident, problem

FLAG = L.SMR_GROUP_MEMBER_SCALARS


def scale(k):
    return lambda x: x * k


def axpby(a, b):
    return lambda x, y: a * x + b * y


def member(f, shape=(4, 4), dtype=np.float64, nin=1):
    ins = [fresh(shape, dtype) for _ in range(nin)]
    return problem(f, fresh(shape, dtype), *ins)


def group(members, **kw):
    return L.Group([m[0] for m in members], keepalive=members, **kw)


def test_the_flag_is_known_and_admits_differing_constants():
    assert FLAG == 2
    ms = [member(scale(2)), member(scale(3))]
    assert create(ms, FLAG)[0] == L.SMR_OK
    assert create(ms, FLAG | L.SMR_GROUP_INDEPENDENT)[0] == L.SMR_OK
    rc, msg = create(ms)  # without the flag: refused as before, with the message of before
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "has another f (program or constants) than member 0" in msg
    rc, msg = create(ms, 4)
    assert rc == L.SMR_EINVAL and "unknown flag" in msg


def test_what_is_still_refused_under_the_flag():
    m0 = member(scale(2))
    rc, msg = create([m0, member(lambda x: x + 2)], FLAG)                       # another program
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg
    rc, msg = create([m0, member(scale(2 + 1j))], FLAG)                         # a complex scalar among real ones
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "computes in another class than member 0" in msg
    rc, msg = create([member(scale(3), dtype=np.int32), member(scale(2.5), dtype=np.int32)], FLAG)  # leaves the integer class
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg and "computes in another class than member 0" in msg
    two = lambda a, b: (lambda x, y: a * x + b * y)  # noqa: E731
    rc, msg = create([member(two(2, 3), nin=2), member(two(2, 2), nin=2)], FLAG)  # equal constants are merged: another program
    assert rc == L.SMR_EUNSUPPORTED and "member 1" in msg
    # the second member is named, not the first offender's neighbour
    rc, msg = create([m0, member(scale(5)), member(lambda x: x + 2)], FLAG)
    assert rc == L.SMR_EUNSUPPORTED and "member 2" in msg


def test_describe_says_where_the_scalars_live():
    differing = [member(scale(1 + i / 8)) for i in range(3)]
    equal = [member(scale(2.5)) for _ in range(3)]
    assert group(differing, member_scalars=True).describe().endswith(" scalars=member")
    assert group(equal, member_scalars=True).describe().endswith(" scalars=shared")
    plain = group(equal).describe()
    assert "scalars=" not in plain
    assert group(equal, member_scalars=True).describe() == plain + " scalars=shared"
    # -0.0 and 0.0 are different constants
    neg = member(scale(0.0))
    neg[0].fconsts[0] = -0.0  # (written into the problem: the front's caches compare captured values with ==)
    assert group([member(scale(0.0)), neg], member_scalars=True).describe().endswith(" scalars=member")
    d = group([member(ident), member(ident)], member_scalars=True).describe()       # an f without constants
    assert d.endswith(" scalars=shared") and "f=ident" in d
    assert group(differing, member_scalars=True, independent=True).describe().endswith(" independent=asserted scalars=member")


def test_layout_and_bytes_do_not_depend_on_the_flag():
    shapes = [(1,), (5, 7), (31, 33), (33, 31), (64, 1, 3), (4,) * 8, (1024,), (1025,), (40, 40, 3)]

    def members(own):
        out = []
        for i, shp in enumerate(shapes):
            a = fresh(shp)
            perm = tuple(reversed(range(len(shp)))) if i % 2 else tuple(range(len(shp)))
            out.append(problem(scale(1 + i / 8 if own else 2.5), fresh(tuple(shp[j] for j in perm)), a.permutedims(perm)))
        return out

    plain, flagged, shared = group(members(False)), group(members(True), member_scalars=True), group(members(False), member_scalars=True)
    assert flagged.describe().endswith("scalars=member") and shared.describe().endswith("scalars=shared")
    assert plain.layout() == flagged.layout() == shared.layout()
    assert {r[0] for r in plain.layout()} == {0, 1}
    assert plain.algorithmic_bytes == flagged.algorithmic_bytes == shared.algorithmic_bytes == sum(2 * 8 * int(np.prod(s)) for s in shapes)
    assert flagged.describe()[:-len(" scalars=member")] == plain.describe()


def test_recognised_functors_keep_their_names():
    k = lambda i: 1 + i / 8  # noqa: E731
    h = lambda i: 2 - i / 16  # noqa: E731
    g = group([member(axpby(k(i), h(i)), nin=2) for i in range(3)], member_scalars=True)
    assert "f=axpby" in g.describe() and "jit=0" in g.describe() and g.describe().endswith("scalars=member")
    g = group([member(scale(k(i))) for i in range(3)], member_scalars=True)
    assert "f=scale" in g.describe() and "jit=0" in g.describe()
    g = group([member((lambda c: lambda x, y: c * x + y)(k(i)), nin=2) for i in range(3)], member_scalars=True)
    assert "f=axpy" in g.describe()
    g = group([member((lambda c: lambda x, y: (x + y) / c)(k(i)), nin=2) for i in range(3)], member_scalars=True)
    assert "f=sym" in g.describe()
    g = group([member((lambda c: lambda x: x * S.fn.exp(c * x) + S.fn.sin(x * x))(k(i))) for i in range(3)], member_scalars=True)
    assert "f=expr5" in g.describe()
    g = group([member((lambda c, d: lambda p, q: c * p + d * q * q)(k(i), h(i)), nin=2) for i in range(3)], member_scalars=True)
    assert "f=prog" in g.describe() and g.describe().endswith("scalars=member")
    # Float32 arrays times a Float64 scalar: a converting group, planned as a program
    g = group([member(scale(0.1 + i), dtype=np.float32) for i in range(3)], member_scalars=True)
    assert "f=prog" in g.describe() and g.describe().endswith("scalars=member")


def test_front_buckets_without_the_values():
    a, b, c = fresh((4, 4)), fresh((4, 4)), fresh((4, 4))
    da, db, dc = a.similar(), b.similar(), c.similar()
    g = Recorder(member_scalars=True)
    g.defer(scale(2), a.size, (da, a))
    g.defer(scale(3), a.size, (db, b))
    g.defer(scale(2.0), a.size, (dc, c))
    g.flush()
    assert g.launches == [[da, db, dc]]
    g = Recorder()                                  # the default: one bucket per value, as before
    g.defer(scale(2), a.size, (da, a))
    g.defer(scale(3), a.size, (db, b))
    g.flush()
    assert g.launches == [[da], [db]]
    g = Recorder(member_scalars=True)               # a real and a complex scalar compute in different classes
    g.defer(scale(2), a.size, (da, a))
    g.defer(scale(2 + 1j), a.size, (db, b))
    g.flush()
    assert g.launches == [[da], [db]]
    ia, ib, ic = (fresh((4, 4), np.int32) for _ in range(3))
    g = Recorder(member_scalars=True)               # an integer-valued and a fractional scalar on integer arrays
    g.defer(scale(3), ia.size, (ia.similar(), ia))
    g.defer(scale(2.5), ia.size, (ib.similar(), ib))
    g.defer(scale(-7), ia.size, (ic.similar(), ic))
    g.flush()
    assert [len(l) for l in g.launches] == [2, 1]
    g = Recorder(member_scalars=True)               # merged constants: a*X + a*Y is another program than a*X + b*Y
    x, y = fresh((4, 4)), fresh((4, 4))
    g.defer(axpby(2, 3), a.size, (da, x, y))
    g.defer(axpby(2, 2), a.size, (db, x, y))
    g.defer(axpby(5, 7), a.size, (dc, x, y))
    g.flush()
    assert g.launches == [[da, dc], [db]]


def test_front_conflict_flush_rule_is_unchanged():
    a, b, c = fresh((4, 4)), fresh((4, 4)), fresh((4, 4))
    da, db, dc = a.similar(), b.similar(), c.similar()
    g = Recorder(member_scalars=True)
    assert g.defer(scale(2), a.size, (da, a))
    assert g.defer(scale(3), a.size, (db, b))
    assert g.launches == []
    assert g.defer(scale(4), a.size, (dc, da))      # reads a pending destination
    assert g.launches == [[da, db]]
    g.flush()
    assert g.launches == [[da, db], [dc]]
    g = Recorder(member_scalars=True)
    g.defer(scale(2), a.size, (da, a))
    g.defer(scale(3), a.size, (a, b))               # writes what a pending call reads
    assert g.launches == [[da]]
    src, dst = fresh((8, 8)), fresh((8, 8))
    ev = [(dst.sview(slice(None), slice(k, None, 2)), src.sview(slice(None), slice(k, None, 2))) for k in (0, 1)]
    g = Recorder(member_scalars=True)
    for i, (d, s) in enumerate(ev):
        g.defer(scale(2 + i), d.size, (d, s))
    assert len(g.launches) == 1
    g = Recorder(member_scalars=True, independent=True)
    for i, (d, s) in enumerate(ev):
        g.defer(scale(2 + i), d.size, (d, s))
    assert g.launches == []
    g.flush()
    assert [len(l) for l in g.launches] == [2]


def test_the_group_cache_key_holds_the_flag(monkeypatch):
    """The same calls under both settings are two cached groups, each built with its own flag."""
    made = []

    class FakeGroup:
        def __init__(self, problems, independent=False, keepalive=(), member_scalars=False):
            made.append((len(problems), bool(member_scalars)))

        def execute(self, stream=None):
            pass

    monkeypatch.setattr(L, "Group", FakeGroup)
    a, b = fresh((4, 4)), fresh((4, 4))
    da, db = a.similar(), b.similar()
    f2, f3 = scale(2), scale(3)
    for own in (True, False, True, False):
        g = S.group(member_scalars=own)
        g.defer(f2, a.size, (da, a))
        g.defer(f3, a.size, (db, b))
        g.flush()
    assert made == [(2, True), (1, False), (1, False)]   # the third and fourth block found their groups in the cache


def test_sequence_analyses_see_a_flagged_group_like_a_plain_one():
    A = [fresh((6, 5)) for _ in range(4)]
    B = [fresh((6, 5)) for _ in range(4)]
    extra = fresh((6, 5))

    def grp(own):
        built = [S.build_problem(scale(1 + i / 8 if own else 2.5), None, None, d.size, (d, s), stream=0) for i, (d, s) in enumerate(zip(B, A))]
        return L.Group([b[0] for b in built], keepalive=built, member_scalars=own)

    plain, flagged = grp(False), grp(True)
    assert flagged.describe().endswith("scalars=member")
    reader = S.make_plan(ident, None, None, extra.size, (extra, B[1]))
    writer = S.make_plan(ident, None, None, extra.size, (A[2], extra))
    aside = S.make_plan(ident, None, None, extra.size, (fresh((6, 5)), fresh((6, 5))))
    for build in (lambda g: S.Sequence().add_group(g), lambda g: S.Sequence().add_group(g).add(reader), lambda g: S.Sequence().add(writer).add_group(g),
                  lambda g: S.Sequence().add_group(g).add(aside).add_group(g)):
        p, f = build(plain), build(flagged)
        assert p.components() == f.components()
        assert p.fences() == f.fences()
    assert S.Sequence().add_group(flagged).add(reader).components() == [0, 0]
    assert S.Sequence().add_group(flagged).fences()[1] == 8 * 6 * 5 * 8
