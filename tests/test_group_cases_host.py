"""Grouped launches, host side (no device): every recipe of tests/group_cases.py is planned on its host views through L.Group /
smr_group_create, and smr_group_layout / smr_group_describe must show that it hits what it claims -- the body of each member, the
canonical ranks, the position of the tiled dim, ragged last chunks, the member counts, the functor names.  A reader without a GPU can
check here what tests/test_gpu_group_fuzz.py covers.  Then: check_independent (csrc/smr_plan_group.cpp) against a brute-force pairwise test."""
import re

import numpy as np
import pytest

import group_cases as G
import strided_jl_amd as S
from strided_jl_amd import _lib as L
from test_group_host import create, problem

CASES = {}


def cases(name, dt=None):
    key = (name, dt)
    if key not in CASES:
        CASES[key] = [(c, G.build_group(c)) for c in G.recipe(name, dt)]
    return CASES[key]


def check_plan(c, g):
    """layout() and describe() of the planned group against the recipe's intentions"""
    d, lay = g.describe(), g.layout()
    assert len(lay) == len(c.calls) == len(c.info) and "members=%d " % len(c.calls) in d, (c, d)
    assert "f=%s " % c.fname in d and "jit=%d" % c.jit in d, (c, d)
    nxt = 0
    for i, ((form, first, wgs, rank), info) in enumerate(zip(lay, c.info)):
        assert (form, first, wgs, rank) == (info["form"], nxt, info["wgs"], info["rank"]), (c, i, info, lay[i])
        nxt += wgs
    assert "grid=%d " % nxt in d
    assert "linear=%d " % sum(1 for m in c.info if m["form"] == 0) in d and "transposing=%d " % sum(1 for m in c.info if m["form"] == 1) in d
    for f, arrays in c.calls:  # the destination's parent reaches beyond the view at both ends
        flat, shift = G.host_flat(arrays[0])
        idx = G.element_index(arrays[0], shift)
        assert 0 < idx.min() and idx.max() < flat.size - 1


def digits_of_256(dims):
    out, rem = [], 256
    for d in dims:
        if d > 1:
            out.append(rem % d)
            rem //= d
    return out


@pytest.mark.parametrize("dt", G.FLOATS)
def test_linear_recipe(dt):
    got = cases("linear", dt)
    assert [c.fname for c, _ in got] == ["ident", "add2"]
    for c, g in got:
        check_plan(c, g)
        info = c.info
        assert all(m["form"] == 0 for m in info)
        assert {m["total"] for m in info if len(m["dims"]) == 1} == {1, 255, 256, 257, 1023, 1024, 1025, 2049}
        assert {m["dims"][0] for m in info} >= {255, 256, 257, 300} and {4, 7, 8} <= {m["rank"] for m in info} and min(m["rank"] for m in info) == 1
        # a last workgroup with one element: only lane 0 holds one
        assert sum(1 for m in info if m["wgs"] >= 2 and m["total"] % G.CHUNK == 1) >= 2
        # radices in which 256 has three and more non-zero digits: the carries of the lane step ripple
        assert sum(1 for m in info if sum(1 for x in digits_of_256(m["dims"]) if x) >= 3) >= 3
        assert any(m["bcast"] for m in info)
    assert sum(1 for c, _ in got for m in c.info if m["bcast"]) >= 5  # one input in six of 48
    views = [a for c, _ in got for f, arrays in c.calls for a in arrays[1:]]
    assert any(min(a.strides) < 0 for a in views) and any(a.offset for a in views) and any(len(a.size) == 1 and abs(a.strides[0]) in (2, 3) for a in views)


@pytest.mark.parametrize("dt", G.FLOATS)
def test_transposing_recipe(dt):
    got = cases("transposing", dt)
    info = []
    for c, g in got:
        check_plan(c, g)
        info += c.info
        assert len({(m["nin"], m["kt"], m["conj"]) for m in c.info}) == 1
    assert all(m["form"] == 1 for m in info)
    assert {(m["p"], m["q"]) for m in info} == {(p, q) for p in G.EDGES for q in G.EDGES} and len(info) == 64
    assert {m["cq"] for m in info} == {1, 2, 3} and {m["rank"] for m in info} == {2, 3, 4}
    assert any(m["both_sides"] and m["cq"] >= 2 for m in info)
    assert {m["rev"] for m in info} == {"", "q", "p"} and {m["step2"] for m in info} == {False, True}
    assert {(m["nin"], m["kt"]) for m in info} == {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}
    assert {m["other"] for m in info if m["nin"] > 1} == {"dst", "b0", "bq"}
    assert {m["conj"] for m in info} == ({False, True} if G.is_complex(dt) else {False})
    for c, _ in got:  # what the planner reads: the staged input's strides, the destination's step, the broadcast companions
        for (f, arrays), m in zip(c.calls, c.info):
            st = arrays[1 + m["kt"]]
            qpos = st.strides.index(-1 if m["rev"] == "q" else 1)
            assert st.size[qpos] == m["q"] and (st.strides[0] < 0) == (m["rev"] == "p") and arrays[0].strides[0] == (2 if m["step2"] else 1)
            assert (st.op == "conj") == m["conj"]
            for k, a in enumerate(arrays[1:]):
                if k != m["kt"]:
                    assert a.strides[0] == (0 if m["other"] == "b0" else 1) and (a.strides[qpos] == 0) == (m["other"] == "bq")


def test_tmin_recipe():
    (c, g), = cases("tmin")
    check_plan(c, g)
    assert [(m["p"], m["q"]) for m in c.info] == G.TMIN_PLANES
    assert [r[0] for r in g.layout()] == [0, 0, 1, 0, 0]  # only (16, 16) has both dims at GROUP_TMIN


@pytest.mark.parametrize("dt", G.FLOATS)
def test_functors_recipe(dt):
    got = cases("functors", dt)
    names = ["ident", "add2", "add3", "add4", "scale", "sym", "axpy", "axpby", "abs2", "mul2"] + ([] if G.is_complex(dt) else ["expr5"])
    assert [c.fname for c, _ in got][:len(names)] == names
    for c, g in got:
        check_plan(c, g)
        assert "linear=3 transposing=3" in g.describe()
        nin = len(c.calls[0][1]) - 1
        assert {m["kt"] for m in c.info if m["form"]} == {0, 1 % nin, nin - 1}
    for c, g in got[:len(names)]:
        assert "jit=0" in g.describe() and c.jit == 0
    rest = [(c.name.split("/", 2)[2], c.fname, c.jit) for c, _ in got[len(names):]]
    assert rest == ([("float64/jit", "prog", 1), ("float64/jit", "prog", 1), ("float64/interpreted", "prog", 0)] if dt is np.float64 else [])


def test_interpreter_refuses_math_opcodes_in_a_group():
    a = S.StridedView(np.zeros((6, 5), order="F"))
    old = S.get_option("jit")
    S.set_option("jit", 0)
    try:
        rc, msg = create([problem(G.MATH_F, a.similar(), a, a.sview(slice(None), slice(None, None, -1)))])
    finally:
        S.set_option("jit", old)
    assert rc == L.SMR_EUNSUPPORTED and "member 0" in msg and "jit" in msg


def test_bitcopy_recipe():
    got = cases("bitcopy")
    assert [(c.fname, np.dtype(c.calls[0][1][0].dtype).itemsize) for c, _ in got] == [("bitcopy", 1), ("bitcopy", 2), ("bitcopy", 4), ("bitcopy", 8), ("ident", 16)]
    for c, g in got:
        check_plan(c, g)
        assert [r[0] for r in g.layout()] == [0, 1]


@pytest.mark.parametrize("dt", [np.int32, np.int64, np.uint8])
def test_integer_recipe(dt):
    got = cases("integer", dt)
    for c, g in got:
        check_plan(c, g)
        assert {r[0] for r in g.layout()} == {0, 1} and all(np.dtype(a.dtype) == np.dtype(dt) for f, arrays in c.calls for a in arrays)
    if dt is np.int64:
        assert [c.fname for c, _ in got] == ["scale", "add2", "prog"]


def test_mixed_recipe():
    got = cases("mixed")
    pairs = set()
    for c, g in got:
        check_plan(c, g)
        assert "f=prog" in g.describe() and "jit=1" in g.describe()
        for (f, arrays), m in zip(c.calls, c.info):
            if m["form"] == 1:  # the staged input has another type than the destination, or the call computes in another one
                pairs.add((np.dtype(arrays[0].dtype).name, np.dtype(arrays[1 + m["kt"]].dtype).name))
    assert pairs == {("float64", "float32"), ("float32", "float32")}


def test_counts_recipe():
    got = cases("counts")
    assert sorted({len(c.calls) for c, _ in got}) == list(G.COUNTS)
    for c, g in got:
        check_plan(c, g)
        K, lay = len(c.calls), g.layout()
        special = sorted({0, K // 2, K - 1})
        kinds = [(lay[i][0], lay[i][2]) for i in special]
        assert set(kinds) <= {(0, 2), (1, 4)} and all(a != b for a, b in zip(kinds, kinds[1:]))
        assert all(lay[i][2] == 1 and c.info[i]["total"] <= 40 for i in range(K) if i not in special)
    first_kinds = {(len(c.calls), g.layout()[0][0]) for c, g in got}
    assert all((K, form) in first_kinds for K in G.COUNTS if K <= 257 for form in (0, 1))


def test_runtime_compiled_signatures_stay_few():
    """every distinct runtime-compiled (f, operand types) of the GPU file costs one compilation there"""
    jit = [c.name for name, (_, types) in G.RECIPES.items() for dt in types for c, _ in cases(name, dt) if c.jit]
    assert len(jit) == len(set(jit)) <= 8, jit


def test_sliced_group_has_cuts_inside_both_bodies():
    c, cuts = G.sliced()
    g = G.build_group(c)
    check_plan(c, g)
    lay = g.layout()
    assert lay[-1][1] + lay[-1][2] == G.SEQ_GRID >= 256
    inside = {0: 0, 1: 0}
    for s in (2, 3, 4):
        assert len(cuts[s]) == s - 1
        hit = [r for x in cuts[s] for r in lay if r[1] < x < r[1] + r[2]]
        assert hit, (s, cuts[s])
        for r in hit:
            inside[r[0]] += 1
    assert inside[0] >= 1 and inside[1] >= 1
    carry = [m for m in c.info if m["form"] == 0 and m["rank"] >= 4]
    ragged = [m for m in c.info if m["form"] == 1 and m["outer"] > 1 and (m["p"] % G.TILE or m["q"] % G.TILE)]
    assert len(carry) >= 4 and len(ragged) >= 4


# ---- check_independent against a brute-force pairwise test ----------------------------------------------------------------------------
NPARENT, SEG = 640, 16   # elements of a shared parent; destinations of a conflict-free draw lie in segments of their own


def byte_range(v):
    """[lo, hi) of the bounding byte range of a view, as csrc/smr_group.h operand_span computes it"""
    lo = hi = v.offset
    for n, s in zip(v.size, v.strides):
        e = (n - 1) * s
        if e < 0:
            lo += e
        else:
            hi += e
    return v._base + lo * v.dtype.itemsize, v._base + (hi + 1) * v.dtype.itemsize


def draw_view(rng, parent, lo, hi, shape):
    """A view of `shape` (1-d or 2-d; stepped, reversed, either memory order) whose elements lie in [lo, hi) of the flat `parent`."""
    for _ in range(8):
        if len(shape) == 1:
            st = [int(rng.choice([1, 1, 2, 3]))]
        else:
            a, b = int(rng.choice([1, 1, 2])), int(rng.choice([1, 1, 2]))
            st = [a, shape[0] * a * b] if rng.integers(0, 2) else [shape[1] * a * b, a]
        span = 1 + sum((n - 1) * s for n, s in zip(shape, st))
        if span <= hi - lo:
            break
    else:
        st = [1] if len(shape) == 1 else [1, shape[0]]
        span = int(np.prod(shape))
    off = lo + int(rng.integers(0, hi - lo - span + 1))
    strides = []
    for n, s in zip(shape, st):
        if rng.integers(0, 3) == 0:
            off += (n - 1) * s
            s = -s
        strides.append(s)
    return S.StridedView(parent, shape, tuple(strides), off)


def same_operand(u, v):
    """one operand to the library: the same parent, offset and strides along every dim longer than 1"""
    key = lambda a: (a._base, a.offset, a.size, tuple(s for n, s in zip(a.size, a.strides) if n > 1))  # noqa: E731
    return key(u) == key(v)


def draw_members(seed):
    rng = np.random.default_rng([G.SEED_OFFSET, 77, seed])
    A, B = np.zeros(NPARENT), np.zeros(NPARENT)
    nin = int(rng.integers(1, 3))
    mode = int(rng.integers(0, 5))
    tidy = mode < 2                           # destinations in segments of their own in A, inputs in B: no conflict unless one is put in
    crowded = mode == 4                       # a few members inside one window of one parent: ranges nest, and a member's own far-reaching
    #                                           range hides the end of another member's behind it
    K = int(rng.integers(2, 41)) if tidy or mode == 2 else int(rng.integers(2, 5))
    hot = int(rng.integers(0, NPARENT - 3 * SEG))
    segs = rng.permutation(NPARENT // SEG)
    members, seen = [], []
    for i in range(K):
        shape = (int(rng.choice([1, 2, 5, 8, SEG])),) if rng.integers(0, 2) else (int(rng.integers(1, 5)), int(rng.integers(1, 5)))
        if tidy:
            dst = draw_view(rng, A, SEG * int(segs[i]), SEG * int(segs[i]) + SEG, shape)
        elif crowded:
            dst = draw_view(rng, A, hot, hot + 3 * SEG, shape)
        else:
            w = int(rng.integers(0, NPARENT - 4 * SEG))
            dst = draw_view(rng, (A, B)[int(rng.integers(0, 2))], w, w + 4 * SEG, shape)
        ins = []
        while len(ins) < nin:
            same = [v for v in seen if v.size == shape]
            r = int(rng.integers(0, 8))
            if r == 0 and same:
                v = same[int(rng.integers(0, len(same)))]            # identical to an earlier input
            elif r == 1 and not ins:
                v = dst                                               # in place
            elif r == 2 and same:
                o = same[int(rng.integers(0, len(same)))]            # nested: inside an earlier input's range
                lo, hi = [(x - o._base) // 8 for x in byte_range(o)]
                v = draw_view(rng, o.parent, lo, hi, shape) if hi - lo >= int(np.prod(shape)) else o
            elif crowded:
                v = draw_view(rng, A, hot, hot + 3 * SEG, shape) if rng.integers(0, 2) else draw_view(rng, B, 0, NPARENT, shape)
            else:
                v = draw_view(rng, B if tidy else (A, B)[int(rng.integers(0, 2))], 0, NPARENT, shape)
            if any(same_operand(u, v) for u in ins):
                continue  # (two identical inputs are one operand to the library: another f than the other members')
            ins.append(v)
        seen += ins
        members.append((dst, tuple(ins)))
    if tidy and rng.integers(0, 3) == 0:      # put one conflict in: a destination or an input drawn from another member's segment
        i, j = [int(x) for x in rng.choice(K, size=2, replace=False)]
        dst, ins = members[j]
        lo = SEG * int(segs[i])
        if rng.integers(0, 2):
            members[j] = (draw_view(rng, A, lo, lo + SEG, dst.size), ins)
        else:
            members[j] = (dst, (draw_view(rng, A, lo, lo + SEG, dst.size),) + ins[1:])
            if nin == 2 and same_operand(members[j][1][0], ins[1]):
                members[j] = (dst, ins)
    return nin, members


def conflicting_pairs(members):
    """(w, o): the destination's range of member w meets a range of another member o"""
    out = set()
    for w, (dst, _) in enumerate(members):
        wl, wh = byte_range(dst)
        for o, (d2, ins) in enumerate(members):
            if o != w and any(lo < wh and wl < hi for lo, hi in [byte_range(v) for v in (d2,) + ins]):
                out.add((w, o))
    return out


def test_check_independent_agrees_with_a_pairwise_test():
    fs = {1: G.ident, 2: lambda a, b: a + b}
    verdicts = {True: 0, False: 0}
    adjacent = 0
    seed = 0
    while seed < 300 or (min(verdicts.values()) < 50 and seed < 3000):
        nin, members = draw_members(seed)
        ms = [problem(fs[nin], dst, *ins) for dst, ins in members]
        rc, msg = create(ms)
        bad = conflicting_pairs(members)
        assert rc == (L.SMR_EUNSUPPORTED if bad else L.SMR_OK), (seed, msg, sorted(bad)[:4])
        if bad:
            m = re.search(r"member (\d+): the destination's byte range of member (\d+) meets a byte range of member (\d+)", msg)
            assert m, (seed, msg)
            tag, w, o = (int(x) for x in m.groups())
            assert (w, o) in bad and tag == max(w, o), (seed, msg, sorted(bad)[:8])
        else:
            ends = sorted(byte_range(dst) for dst, _ in members)
            adjacent += sum(1 for a, b in zip(ends, ends[1:]) if a[1] == b[0])
        verdicts[not bad] += 1
        seed += 1
    assert min(verdicts.values()) >= 50, verdicts
    assert adjacent >= 20  # accepted groups whose destinations touch: a range ends where the next one starts
