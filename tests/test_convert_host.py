"""The table of tests/convert_cases.py, checked without a device: the whole-parent checker reports a flipped byte inside the view and in the
pad; the model of Julia's conversions gives hand-written known answers; E.result_dtype agrees with the model's type for every expression of
the table; the CPU oracle equals the model bit for bit on every row with 1 and 3 threads; from describe() every row takes the converting
(mixed) instantiation of the family and form it names, every cell has float and integer destinations, and every admitted (source,
destination) pair is in STREAM, in TILED and in a reduction epilogue; the rows that compile f at runtime stay at 40 compiled kernels or
fewer; and the 64-bit integer inputs of a float class and UInt64 under an order test are refused."""
import collections
import functools

import numpy as np
import pytest

import convert_cases as CC
import oraclelib
import strided_jl_amd as S
import window_cases as W
from convert_cases import A, B, C32, C64, F32, F64, I8, I16, I32, I64, L, U8, U16, U32, U64

E = S.expr


# ---- the checker is checked ---------------------------------------------------------------------------------------------------------------
def _first(cell, **want):
    for s in CC.TABLE:
        if s["cell"] == cell and all(s.get(k) == v or (k == "dest" and np.dtype(s["dest"]) == v) for k, v in want.items()):
            return CC.build(s)
    raise KeyError((cell, want))


@pytest.mark.parametrize("cell,dest", [("stream1", F32), ("tiled", I16), ("row:split1", F32), ("accumulate", U64)])
def test_checker_reports_a_flipped_byte_inside_the_view_and_in_the_pad(cell, dest):
    r = _first(cell, dest=dest)
    assert r.inside.any() and not r.inside.all()
    good = r.expected.copy()
    assert r.mismatch(good) is None and r.mismatch(good.view(np.uint8)) is None
    isz = good.dtype.itemsize
    outside, inside = np.flatnonzero(~r.inside), np.flatnonzero(r.inside)
    for e, label in ((int(outside[0]), "outside"), (int(outside[-1]), "outside"), (int(inside[0]), "inside"), (int(inside[-1]), "inside")):
        for byte in (0, isz - 1):
            bad = good.copy()
            bad.view(np.uint8)[e * isz + byte] ^= 0x10
            msg = r.mismatch(bad, "DESCRIBE-TEXT")
            assert msg is not None and msg.startswith("element %d " % e) and "(%s the view)" % label in msg and "DESCRIBE-TEXT" in msg and r.name in msg, msg
            assert "1 of %d elements differ" % good.size in msg, msg
    assert r.mismatch(r.before) is not None          # the destination as allocated is not the result
    assert "bytes, expected" in r.mismatch(good[:-1])


# ---- the model against hand-written known answers -------------------------------------------------------------------------------------------
def _one(tree, *vals):
    return CC.evaluate(tree, [np.array([v]) for v in vals])[0]


def test_model_known_answers():
    cv = CC.convert
    assert cv(np.array([16777217], I32), F32)[0] == np.float32(16777216) and cv(np.array([16777217], I32), F32).dtype == F32   # tie, to even
    assert cv(np.array([16777219], I32), F32)[0] == np.float32(16777220)                                                      # tie, to even (up)
    assert cv(np.array([16777219.0]), F32)[0] == np.float32(16777220)
    assert cv(np.array([-16777217], I64), F32)[0] == np.float32(-16777216)
    assert cv(np.array([2 ** 32 - 1], U32), F32)[0] == np.float32(4294967296.0) and cv(np.array([2 ** 32 - 128], U32), F32)[0] == np.float32(4294967296.0)
    assert cv(np.array([2 ** 31 - 64], I32), F32)[0] == np.float32(2147483648.0) and cv(np.array([2 ** 31 - 65], I32), F32)[0] == np.float32(2147483520.0)
    # Float32[1] .+ Int32[16777217]: the Int32 is converted first
    r = _one(("add", A(0), A(1)), np.float32(1), np.int32(16777217))
    assert r.dtype == F32 and r == np.float32(16777216)
    r = _one(("add", A(0), L(16777217)), np.float32(1))
    assert r.dtype == F32 and r == np.float32(16777216)
    assert _one(("add", A(0), A(1)), np.float64(1), np.int32(16777217)) == 16777218.0
    # UInt64 of floats at and above 2^63
    for v in (2.0 ** 64 - 2048, 2.0 ** 63, 2.0 ** 63 + 2048, 2.0 ** 63 - 1024):
        got = cv(np.array([v]), U64)
        assert got.dtype == U64 and int(got[0]) == int(v)
    assert int(cv(np.array([2.0 ** 64 - 2048]), U64)[0]) == 18446744073709549568
    assert int(cv(np.array([-2.0 ** 63]), I64)[0]) == -2 ** 63
    # Float32(nextfloat of the midpoint between 1 and nextfloat(1f0)) rounds up, the midpoint itself to even (down), the one above it up
    mid = 1.0 + 2.0 ** -24
    assert cv(np.array([mid]), F32)[0] == np.float32(1) and cv(np.array([np.nextafter(mid, 2.0)]), F32)[0] == np.float32(1 + 2.0 ** -23)
    assert cv(np.array([1.0 + 3 * 2.0 ** -24]), F32)[0] == np.float32(1 + 2.0 ** -22)
    thr = (2.0 - 2.0 ** -24) * 2.0 ** 127
    assert cv(np.array([np.nextafter(thr, 0.0)]), F32)[0] == np.finfo(np.float32).max and np.isinf(cv(np.array([thr]), F32)[0])
    assert cv(np.array([2.0 ** -150]), F32)[0] == 0 and cv(np.array([np.nextafter(2.0 ** -150, 1.0)]), F32)[0] == np.float32(2.0 ** -149)
    assert np.signbit(cv(np.array([-2.0 ** -151]), F32)[0])
    # integer typing
    r = _one(("add", A(0), A(1)), np.int8(-1), np.uint8(0))
    assert r.dtype == U8 and r == 255                                    # Int8 + UInt8 is a UInt8 that wraps
    r = _one(("add", A(0), A(1)), np.int8(-128), np.uint8(255))
    assert r.dtype == U8 and r == 127
    r = _one(("add", A(0), A(1)), np.int32(-1), np.uint32(0))
    assert r.dtype == U32 and r == 2 ** 32 - 1                           # Int32 + UInt32 is a UInt32
    assert _one(("add", A(0), A(1)), np.int64(-1), np.uint64(1)).dtype == U64
    assert _one(("div", A(0), A(1)), np.int32(1), np.int16(3)).dtype == F64
    assert _one(("div", A(0), A(1)), np.float32(1), np.int64(3)) == np.float32(1) / np.float32(3)
    assert _one(("add", A(0), A(1)), True, True).dtype == I64 and _one(("add", A(0), A(1)), True, True) == 2
    assert _one(("mul", A(0), A(1)), True, False).dtype == B
    assert _one(("mul", A(0), A(1)), np.complex64(1 + 2j), np.int32(3)).dtype == C32
    assert _one(("sqrt", A(0)), np.int16(4)).dtype == F64
    assert bool(_one(("lt", A(0), A(1)), np.float32(16777216), np.int32(16777217)))   # mathematical: Float32(16777217) == 16777216 is not asked
    with pytest.raises(AssertionError):
        cv(np.array([1.5]), I32)
    with pytest.raises(AssertionError):
        cv(np.array([256.0]), U8)
    with pytest.raises(AssertionError):
        cv(np.array([1 + 1j]), F64)
    assert CC.promote_type(F32, I64) == F32 and CC.promote_type(C32, I32) == C32 and CC.promote_type(C32, F64) == C64 and CC.promote_type(B, U8) == U8
    assert CC.promote_type(I8, U16) == U16 and CC.promote_type(I16, U16) == U16 and CC.promote_type(I64, U8) == I64


def test_value_sets_hold_the_edges():
    assert {2 ** 24 + 1, -(2 ** 24 + 3), 2 ** 31 - 1, 2 ** 31 - 64, -2 ** 31} <= set(CC.int_values(I32))
    assert {2 ** 32 - 1, 2 ** 32 - 128, 0} <= set(CC.int_values(U32)) and set(CC.int_values(B)) == {0, 1} and set(CC.int_values(I8)) == {-128, -1, 0, 1, 127}
    assert {2 ** 63 - 1024, 2 ** 63, 2 ** 63 + 2048, 2 ** 64 - 2048} <= set(CC.float_to_int_values(F64, U64))
    assert {-2 ** 63, 2 ** 63 - 1024} <= set(CC.float_to_int_values(F64, I64))
    assert {2 ** 63, 2 ** 64 - 2 ** 40, -0 + 2 ** 63 + 2 ** 40} <= set(CC.float_to_int_values(F32, U64)) and 2 ** 63 - 1024 not in CC.float_to_int_values(F32, U64)
    assert {2 ** 31 - 1, -2 ** 31} <= set(CC.float_to_int_values(F64, I32)) and {2 ** 31 - 128, -2 ** 31} <= set(CC.float_to_int_values(F32, I32))
    v = np.array(CC.f64_to_f32_values())
    assert np.isnan(v).any() and np.isinf(v).sum() == 2 and (np.signbit(v) & (v == 0)).any()
    with np.errstate(over="ignore"):
        w = v.astype(np.float32)
    assert (np.isinf(w) & ~np.isinf(v)).sum() >= 4 and ((w == 0) & (v != 0)).sum() >= 4 and ((w != 0) & (np.abs(w) < np.finfo(np.float32).tiny)).sum() >= 6


# ---- typing: E.result_dtype is the model's type ---------------------------------------------------------------------------------------------
def _typing_cases():
    seen, out = set(), []
    for s in CC.TABLE:
        key = (CC.show(s["tree"]), tuple(np.dtype(t) for t in s["types"]))
        if key not in seen:
            seen.add(key)
            out.append((s["tree"], key[1]))
    return out + [(t, tuple(ts)) for t, ts in CC.TYPING]


def test_result_dtype_is_the_models_type_for_every_expression_of_the_table():
    bad = []
    for tree, types in _typing_cases():
        want = CC.result_type(tree, types)
        got = E.result_dtype(E.trace(CC.library_function(tree), len(types)), list(types))
        if got != want:
            bad.append("%s of %s: %s, Julia %s" % (CC.show(tree), [CC.NAMES[t] for t in types], got, CC.NAMES[want]))
    assert not bad, bad


def test_result_dtype_known_answers():
    def rd(f, *types):
        return E.result_dtype(E.trace(f, len(types)), list(types))
    assert rd(lambda a, b: a + b, F32, I32) == F32 and rd(lambda a, b: a / b, F32, I64) == F32
    assert rd(lambda a, b: a * b, C32, I32) == C32
    assert rd(lambda a, b: a + b, I32, U32) == U32 and rd(lambda a, b: a + b, I8, U8) == U8 and rd(lambda a, b: a + b, I64, U64) == U64
    assert rd(lambda a, b: a / b, I32, I16) == F64 and rd(lambda a, b: a + b, B, B) == I64 and rd(lambda a, b: a - b, B, B) == I64
    assert rd(lambda a, b: S.fn.max(a, b), F32, I32) == F32 and rd(lambda a: a + 16777217, F32) == F32


def test_sums_and_products_widen_small_integers_as_base_add_sum_does():
    from strided_jl_amd.mapreduce import _reduced_dtype
    for op in ("+", "*"):
        for t, want in ((U8, U64), (U16, U64), (U32, U64), (U64, U64), (B, I64), (I8, I64), (I16, I64), (I32, I64), (I64, I64), (F32, F32), (C32, C32)):
            v = S.StridedView(np.zeros((3, 2), dtype=t, order="F"))
            assert _reduced_dtype(E.trace(lambda x: x, 1), op, v) == want, (op, t)
    v = S.StridedView(np.zeros((3, 2), dtype=U8, order="F"))
    assert _reduced_dtype(E.trace(lambda x: x, 1), "max", v) == U8


# ---- the oracle equals the model; what the rows reach ---------------------------------------------------------------------------------------
def signature(plan, desc):
    """What one runtime compilation is made from: the functor's source and the kernel variant of the family."""
    keys = ("family", "ct", "form", "fold", "vec", "tile", "staged", "threads", "mode", "lanes_per_out")
    return (plan.jit_source(),) + tuple(W.token(desc, k) if k != "family" else W.family(desc) for k in keys) + \
        ((CC.stream_form(desc, None),) if W.family(desc) == "stream" else ()) + (" wide" in desc,)


@functools.lru_cache(maxsize=None)
def survey(cell):
    """Every row of a cell through the CPU oracle with 1 and 3 threads: (failures, [(cell reached, mixed, types, spec)], signatures)."""
    bad, reach, sigs = [], [], set()
    old = S.get_option("jit")
    try:
        for r in CC.rows(cell):
            S.set_option("jit", 1 if r.jit else 0)
            plan = r.plan()
            r.desc = plan.describe()
            reach.append((CC.reached(r.desc, r.types), "(mixed)" in r.desc, r.types, r.spec, r.desc))
            if r.jit:
                sigs.add(signature(plan, r.desc))
            plan.close()
            for threads in (1, 3):
                r.reset()
                p, keep = S.build_problem(r.f, r.op, r.initop, r.dims, r.arrays, stream=0)
                oraclelib.mapreduce(p, threads)
                msg = r.mismatch(r.arrays[0].parent) or r.inputs_changed({a.parent.ctypes.data: a.parent for a in r.arrays[1:]})
                if msg:
                    bad.append("%d threads: %s" % (threads, msg))
    finally:
        S.set_option("jit", old)
    return bad, reach, sigs


NAMED = {"stream2c": "stream2", "tiled3": "tiled"}   # (cells that differ in shape only)


@pytest.mark.parametrize("cell", CC.cells())
def test_oracle_equals_the_model_bit_for_bit_and_rows_reach_their_cell(cell):
    bad, reach, _ = survey(cell)
    assert reach
    assert not bad, "%d of %d rows differ, the first: %s" % (len(bad), len(reach), bad[0])
    for got, mixed, types, spec, desc in reach:
        assert got == NAMED.get(cell, cell) and mixed, "%s: reached %s | %s" % (spec["name"], got, desc)


def test_every_cell_has_float_and_integer_destinations_and_every_pair_is_in_three_families():
    per_cell = collections.defaultdict(lambda: [0, 0])
    seen = collections.defaultdict(set)
    for cell in CC.cells():
        for got, mixed, types, spec, desc in survey(cell)[1]:
            per_cell[got][0 if CC.is_float(types[0]) else 1] += 1
            if spec.get("pair"):
                seen[(types[1], types[0])].add(W.family(desc) if spec.get("op") is None else W.token(desc, "fold"))
    want = ["stream0", "stream1", "stream2", "tiled", "generic", "all:epilogue", "all:second-launch", "row:split1", "row:in-launch", "col:in-launch",
            "col:second-launch", "accumulate"]
    short = {c: per_cell[c] for c in want if per_cell[c][0] < 2 or per_cell[c][1] < 2}
    assert not short, "cells with fewer than 2 float or 2 integer destinations (float, integer): %s" % short
    pairs = CC.admitted_pairs()
    assert len(pairs) == 7 * 4 + 4 * 9 + 12
    missing = {CC._pair_name(s, d): sorted(seen[(s, d)]) for s, d in pairs if seen[(s, d)] != {"stream", "tiled", "epilogue"}}
    assert not missing, missing
    # GENERIC is reachable with converting operands (strided along every dim, no dim of 64): the table has rows there


def test_group_rows_take_both_bodies_of_the_grouped_kernel():
    for cell, form in (("group:linear", 0), ("group:tiled", 1)):
        members = CC.group_rows(cell)
        g = CC.build_group(members)
        d = g.describe()
        assert "family=group" in d and "f=prog" in d, d   # (converting members run the f-program body: no native functor)
        assert [m[0] for m in g.layout()] == [form] * len(members), (cell, g.layout())
        for r in members:
            p, keep = S.build_problem(r.f, None, None, r.dims, r.arrays, stream=0)
            oraclelib.mapreduce(p, 1)
            assert r.mismatch(r.arrays[0].parent) is None, r.mismatch(r.arrays[0].parent)


def test_runtime_compiled_signatures_stay_few():
    """every distinct (functor source, kernel variant) among the rows that also run runtime-compiled costs one compilation in the GPU file;
    the other rows run interpreted (jit = 0)"""
    sigs = set()
    for cell in CC.cells():
        sigs |= survey(cell)[2]
    assert 0 < len(sigs) <= 40, len(sigs)
    jit_pairs = {(np.dtype(s["types"][0]), np.dtype(s["dest"])) for s in CC.TABLE if s.get("pair") and s.get("jit")}
    assert jit_pairs == set(CC.admitted_pairs())   # the pure conversions all run both ways


def test_converting_kernels_compile_at_runtime_for_gfx950():
    """One flagged row of every family through the runtime compiler (which cross-compiles without a device): the converting (MIXED)
    instantiation with the generated functor builds, nothing is precompiled for these rows, and no compilation fails -- on the device a
    failure would fall back to the interpreter silently, which tests/test_gpu_convert.py guards against with the same counters."""
    picks = {}
    for s in CC.TABLE:
        if s.get("jit"):
            picks.setdefault(s["cell"].split(":")[0] if s["cell"] != "accumulate" else "accumulate", s)
    assert set(picks) >= {"stream1", "tiled", "all", "row", "col", "accumulate"}, sorted(picks)
    old = S.get_option("jit")
    S.set_option("jit", 1)
    try:
        for key in ("stream1", "tiled", "all", "row", "accumulate"):
            r = CC.build(picks[key])
            before = [S.get_option(k) for k in ("jit_compiles", "jit_hits", "jit_failures")]
            plan = r.plan()
            size = plan.jit_compile()
            plan.close()
            c, h, f = [S.get_option(k) for k in ("jit_compiles", "jit_hits", "jit_failures")]
            assert size > 0 and f == before[2] and c + h > before[0] + before[1], (r.name, size, before, (c, h, f))
    finally:
        S.set_option("jit", old)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tree,types,dest,op", CC.REFUSALS, ids=[r[0] for r in CC.REFUSALS])
def test_refused_on_the_device(name, tree, types, dest, op):
    rng = np.random.default_rng(5)
    dims = (12, 5)
    ins = [CC.new_input(dims, (0, 1), [1, 0], [1, 1], t, np.arange(60) % 2) for t in types]
    out = CC.new_dest(rng, dims, (0, 1), [1, 1], [0, 1], dest, bcast=(1,) if op else (), old=np.zeros(12) if op else None)
    with pytest.raises(S._lib.UnsupportedOnDevice):
        S.make_plan(CC.library_function(tree), op, None, dims, [out] + ins)


def test_flat_and_orbit_refuse_converting_operands():
    """the FLAT and ORBIT planners take typed operands only: the shapes of their window recipes, with a destination of another type, plan
    as another family"""
    rng = np.random.default_rng(6)
    for dims, perm in W.FLAT_TWO + [((3, 480, 64), (2, 1, 0)), ((9, 11, 800), (1, 0, 2))]:
        N = len(dims)
        typed = S.make_plan(lambda x: x, None, None, dims, (W.dest_view(rng, dims, W.ident_perm(N), [0] * N, [0] * N, F32), W.input_view(rng, dims, perm, [0] * N, [0] * N, F32)))
        mixed = S.make_plan(lambda x: x, None, None, dims, (W.dest_view(rng, dims, W.ident_perm(N), [0] * N, [0] * N, F64), W.input_view(rng, dims, perm, [0] * N, [0] * N, F32)))
        dt, dm = typed.describe(), mixed.describe()
        typed.close(); mixed.close()
        assert W.family(dt) == "flat" and W.family(dm) not in ("flat", "orbit") and "(mixed)" in dm, (dt, dm)
    dims = (16, 16, 16, 16)
    a = W.input_view(rng, dims, W.ident_perm(4), [0] * 4, [0] * 4, F32)
    views = [S.StridedView(a.parent, dims, tuple(a.strides[p[i]] for i in range(4)), a.offset) for p in W.CYCLIC]
    f4 = lambda a, b, c, d: a + b + c + d   # noqa: E731
    typed = S.make_plan(f4, None, None, dims, [W.dest_view(rng, dims, W.ident_perm(4), [0] * 4, [0, 0, 0, 1], F32)] + views)
    mixed = S.make_plan(f4, None, None, dims, [W.dest_view(rng, dims, W.ident_perm(4), [0] * 4, [0, 0, 0, 1], F64)] + views)
    dt, dm = typed.describe(), mixed.describe()
    typed.close(); mixed.close()
    assert W.family(dt) == "orbit" and W.family(dm) not in ("flat", "orbit") and "(mixed)" in dm, (dt, dm)
