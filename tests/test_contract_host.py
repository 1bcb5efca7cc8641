"""The CONTRACT family's planner without a device: smr_plan_create and describe() need none.

The shape rules against the table of tests/contract_cases.py (the expected family per row is written there), the tile geometry,
the "contract" option's three values, and the default gate on a pinned sample of the reduction and window fuzz tables."""
import os

import numpy as np
import pytest

import contract_cases as CC
import reduce_fuzz_cases as RF
import strided_jl_amd as S
import window_cases as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = CC.table()


def mul_views(m, n, k, dt):
    mk = lambda *shape: S.StridedView(np.zeros(shape, dtype=dt, order="F"))  # noqa: E731
    return mk(m, n), mk(m, k), mk(k, n)


def mul_plan_desc(m, n, k, dt):
    """describe() of the plan S.mul_(C, A, B) makes: the box of linalg._matmul_."""
    C, A, B = mul_views(m, n, k, dt)
    c = CC.Case("mul", (m, n, k), CC.MM, (dt,) * 3, None)
    A2 = S.StridedView(A.parent, (m, 1, k), (A.strides[0], 0, A.strides[1]), A.offset, A.op)
    B2 = S.StridedView(B.parent, (1, n, k), (0, B.strides[1], B.strides[0]), B.offset, B.op)
    C2 = S.StridedView(C.parent, (m, n, 1), (C.strides[0], C.strides[1], 0), C.offset, C.op)
    p = c.plan((C2, A2, B2))
    d = p.describe()
    p.close()
    return d


def test_mul_256_f64_is_planned_as_a_contraction_by_default():
    """At 256^3 the planner takes 16 x 16 tiles (256 workgroups, one per CU).  Measured (tools/contract_cases.py, MI355X, us per launch,
    median +- spread): Float64 REDUCE_PART 15.0 against CONTRACT 10.6 (1.41x), Float32 10.2 against 7.6 (1.36x); spread under 0.1 us."""
    assert S.get_option("contract") == 1
    d = mul_plan_desc(256, 256, 256, np.float64)
    assert CC.family(d) == "contract", d
    with CC.option("contract", 0):
        d0 = mul_plan_desc(256, 256, 256, np.float64)
    assert CC.family(d0) == "reduce_part", d0


def test_option_values():
    """0 never, 2 wherever the shape qualifies, 1 only above the measured thresholds (profiles/contract_cases.txt)."""
    for c, want in ((0, "reduce_part"), (2, "contract"), (1, "reduce_part")):
        with CC.option("contract", c):
            assert CC.family(mul_plan_desc(40, 40, 40, np.float32)) == want
    with CC.option("contract", 1):
        assert CC.family(mul_plan_desc(1024, 1024, 1024, np.float32)) == "contract"
        assert CC.family(mul_plan_desc(512, 512, 512, np.float64)) == "contract"     # 256 output tiles: measured 2.0x
        assert CC.family(mul_plan_desc(256, 256, 256, np.float32)) == "contract"     # 256 tiles of 16 x 16: measured 1.36x
        assert CC.family(mul_plan_desc(128, 128, 64, np.float32)) == "reduce_part"   # 64 tiles: under a workgroup per CU
        assert CC.family(mul_plan_desc(64, 64, 4096, np.float32)) == "reduce_part"   # few outputs, long k: the split forms' ground


@pytest.mark.parametrize("case", ROWS, ids=[c.name for c in ROWS])
def test_shape_rules(case):
    with CC.option("contract", 2):
        ops = case.build()
        p = case.plan(ops, "zero" if case.op else None)
        d = p.describe()
        alg = p.algorithmic_bytes
        p.close()
    assert CC.family(d) == case.family, d
    with CC.option("contract", 0):
        p0 = case.plan(ops, "zero" if case.op else None)
        d0, alg0 = p0.describe(), p0.algorithmic_bytes
        p0.close()
    assert CC.family(d0) != "contract", d0
    assert alg == alg0
    if case.family != CC.CONTRACT:
        return
    # geometry: the tile dims are kept dims, the grid covers the outputs, the LDS fits
    di, ti, dj, tj, tk = CC.tile_of(d)
    cdims = [int(x) for x in CC.field(d, "dims").split("x")]
    nk = len(cdims) - len([r for r in case.rdims if case.dims[r] > 1])
    assert di != dj and di < nk and dj < nk, d
    rest = int(np.prod([cdims[x] for x in range(nk) if x not in (di, dj)]))
    assert int(CC.field(d, "grid")) == -(-cdims[di] // ti) * -(-cdims[dj] // tj) * rest, d
    assert int(CC.field(d, "lds")) <= min(65536, S.get_option("max_lds_bytes")), d
    assert int(CC.field(d, "vec")) in (1, 2, 4) and tk >= 1


def _contract_plans(types):
    """(case, describe()) of every CONTRACT row of the given types, planned under contract = 2."""
    out = []
    with CC.option("contract", 2):
        for case in ROWS:
            if case.family == CC.CONTRACT and case.dts in types:
                p = case.plan(case.build())
                out.append((case, p.describe()))
                p.close()
    return out


def test_the_table_reaches_every_tile_size_with_whole_and_several_chunks():
    """16 x 16 (one output per lane), 32 x 32 and 64 x 64 tiles are three instantiations of the kernel.  For each of them and each of
    Float32, Float64, ComplexF64 and Int64 the table must hold rows whose inner reduced extent K is exactly one chunk (the unrolled
    body), one chunk and a row, and more than two chunks (the double-buffer swap in its steady state), and a row with two reduced
    dims that spans several chunks per outer index; the mixed, ComplexF32 and Int32 rows reach more than two chunks on each tile."""
    four = [CC.TYPES[t] for t in ("f32", "f64", "c64", "i64")]
    for tn, dts in CC.TYPES.items():
        seen = {}
        for case, d in _contract_plans([dts]):
            _, ti, _, _, tk = CC.tile_of(d)
            cdims = [int(x) for x in CC.field(d, "dims").split("x")]
            nred = len([r for r in case.rdims if case.dims[r] > 1])
            K = cdims[len(cdims) - nred]   # the inner reduced dim: the first reduced extent listed
            seen.setdefault(ti, []).append((K, tk, nred, int(CC.field(d, "vec")), case.name))
        assert sorted(seen) == [16, 32, 64], (tn, sorted(seen))
        for tile, rows in seen.items():
            assert any(K > 2 * tk for K, tk, *_ in rows), (tn, tile, "no row with more than two chunks")
            if dts not in four:
                continue
            assert any(K == tk for K, tk, *_ in rows), (tn, tile, "no row of exactly one chunk")
            assert any(K == tk + 1 for K, tk, *_ in rows), (tn, tile, "no row of one chunk and a row")
            assert any(nred == 2 and K > tk for K, tk, nred, *_ in rows), (tn, tile, "no row with two reduced dims over several chunks")
            if tn != "c64":  # (16-byte elements are their own vector)
                assert any(vec > 1 and K >= 2 * tk for K, tk, _, vec, _ in rows), (tn, tile, "no vector-load row past the first chunk")
                assert any(vec > 1 and K > 2 * tk for K, tk, _, vec, _ in rows), (tn, tile, "no vector-load row with a ragged last chunk")


def test_the_chunk_rows_get_the_tile_they_are_listed_under():
    for case, d in _contract_plans(list(CC.TYPES.values())):
        for tile in (32, 64):
            if "/t%d_" % tile in case.name:
                assert CC.tile_of(d)[1] == tile and CC.tile_of(d)[3] == tile, (case.name, d)


JIT_PLANS = [  # (tile, type, f, op): a runtime-compiled f on every tile size; (tile 16: one box of whole tiles)
    (16, "f32", "dist", "+"), (16, "mixed", "mul", "+"), (32, "f64", "plus", "min"), (32, "i64", "dist", "+"), (64, "c64", "dist", "+"),
    (64, "f32", "asym", "+")]


@pytest.mark.parametrize("tile,tn,f,op", JIT_PLANS, ids=["t%d-%s-%s" % p[:3] for p in JIT_PLANS])
def test_the_contract_source_compiles_at_run_time(tile, tn, f, op):
    """The launchers fall back to the interpreter when runtime compilation is unavailable, so a result alone cannot tell the two apart
    (tests/test_gpu_contract.py reads the library's counters as well): the family's source must compile for the plan's f-program
    here, where gfx950 cross-compiles without a device."""
    tk = CC.tile_numbers(tn, tile)[2]
    kept = (64, 64) if tile == 16 else CC.TILE_SHAPES[tile][0]
    case = CC.Case("jit/%s" % tn, kept + (tk + 1,), CC.MM if tile == 16 else CC.BATCH, CC.TYPES[tn], CC.CONTRACT, f=f, op=op)
    with CC.option("contract", 2):
        p = case.plan(case.build(), None)
        d = p.describe()
        assert CC.family(d) == "contract" and CC.tile_of(d)[1] == tile, d
        before = S.get_option("jit_failures")
        n = p.jit_compile()
        p.close()
    assert n > 1000, d
    assert S.get_option("jit_failures") == before


def test_the_default_gate_leaves_interpreted_f_and_short_inner_dims_alone():
    """contract = 1 with jit = 0: the product of same-typed operands is compiled natively and stays; every other f would be interpreted
    (kernels with scratch memory, never measured) and goes to REDUCE_PART.  The reduced-length threshold is on the inner reduced dim,
    the one walked in chunks: 2 x 64 reduced elements with an inner extent of 2 are chunks of two rows."""
    big = CC.Case("gate", (512, 512, 64), CC.MM, CC.TYPES["f32"], CC.CONTRACT, layouts=("whole",) * 3)
    dist = CC.Case("gate", (512, 512, 64), CC.MM, CC.TYPES["f32"], CC.CONTRACT, layouts=("whole",) * 3, f="dist")
    mixed = CC.Case("gate", (512, 512, 64), CC.MM, CC.TYPES["mixed"], CC.CONTRACT, layouts=("whole",) * 3)
    short = CC.Case("gate", (512, 512, 2, 64), ((0, 1), (0, 2, 3), (1, 2, 3)), CC.TYPES["f32"], CC.CONTRACT)
    long_ = CC.Case("gate", (512, 512, 64, 2), ((0, 1), (0, 2, 3), (1, 2, 3)), CC.TYPES["f32"], CC.CONTRACT)

    def fam(case):
        p = case.plan(case.build())
        d = p.describe()
        p.close()
        return CC.family(d)

    assert S.get_option("contract") == 1
    assert [fam(c) for c in (big, dist, mixed, long_)] == ["contract"] * 4
    assert fam(short) == "reduce_part"
    with CC.option("jit", 0):
        assert fam(big) == "contract"
        assert fam(dist) == "reduce_part" and fam(mixed) == "reduce_part"


@pytest.mark.parametrize("tn", sorted(CC.TYPES))
def test_a_smaller_lds_budget_shrinks_the_tile_or_refuses(tn):
    for shape in ((2048, 2048, 64), (64, 64, 16)):
        c = CC.Case("lds/%s" % tn, shape, CC.MM, CC.TYPES[tn], CC.CONTRACT, layouts=("whole",) * 3)
        ops = c.build()
        with CC.option("contract", 2):
            p = c.plan(ops)
            d = p.describe()
            p.close()
            with CC.option("max_lds_bytes", 16384):
                p = c.plan(ops)
                d2 = p.describe()
                p.close()
        assert CC.family(d) == "contract" and int(CC.field(d, "lds")) <= 65536, d
        if CC.family(d2) == "contract":
            assert int(CC.field(d2, "lds")) <= 16384, d2
            if int(CC.field(d, "lds")) > 16384:  # it did not fit: a smaller tile
                assert CC.tile_of(d2)[1] < CC.tile_of(d)[1], (d, d2)
        else:
            assert CC.family(d2) == "reduce_part", d2


def sample_names():
    with open(os.path.join(HERE, "golden", "contract_gate_sample.txt")) as fh:
        return [ln.strip() for ln in fh if ln.strip() and not ln.startswith("#")]


def describe_named(name):
    table, recipe, seed, t = name.split(":")
    if table == "reduce":
        return RF.host_describe(RF.build(recipe, int(seed), t))
    case = W.build(recipe, int(seed), np.dtype(t))
    p = case.plan()
    d = p.describe()
    p.close()
    return d


def test_the_default_gate_steals_nothing_from_the_fuzz_tables():
    """describe() of a pinned sample of tests/reduce_fuzz_cases.py and tests/window_cases.py is identical under contract = 1 and
    contract = 0, unless the row is of the contraction shape and above the thresholds.  That exception covered 0 rows when the sample
    was pinned: those tables hold reductions of one input, or of inputs that vary along the same dims."""
    names = sample_names()
    assert len(names) >= 30
    moved = []
    for name in names:
        with CC.option("contract", 1):
            d1 = describe_named(name)
        with CC.option("contract", 0):
            d0 = describe_named(name)
        if d1 != d0:
            assert CC.family(d1) == "contract", (name, d1, d0)
            moved.append(name)
    assert moved == [], moved
