"""GPU: every reduction path bit-exactly at its planning boundaries.

The cases come from reduce_exact_cases.py (checked on the CPU oracle by test_reduce_exact_oracle.py): integer-valued data
bounded so that any reduction order gives the same bits, products of powers of two, min / max with planted extremes, NaN,
signed zeros and Inf.  Every case must match the table bit for bit, leave every byte of the destination's parent outside
its elements unchanged, and run on the kernel path the table names -- checked through describe(), which reports the
vector width and the fold form the launch takes (smr_plan_reduce.cpp: reduce_launch).  Then determinism (order-sensitive random
data: two executions and a fresh plan agree bitwise) and accumulation precision (the error bound of the launch geometry,
far below the serial chain's), and a final check that every cell of the coverage table was reached.
"""
import math

import numpy as np
import pytest

import reduce_exact_cases as RC
import strided_jl_amd as S
from strided_jl_amd import _lib as L
from test_reduce_exact_oracle import F, TABLE, views

pytestmark = pytest.mark.gpu

REACHED = {}  # cell -> describe() of a case that reached it


@pytest.fixture
def option():
    lib = L.load()
    saved = {}

    def setopt(name, value):
        if name not in saved:
            saved[name] = lib.smr_get_option(name.encode())
        L.check(lib.smr_set_option(name.encode(), value))

    yield setopt
    for k, v in saved.items():
        L.check(lib.smr_set_option(k.encode(), v))


def cur():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def cuda(a):
    import torch
    if a.dtype == np.bool_:
        return torch.from_numpy(a.view(np.uint8)).cuda().view(torch.bool)
    return torch.from_numpy(a).cuda()


def host_parent(view):
    import torch
    t = view.parent
    if t.dtype == torch.bool:
        return t.view(torch.uint8).cpu().numpy().view(np.bool_)
    return t.cpu().numpy()


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_case_on_the_gpu(name, option):
    case = TABLE[name]()
    for k, v in case.options.items():
        option(k, v)
    arrs = views(case, cuda)
    plan = S.make_plan(F[case.f], case.op, case.initop, case.dims, arrs)
    d = plan.describe()
    for s in case.expect:
        assert s in d + " ", (name, s, d)
    plan.execute(cur())
    import torch
    torch.cuda.synchronize()
    err = case.mismatch(host_parent(arrs[0]))
    assert err is None, f"{err} [{d}]"
    REACHED.setdefault(case.cell, d)


# ---- determinism -----------------------------------------------------------------------------------------------------
DET = [  # (dims, reduced dims, dtype, options, describe substrings)
    ((64 * 4096,), (0,), np.float32, {}, ("fold=in-launch",)),
    ((300 * 4096,), (0,), np.float64, {}, ("fold=second-launch",)),
    ((3 * 4096 + 1,), (0,), np.complex64, {}, ("vec=1 fold=in-launch",)),
    ((32768, 2), (0,), np.float32, {}, ("form=row", "fold=in-launch")),
    ((128, 256), (1,), np.float64, {}, ("form=col", "fold=in-launch")),
    ((64, 65536), (1,), np.float32, {"reduce_single": 1 << 20}, ("form=col", "fold=in-launch")),
    ((100, 2000), (1,), np.float32, {}, ("form=col", "fold=second-launch", "lanes=25x10")),
    ((65536, 2), (0,), np.float32, {"reduce_part_kind": 0}, ("form=general", "fold=in-launch")),
]


@pytest.mark.parametrize("dims,rdims,dt,opts,expect", DET, ids=[f"{d}-{np.dtype(t).name}" for d, _, t, _, _ in DET])
def test_reductions_are_run_to_run_identical(dims, rdims, dt, opts, expect, option):
    """no float atomics, so results are bitwise identical from run to run -- including the in-launch folds,
    where the workgroup that arrives last (and folds) varies.  Non-integer data: any change of order shows."""
    import torch
    for k, v in opts.items():
        option(k, v)
    rng = np.random.default_rng(7)
    n = int(np.prod(dims))
    a = rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(dt).kind == "c" else 0)
    A = S.StridedView(cuda(a.astype(dt)), dims, tuple(int(np.prod(dims[:i])) for i in range(len(dims))), 0)
    oshape = tuple(1 if i in rdims else m for i, m in enumerate(dims))
    out = S.StridedView(torch.zeros(int(np.prod(oshape)), dtype=A.parent.dtype, device="cuda"), oshape,
                        tuple(int(np.prod(oshape[:i])) for i in range(len(oshape))), 0)
    args = S.promoteshape(dims, out, A)
    plan = S.make_plan(lambda x: x, "+", "zero", dims, args)
    d = plan.describe()
    assert all(s in d for s in expect), d
    got = []
    for p in (plan, plan, S.make_plan(lambda x: x, "+", "zero", dims, args)):
        p.execute(cur())
        torch.cuda.synchronize()
        got.append(out.parent.cpu().numpy().copy())
    for g in got[1:]:
        assert np.array_equal(g.view(np.uint8), got[0].view(np.uint8)), d


# ---- accumulation precision ------------------------------------------------------------------------------------------
# k = the additions on the longest path from an element to the result, from the launch geometry the plan reports:
#   REDUCE_ALL, 2^22 elements, 1024 workgroups: 4 serial per accumulator (Float32: 1 row of 4-vectors; Float64: 2 rows of
#     2-vectors) + 2 (4 accumulators) + 6 (wave) + 2 (4 waves) + 4 serial per lane of the fold (1024 partials / 256 lanes)
#     + 6 + 2 + 1 (epilogue) = 27
#   ROW, 4 outputs x 2^20 Float32 (2^19 Float64), 256 lanes, 128 chunks: 8 (Float64: 4) serial per accumulator + 2 (U = 4)
#     + 6 (wave) + 3 (4 waves through LDS) + second pass, 32 lanes per output: 2 + 5 + 1 = 27 (Float64: 23)
#   COL, 32 outputs x 2^17 Float32 (2^16 Float64), 32 (16) rows per workgroup, 512 chunks: 8 serial per accumulator + 5 (4)
#     LDS levels + second pass, 64 lanes, 8 partials each into 4 accumulators: 2 + 2 + 6 + 1 = 24 (Float64: 23)
# The serial worst case n * u is 10^4 - 10^5 times larger.
PREC = [
    ((1 << 22,), (0,), np.float32, 27, "blocks=1024 vec=4 fold=second-launch"),
    ((1 << 22,), (0,), np.float64, 27, "blocks=1024 vec=2 fold=second-launch"),
    ((1 << 20, 4), (0,), np.float32, 27, "form=row lanes_per_out=256 split=128 vec=4"),
    ((1 << 19, 4), (0,), np.float64, 23, "form=row lanes_per_out=256 split=128 vec=2"),
    ((32, 1 << 17), (1,), np.float32, 24, "form=col lanes_per_out=32 split=512 vec=4"),
    ((32, 1 << 16), (1,), np.float64, 23, "form=col lanes_per_out=16 split=512 vec=2"),
]


@pytest.mark.parametrize("dims,rdims,dt,k,expect", PREC, ids=[f"{d}-{np.dtype(t).name}" for d, _, t, _, _ in PREC])
def test_accumulation_error_is_bounded_by_the_tree_depth(dims, rdims, dt, k, expect):
    import torch
    rng = np.random.default_rng(3)
    n = int(np.prod(dims))
    a = rng.random(n).astype(dt)
    A = S.StridedView(cuda(a), dims, tuple(int(np.prod(dims[:i])) for i in range(len(dims))), 0)
    oshape = tuple(1 if i in rdims else m for i, m in enumerate(dims))
    out = S.StridedView(torch.zeros(int(np.prod(oshape)), dtype=A.parent.dtype, device="cuda"), oshape,
                        tuple(int(np.prod(oshape[:i])) for i in range(len(oshape))), 0)
    plan = S.make_plan(lambda x: x, "+", "zero", dims, S.promoteshape(dims, out, A))
    d = plan.describe()
    assert expect in d, d
    plan.execute(cur())
    torch.cuda.synchronize()
    got = out.parent.cpu().numpy().astype(np.float64).reshape(oshape, order="F")
    u = float(np.finfo(dt).eps) / 2
    x = a.astype(np.float64).reshape(dims, order="F")
    kept = [i for i in range(len(dims)) if i not in rdims]
    xs = np.moveaxis(x, kept, list(range(len(kept)))).reshape(int(np.prod([dims[i] for i in kept])) if kept else 1, -1)
    for o, (row, g) in enumerate(zip(xs, got.reshape(-1, order="F"))):
        exact = math.fsum(row.tolist())  # positive data: the sum of magnitudes is the sum
        assert abs(g - exact) <= k * u * exact, (o, g, exact, abs(g - exact) / (u * exact), d)


def test_every_cell_was_reached():
    """runs after the table (file order): every cell of the coverage table was reached on the GPU, as describe() showed"""
    if not REACHED:
        pytest.skip("the table did not run in this session")
    missing = sorted(set(RC.CELLS) - set(REACHED))
    assert not missing, missing
    print("[reduce exact] cells: " + ", ".join(f"{c}" for c in sorted(REACHED)))
