"""GPU: the CONTRACT family (outer-product reductions, csrc/smr_k_contract.hip) on the table of tests/contract_cases.py.

Every case runs with contract = 2 (set and restored inside the test) on device copies of windowed operands; the destination's WHOLE
parent is compared byte for byte with NumPy's result written into a copy of it.
  1. exact: integer-valued data, every op, every initop form;
  2. order: random Float32 / Float64 data against the sequential loop the family's accumulation order defines, bit for bit
     (REDUCE_PART's COL form folds rows through an LDS tree: this test fails without the family);
  3. f kinds: pairwise distance interpreted and runtime-compiled, min-plus with planted NaN and +-Inf;
  4. dispatch: a library-owned stream, a recorded sequence replayed twice, plain HIP launches -- the same bytes;
  5. A/B: every case of 1 again with contract = 0 -- the same bytes."""
import itertools

import numpy as np
import pytest

import contract_cases as CC
import strided_jl_amd as S
from util import to_device

pytestmark = pytest.mark.gpu
ROWS = {c.name: c for c in CC.exact_rows()}
INITOPS = {"zero": "zero", "none": None, "scale": ("scale", 2), "const": ("const", 3), "conj": "conj", "identity": "identity"}


class jit_mode:
    """with jit_mode(jit): the "jit" option set and restored; under jit = 1 the block must have run a runtime-compiled kernel (a code
    object compiled or found in the cache, and no failure): the launchers fall back to the interpreter silently, and its results are
    the same."""

    def __init__(self, jit):
        self.jit, self.opt = jit, CC.option("jit", jit)

    def __enter__(self):
        self.opt.__enter__()
        self.before = [S.get_option(k) for k in ("jit_compiles", "jit_hits", "jit_failures")]

    def __exit__(self, et, ev, tb):
        self.opt.__exit__(et, ev, tb)
        if et is None:
            c, h, f = [S.get_option(k) for k in ("jit_compiles", "jit_hits", "jit_failures")]
            assert f == self.before[2], "runtime compilation failed"
            if self.jit:
                assert c + h > self.before[0] + self.before[1], "no runtime-compiled kernel ran"
            else:
                assert c + h == self.before[0] + self.before[1], "jit = 0 compiled a kernel"


def device_run(case, ops, run, contract=2, check_family=True):
    """Runs `run(device operands)` on fresh device copies; returns the destination's whole parent as a host array."""
    import torch
    cache = {}
    dev = tuple(to_device(a, cache) for a in ops)
    with CC.option("contract", contract):
        if check_family:
            p = case.plan(dev)
            d = p.describe()
            p.close()
            assert CC.family(d) == (CC.CONTRACT if contract else "reduce_part"), d
        run(dev)
    torch.cuda.synchronize()
    return cache[ops[0].parent.ctypes.data].cpu().numpy()


def initops_for(case, i):
    """zero for every row, and two of the other five forms in turn, so that every form meets every type."""
    if case.dts[0] == CC.BOOL:
        return ["none", "zero"]
    others = ["none", "scale", "const", "conj", "identity"]
    return ["zero", others[i % 5], others[(i + 2) % 5]]


@pytest.mark.parametrize("name", sorted(ROWS))
def test_exact_and_same_bytes_without_the_family(name):
    """Tests 1 and 5: byte for byte against NumPy under contract = 2, and the same under contract = 0."""
    case = ROWS[name]
    i = sorted(ROWS).index(name)
    for key in initops_for(case, i):
        initop = INITOPS[key]
        ops = case.build()
        want = case.expected(ops, initop)
        for contract in (2, 0):
            got = device_run(case, ops, lambda dev: case.call(dev, initop), contract)
            msg = CC.mismatch(case, got, want, "initop=%s contract=%d" % (key, contract))
            assert msg is None, msg


@pytest.mark.parametrize("tn", ["f32", "f64", "c64", "i64"])
def test_mul_front_alpha_beta(tn):
    """S.mul_(C, A, B, alpha, beta) with beta in {0, 1, 2}: initop zero / nothing / scale through the front end."""
    import torch
    dts = CC.TYPES[tn]
    case = CC.Case("mul_/%s" % tn, (37, 35, 19), CC.MM, dts, CC.CONTRACT, layouts=("col", "col", "trans"))
    for beta, initop in ((0, "zero"), (1, None), (2, ("scale", 2))):
        ops = case.build()
        want = case.expected(ops, initop)
        cache = {}
        C3, A3, B3 = (to_device(a, cache) for a in ops)
        m, n, k = case.dims
        C = S.StridedView(C3.parent, (m, n), C3.strides[:2], C3.offset, C3.op)
        A = S.StridedView(A3.parent, (m, k), (A3.strides[0], A3.strides[2]), A3.offset, A3.op)
        B = S.StridedView(B3.parent, (k, n), (B3.strides[2], B3.strides[1]), B3.offset, B3.op)
        with CC.option("contract", 2):
            S.mul_(C, A, B, 1, beta)
        torch.cuda.synchronize()
        msg = CC.mismatch(case, cache[ops[0].parent.ctypes.data].cpu().numpy(), want, "beta=%d" % beta)
        assert msg is None, msg


def sequential(case, ops, beta, dt):
    """The loop the accumulation order defines, in dtype dt: acc = -0.0; over q ascending, over k ascending: acc = acc + a * b (a
    separate multiply and add); C = old * beta + acc.  The reduced dims in the planner's canonical order: the plan's describe() lists
    the canonical extents, kept dims first, so the inner reduced dim is the first reduced extent listed."""
    A, B = (x.toarray().astype(dt) for x in ops[1:])
    rd = case.rdims
    with CC.option("contract", 2):
        p = case.plan(ops)
        d = p.describe()
        p.close()
    cdims = [int(x) for x in CC.field(d, "dims").split("x")]
    red_ext = cdims[len(cdims) - len(rd):] if len(rd) > 1 else [case.dims[rd[0]]]
    order = list(rd)
    if len(rd) > 1 and [case.dims[r] for r in rd] != red_ext:
        order = list(reversed(rd))
    assert [case.dims[r] for r in order] == red_ext, (d, order)
    kshape = tuple(1 if r in rd else n for r, n in enumerate(case.dims))
    Af, Bf = np.broadcast_to(A, case.dims), np.broadcast_to(B, case.dims)
    acc = np.full(kshape, -0.0, dtype=dt)
    walk = list(reversed(order))  # itertools.product runs its LAST range fastest: the inner reduced dim
    for idx in itertools.product(*[range(case.dims[r]) for r in walk]):
        sel = [slice(None)] * len(case.dims)
        for r, v in zip(walk, idx):
            sel[r] = slice(v, v + 1)
        acc = acc + (Af[tuple(sel)] * Bf[tuple(sel)]).astype(dt)
    old = ops[0].toarray().astype(dt)
    return (old * dt(beta) + acc).astype(dt)


@pytest.mark.parametrize("tn", ["f32", "f64"])
@pytest.mark.parametrize("shape", ["ragged", "two_reduced", "k_2tk+1", "t32_k_2tk+1", "t64_k_2tk+1"])
def test_accumulation_order_is_the_sequential_loop(tn, shape):
    """Test 2.  Random non-integer data (fixed seed): bit for bit the sequential loop.  A pairwise (tree) order over k differs from it in
    at least one element for this seed, which the test asserts on the host first, so it cannot pass by coincidence."""
    dt = CC.TYPES[tn][0]
    ti, tj, tk = CC.tile_numbers(tn)
    if shape == "ragged":
        case = CC.Case("order/%s/ragged" % tn, (65, 63, 17), CC.MM, CC.TYPES[tn], CC.CONTRACT)
    elif shape == "two_reduced":
        case = CC.Case("order/%s/two" % tn, (33, 34, 5, 3), ((0, 1), (0, 2, 3), (1, 2, 3)), CC.TYPES[tn], CC.CONTRACT)
    elif shape == "k_2tk+1":
        case = CC.Case("order/%s/2tk+1" % tn, (ti + 3, tj + 5, 2 * tk + 1), CC.MM, CC.TYPES[tn], CC.CONTRACT, layouts=("col", "trans", "col"))
    else:  # more than two chunks through the 32 x 32 / 64 x 64 tile (a batch dim gives the workgroups those tiles ask for)
        tile = int(shape[1:3])
        case = CC.Case("order/%s/%s" % (tn, shape), CC.TILE_SHAPES[tile][0] + (2 * CC.tile_numbers(tn, tile)[2] + 1,), CC.BATCH, CC.TYPES[tn],
                       CC.CONTRACT, layouts=("col", "trans", "col"))
    ops = case.build()
    rng = np.random.default_rng(20261019)
    for a in ops:
        idx = CC.W.element_index(a).ravel()
        a.parent[np.unique(idx)] = rng.standard_normal(np.unique(idx).size).astype(dt)
    beta = 2
    want_view = sequential(case, ops, beta, dt)
    # a pairwise order over the mapped values differs somewhere (host check, no device)
    A, B = (x.toarray().astype(dt) for x in ops[1:])
    mapped = (np.broadcast_to(A, case.dims) * np.broadcast_to(B, case.dims)).astype(dt)
    flat = np.moveaxis(mapped, case.rdims, tuple(range(-len(case.rdims), 0))).reshape(want_view.size, -1)
    while flat.shape[1] > 1:  # halving tree
        h = (flat.shape[1] + 1) // 2
        lo, hi = flat[:, :h].copy(), flat[:, h:]
        lo[:, :hi.shape[1]] = lo[:, :hi.shape[1]] + hi
        flat = lo
    tree = (ops[0].toarray().astype(dt).ravel() * dt(beta) + flat[:, 0]).astype(dt)
    assert not np.array_equal(tree.view(np.uint8), want_view.ravel().view(np.uint8)), "the seed does not tell the orders apart"
    want = ops[0].parent.copy()
    want[CC.W.element_index(ops[0]).ravel()] = want_view.ravel()
    with CC.option("contract", 2):
        p = case.plan(ops)
        assert shape[:2] not in ("t3", "t6") or CC.tile_of(p.describe())[1] == int(shape[1:3]), p.describe()
        p.close()
    got = device_run(case, ops, lambda dev: case.call(dev, ("scale", beta)))
    msg = CC.mismatch(case, got, want, "sequential order")
    assert msg is None, msg


@pytest.mark.parametrize("jit", [0, 1])
def test_pairwise_distance_interpreted_and_compiled(jit):
    """Test 3: f = abs2(a - b), op = +, on integer-valued data: the interpreter (jit = 0) and the runtime-compiled kernel."""
    for tn in ("f32", "c64", "i64"):
        case = CC.Case("dist/%s/jit%d" % (tn, jit), (37, 35, 19), CC.MM, CC.TYPES[tn], CC.CONTRACT, f="dist", layouts=("col", "trans", "col"))
        ops = case.build()
        want = case.expected(ops, None)
        with jit_mode(jit):
            got = device_run(case, ops, lambda dev: case.call(dev, None))
        msg = CC.mismatch(case, got, want, "jit=%d" % jit)
        assert msg is None, msg


@pytest.mark.parametrize("jit", [0, 1])
def test_min_plus_with_nan_and_inf(jit):
    """Test 3: f = a + b, op = min with planted NaN, +Inf and -Inf: NaN wins where it meets an output, -Inf otherwise."""
    case = CC.Case("minplus/jit%d" % jit, (37, 35, 19), CC.MM, CC.TYPES["f64"], CC.CONTRACT, f="plus", op="min")
    ops = case.build()
    A, B = ops[1], ops[2]
    ia, ib = CC.W.element_index(A), CC.W.element_index(B)
    A.parent[ia[3, 0, 7]] = np.nan      # row 3 of the result is NaN
    A.parent[ia[5, 0, 2]] = -np.inf     # row 5 is -Inf ...
    B.parent[ib[0, 9, 2]] = np.inf      # ... except (5, 9): -Inf + Inf = NaN
    B.parent[ib[0, 11, 4]] = np.inf     # a +Inf never wins
    a, b = A.toarray(), B.toarray()
    with np.errstate(all="ignore"):
        part = np.fmin.reduce(a + b, axis=2, keepdims=True)
        part[np.isnan(a + b).any(axis=2, keepdims=True)] = np.nan   # Julia's min: NaN if any argument is NaN
    old = ops[0].toarray()
    w = np.where(np.isnan(part), np.nan, np.minimum(old, part))
    want = ops[0].parent.copy()
    want[CC.W.element_index(ops[0]).ravel()] = w.ravel()
    with jit_mode(jit):
        got = device_run(case, ops, lambda dev: case.call(dev, None))
    # NaN payloads are not defined: compare NaN positions, then the bytes of everything else
    gv, wv = got.copy(), want.copy()
    nanpos = np.isnan(wv)
    assert np.array_equal(np.isnan(gv), nanpos), "NaN positions differ"
    gv[nanpos] = 0
    wv[nanpos] = 0
    msg = CC.mismatch(case, gv, wv, "jit=%d" % jit)
    assert msg is None, msg
    assert np.isnan(w[3]).all() and np.isnan(w[5, 9, 0]) and np.isneginf(w[5, 0, 0])


@pytest.mark.parametrize("tn", sorted(CC.TYPES))
def test_dispatch_paths_give_the_same_bytes(tn):
    """Test 4: plain HIP launches, a library-owned stream (eager direct dispatch) and a recorded sequence replayed twice."""
    import torch
    case = ROWS["%s/tile_ragged" % tn]
    initop = "zero"  # (replaying twice must be idempotent)
    ops = case.build()
    want = case.expected(ops, initop)
    results = {}

    def hip(dev):
        p = case.plan(dev, initop)
        p.execute(int(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        p.close()

    def owned(dev):
        p = case.plan(dev, initop)
        with S.Stream() as st:
            p.execute(st.handle)
        torch.cuda.synchronize()
        st.close()
        p.close()

    def sequence(dev):
        p = case.plan(dev, initop)
        assert "split=" not in p.describe() and "fold=" not in p.describe()  # no partials, no scratch: one launch
        q = S.Sequence().add(p)
        q.set("slices", 1)
        q.run(2, int(torch.cuda.current_stream().cuda_stream))
        q.wait()
        torch.cuda.synchronize()
        print("[contract] %s sequence: %s" % (case.name, q.info().split(" last_replay")[0]))
        del q
        p.close()

    for name, run in (("hip", hip), ("owned stream", owned), ("sequence", sequence)):
        results[name] = device_run(case, ops, run)
        msg = CC.mismatch(case, results[name], want, name)
        assert msg is None, msg
