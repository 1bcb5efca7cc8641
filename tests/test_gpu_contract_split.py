"""GPU: the split form of the CONTRACT family (csrc/smr_k_contract.hip: k_contract_split, k_contract_fold) on the table of
tests/contract_split_cases.py: every row planned under contract = 2 with a forced tile and forced slices.

  1. exact: integer-valued data, byte for byte on the destination's whole parent, initop zero and two of the other five forms;
  2. order: random Float32 / Float64 data against the host loop the split form's accumulation order defines ("sliced sequential"),
     bit for bit -- after asserting on the host that this loop differs from the plain sequential loop and from a halving tree;
  3. the same plan again: three executions on one stream, a fourth on another (the partials are reused, the executions chained);
  4. dispatch: plain HIP launches, a library-owned stream, a recorded sequence replayed twice -- two launches per replay;
  5. by the rule through the front: S.mul_ at (64, 64, 4096) under contract = 1, contract_split = 1."""
import numpy as np
import pytest

import contract_cases as CC
import contract_split_cases as SC
import strided_jl_amd as S
from util import to_device

pytestmark = pytest.mark.gpu
ROWS = SC.by_name()
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


def needs_prog(case):
    """Rows whose f is not the natively compiled product of same-typed operands: runtime-compiled under jit = 1."""
    return case.fname != "mul" or len(set(np.dtype(t) for t in case.dts)) > 1 or case.dts[0] == CC.BOOL


def device_run(case, ops, run, want_kparts=None):
    """Runs `run(device operands)` under the row's options on fresh device copies; returns the destination's whole parent as a host
    array.  The plan must be a split CONTRACT plan on the row's tile."""
    import torch
    cache = {}
    dev = tuple(to_device(a, cache) for a in ops)
    with case.options():
        p = case.plan(dev)
        d = p.describe()
        p.close()
        assert CC.family(d) == CC.CONTRACT and CC.tile_of(d)[1] == case.tile and SC.slices(d)[0] >= 2, d
        assert want_kparts is None or SC.slices(d)[0] == want_kparts, d
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
def test_exact(name):
    """Test 1: byte for byte against NumPy, under jit = 1; the rows with another f under jit = 0 as well (the interpreter)."""
    case = ROWS[name]
    i = sorted(ROWS).index(name)
    ops = case.build()
    prog = needs_prog(case)
    jits = [1, 0] if case.fname == "dist" else [1]
    for key in initops_for(case, i):
        initop = INITOPS[key]
        want = case.expected(ops, initop)
        for jit in jits:
            with (jit_mode(jit) if prog else CC.option("jit", jit)):
                got = device_run(case, ops, lambda dev: case.call(dev, initop))
            msg = CC.mismatch(case, got, want, "initop=%s jit=%d" % (key, jit))
            assert msg is None, msg


@pytest.mark.parametrize("jit", [0, 1])
def test_min_plus_with_nan_and_inf_in_the_last_slice(jit):
    """f = a + b, op = min with planted NaN, +Inf and -Inf, all in rows of k that belong to the LAST slice: a fold that drops a slice
    shows.  NaN wins where it meets an output, -Inf otherwise."""
    tk = CC.tile_numbers("f64", 16)[2]
    K = 2 * tk + 3  # 3 chunks, S = 3: the last slice is rows 2 tk .. 2 tk + 2
    case = SC.SplitCase("minplus/jit%d" % jit, (37, 35, K), CC.MM, CC.TYPES["f64"], 16, 3, f="plus", op="min")
    ops = case.build()
    A, B = ops[1], ops[2]
    ia, ib = CC.W.element_index(A), CC.W.element_index(B)
    A.parent[ia[3, 0, 2 * tk + 1]] = np.nan      # row 3 of the result is NaN
    A.parent[ia[5, 0, 2 * tk]] = -np.inf         # row 5 is -Inf ...
    B.parent[ib[0, 9, 2 * tk]] = np.inf          # ... except (5, 9): -Inf + Inf = NaN
    B.parent[ib[0, 11, 2 * tk + 2]] = np.inf     # a +Inf never wins
    a, b = A.toarray(), B.toarray()
    with np.errstate(all="ignore"):
        part = np.fmin.reduce(a + b, axis=2, keepdims=True)
        part[np.isnan(a + b).any(axis=2, keepdims=True)] = np.nan   # Julia's min: NaN if any argument is NaN
    old = ops[0].toarray()
    w = np.where(np.isnan(part), np.nan, np.minimum(old, part))
    want = ops[0].parent.copy()
    want[CC.W.element_index(ops[0]).ravel()] = w.ravel()
    with jit_mode(jit):
        got = device_run(case, ops, lambda dev: case.call(dev, None), want_kparts=3)
    gv, wv = got.copy(), want.copy()
    nanpos = np.isnan(wv)
    assert np.array_equal(np.isnan(gv), nanpos), "NaN positions differ"
    gv[nanpos] = 0
    wv[nanpos] = 0
    msg = CC.mismatch(case, gv, wv, "jit=%d" % jit)
    assert msg is None, msg
    assert np.isnan(w[3]).all() and np.isnan(w[5, 9, 0]) and np.isneginf(w[5, 0, 0])


def test_a_sum_of_negative_zeros_is_negative_zero():
    """Float64, every product -0.0, the old destination -0.0, initop None, S = 3: -0.0 bit for bit (the partials are seeded with the
    neutral element -0.0 and the fold starts from P_0, not from +0.0)."""
    tk = CC.tile_numbers("f64", 16)[2]
    case = SC.SplitCase("negzero", (33, 31, 2 * tk + 1), CC.MM, CC.TYPES["f64"], 16, 3)
    ops = case.build()
    for k, v in ((0, -0.0), (1, -0.0), (2, 1.0)):
        ops[k].parent[np.unique(CC.W.element_index(ops[k]).ravel())] = v
    want = ops[0].parent.copy()
    got = device_run(case, ops, lambda dev: case.call(dev, None), want_kparts=3)
    view = got[CC.W.element_index(ops[0]).ravel()]
    assert np.all(view == 0) and np.all(np.signbit(view)), "a +0.0 came out of a sum of -0.0"
    msg = CC.mismatch(case, got, want, "signed zero")
    assert msg is None, msg


# ---- 2. order ------------------------------------------------------------------------------------------------------------------------
def _reduced_order(case, ops):
    """The reduced box dims in the planner's canonical order (inner first), and (tk, kparts, cps) of the row's plan."""
    d = case.describe(ops)
    cdims = [int(x) for x in CC.field(d, "dims").split("x")]
    rd = list(case.rdims)
    red_ext = cdims[len(cdims) - len(rd):]
    if [case.dims[r] for r in rd] != red_ext:
        rd = list(reversed(rd))
    assert [case.dims[r] for r in rd] == red_ext, (d, rd)
    kparts, cps, _ = SC.slices(d)
    return rd, CC.tile_of(d)[4], kparts, cps


def _chunks(case, rd, tk):
    """The chunk walk: a list of chunks, each the list of index tuples over the reduced dims `rd` (inner first) it holds, in order."""
    K = case.dims[rd[0]]
    outer = [case.dims[r] for r in rd[1:]]
    Q = int(np.prod(outer, dtype=np.int64)) if outer else 1
    nkc = -(-K // tk)
    out = []
    for t in range(Q * nkc):
        q, kc = divmod(t, nkc)
        qi = []
        for n in outer:  # dim NK + 1 fastest
            qi.append(q % n)
            q //= n
        out.append([(k,) + tuple(qi) for k in range(kc * tk, min((kc + 1) * tk, K))])
    return out


def _accumulate(case, Af, Bf, rd, steps, dt):
    kshape = tuple(1 if r in case.rdims else n for r, n in enumerate(case.dims))
    acc = np.full(kshape, -0.0, dtype=dt)
    for idx in steps:
        sel = [slice(None)] * len(case.dims)
        for r, v in zip(rd, idx):
            sel[r] = slice(v, v + 1)
        acc = acc + (Af[tuple(sel)] * Bf[tuple(sel)]).astype(dt)
    return acc


@pytest.mark.parametrize("tn", ["f32", "f64"])
@pytest.mark.parametrize("tile", SC.TILES)
@pytest.mark.parametrize("shape", ["3tk+1_s2", "two_s3"])
def test_accumulation_order_is_the_sliced_sequential_loop(tn, tile, shape):
    """Test 2.  dest = old * beta + (((P_0 + P_1) + P_2) ...), P_s the sequential sum, from -0.0, over the chunks of slice s."""
    dt = CC.TYPES[tn][0]
    base = ROWS["%s/t%d/%s" % (tn, tile, shape)]
    case = SC.SplitCase("order/" + base.name, base.dims, base.axes, base.dts, tile, base.S, layouts=("col", "trans", "col"))
    ops = case.build()
    rng = np.random.default_rng(20261020)
    for a in ops:
        idx = np.unique(CC.W.element_index(a).ravel())
        a.parent[idx] = rng.standard_normal(idx.size).astype(dt)
    beta = 2
    rd, tk, kparts, cps = _reduced_order(case, ops)
    assert kparts == case.S, (kparts, case.S)
    A, B = (x.toarray().astype(dt) for x in ops[1:])
    Af, Bf = np.broadcast_to(A, case.dims), np.broadcast_to(B, case.dims)
    chunks = _chunks(case, rd, tk)
    parts = [_accumulate(case, Af, Bf, rd, [i for ch in chunks[s * cps:(s + 1) * cps] for i in ch], dt) for s in range(kparts)]
    assert all(len(chunks[s * cps:(s + 1) * cps]) > 0 for s in range(kparts))
    total = parts[0]
    for p in parts[1:]:
        total = (total + p).astype(dt)
    old = ops[0].toarray().astype(dt)
    want_view = (old * dt(beta) + total).astype(dt)
    # the two orders this must not be mistaken for (host checks, no device)
    plain = (old * dt(beta) + _accumulate(case, Af, Bf, rd, [i for ch in chunks for i in ch], dt)).astype(dt)
    assert not np.array_equal(plain.view(np.uint8), want_view.view(np.uint8)), "the seed does not tell the sliced loop from the plain one"
    mapped = (Af * Bf).astype(dt)
    flat = np.moveaxis(mapped, case.rdims, tuple(range(-len(case.rdims), 0))).reshape(want_view.size, -1)
    while flat.shape[1] > 1:  # halving tree
        h = (flat.shape[1] + 1) // 2
        lo, hi = flat[:, :h].copy(), flat[:, h:]
        lo[:, :hi.shape[1]] = lo[:, :hi.shape[1]] + hi
        flat = lo
    tree = (old.ravel() * dt(beta) + flat[:, 0]).astype(dt)
    assert not np.array_equal(tree.view(np.uint8), want_view.ravel().view(np.uint8)), "the seed does not tell the sliced loop from a tree"
    want = ops[0].parent.copy()
    want[CC.W.element_index(ops[0]).ravel()] = want_view.ravel()
    got = device_run(case, ops, lambda dev: case.call(dev, ("scale", beta)), want_kparts=kparts)
    msg = CC.mismatch(case, got, want, "sliced sequential order")
    assert msg is None, msg


# ---- 3. the same plan again ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f64/t16/5tk_s3", "f32/t32/3tk+1_s2", "i64/t64/two_s3"])
def test_one_plan_executed_again_and_on_a_second_stream(name):
    import torch
    case = ROWS[name]
    ops = case.build()
    once = case.expected(ops, "zero")
    idx = CC.W.element_index(ops[0]).ravel()
    want = ops[0].parent.copy()
    want[idx] = ops[0].parent[idx] + 4 * once[idx]

    def run(dev):
        p = case.plan(dev, None)
        assert SC.slices(p.describe())[0] >= 2
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for _ in range(3):
            p.execute(int(s1.cuda_stream))
        p.execute(int(s2.cuda_stream))  # (chained behind the executions on s1 by the library: one set of partials)
        s2.synchronize()
        s1.synchronize()
        p.close()

    got = device_run(case, ops, run)
    msg = CC.mismatch(case, got, want, "old + 4 sums")
    assert msg is None, msg


# ---- 4. dispatch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tn", sorted(CC.TYPES))
def test_dispatch_paths_give_the_same_bytes(tn):
    import torch
    case = ROWS["%s/t32/3tk+1_s2" % tn]
    initop = "zero"  # (replaying twice must be idempotent)
    ops = case.build()
    want = case.expected(ops, initop)

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
        assert "split=" not in p.describe() and CC.field(p.describe(), "fold") == "second-launch"
        q = S.Sequence().add(p)
        q.set("slices", 1)
        before = S.get_option("launches")
        q.run(2, int(torch.cuda.current_stream().cuda_stream))
        q.wait()
        torch.cuda.synchronize()
        info = q.info().split(" last_replay")[0]
        print("[contract_split] %s sequence: %s" % (case.name, info))
        if "backend=aql" in info:
            assert " items=1 " in info and " packets=2 " in info, info  # the main launch and the fold
        else:
            assert S.get_option("launches") - before == 4, info
        del q
        p.close()

    for name, run in (("hip", hip), ("owned stream", owned), ("sequence", sequence)):
        with CC.option("jit", 1):
            got = device_run(case, ops, run, want_kparts=2)
        msg = CC.mismatch(case, got, want, name)
        assert msg is None, msg


# ---- 5. by the rule, through the front -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tn", ["f32", "f64"])
def test_mul_front_by_the_rule(tn):
    import torch
    dts = CC.TYPES[tn]
    case = CC.Case("mul_/%s" % tn, (64, 64, 4096), CC.MM, dts, CC.CONTRACT, layouts=("col", "col", "trans"))
    assert S.get_option("contract") == 1
    ops = case.build()
    # (64 x 64 outputs of 4096 products of integers of [-3, 3]: every partial sum is exact in Float32)
    for beta, initop in ((0, "zero"), (1, None), (2, ("scale", 2))):
        want = case.expected(ops, initop)
        cache = {}
        C3, A3, B3 = (to_device(a, cache) for a in ops)
        m, n, k = case.dims
        C = S.StridedView(C3.parent, (m, n), C3.strides[:2], C3.offset, C3.op)
        A = S.StridedView(A3.parent, (m, k), (A3.strides[0], A3.strides[2]), A3.offset, A3.op)
        B = S.StridedView(B3.parent, (k, n), (B3.strides[2], B3.strides[1]), B3.offset, B3.op)
        with CC.option("contract_split", 1):
            p = case.plan((C3, A3, B3), initop)
            d = p.describe()
            p.close()
            assert CC.family(d) == CC.CONTRACT and SC.slices(d)[0] >= 2, d
            S.mul_(C, A, B, 1, beta)
        torch.cuda.synchronize()
        msg = CC.mismatch(case, cache[ops[0].parent.ctypes.data].cpu().numpy(), want, "beta=%d %s" % (beta, d))
        assert msg is None, msg
