"""GPU: contraction groups (csrc/smr_k_gcontract.hip) on the table of tests/group_contract_cases.py.

  1. every row: each member's WHOLE destination parent, byte for byte, against NumPy's result (Case.expected) and against the same
     member run alone under contract = 2 -- whatever tile either side picked; rows whose f is a program run runtime-compiled
     (asserted from the library's counters) and interpreted (jit = 0), with the same bytes;
  2. order: random Float32 / Float64 data against the sequential loop, bit for bit;
  3. dispatch: plain HIP, a library-owned stream, a recorded sequence replayed twice (beta = 1 members accumulate twice: compared
     with two single calls) and the same sequence cut into three block ranges -- the same bytes, and the replay is AQL packets;
  4. the front: `with S.group(contract=True):` around 37 mul_ calls fed by 37 permutedims_ is two launches."""
import functools
import itertools

import numpy as np
import pytest

import contract_cases as CC
import group_contract_cases as GC
import strided_jl_amd as S
from util import to_device

pytestmark = pytest.mark.gpu
ROWS = GC.table()


class jit_mode:
    """with jit_mode(jit): the "jit" option set and restored; under jit = 1 the block must have run a runtime-compiled kernel (a code
    object compiled or found in the cache, and no failure), under jit = 0 none (tests/test_gpu_contract.py: jit_mode)."""

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


def sync():
    import torch
    torch.cuda.synchronize()


def stream():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def upload(built):
    """Device copies of every member's operands: ([(C, A, B), ...], [cache per member])."""
    devs, caches = [], []
    for ops in built:
        cache = {}
        devs.append(tuple(to_device(a, cache) for a in ops))
        caches.append(cache)
    return devs, caches


def parents(built, caches):
    """Every member's destination parent, whole, as host arrays."""
    sync()
    return [cache[ops[0].parent.ctypes.data].cpu().numpy() for ops, cache in zip(built, caches)]


def run_group(row, built, how=lambda g: g.execute(stream())):
    devs, caches = upload(built)
    g = row.group(devs, stream=stream())
    how(g)
    out = parents(built, caches)
    g.close()
    return out


def run_singles(row, built, times=1):
    """Every member alone, `times` times, under contract = 2."""
    devs, caches = upload(built)
    with CC.option("contract", 2):
        for _ in range(times):
            for i, (c, dev) in enumerate(zip(row.members, devs)):
                c.call(dev, row.initop(i))
    return parents(built, caches)


def compare(row, got, want, what):
    for c, g, w in zip(row.members, got, want):
        msg = GC.mismatch(c, g, w, "%s | %s" % (row.name, what))
        assert msg is None, msg


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_member_is_exact_and_the_single_calls_bytes(row):
    built = row.build()
    want = row.expected(built)
    if not row.needs_prog:
        compare(row, run_group(row, built), want, "group vs NumPy")
        compare(row, run_singles(row, built), want, "single calls vs NumPy")
        return
    with jit_mode(1):   # a runtime-compiled kernel ran: the launchers fall back to the interpreter silently, with the same results
        compare(row, run_group(row, built), want, "group, runtime-compiled, vs NumPy")
        if row.fname == "and":   # `&` is a math opcode (include/strided_hip.h): runtime-compiled kernels only, jit = 0 refuses it
            compare(row, run_singles(row, built), want, "single calls, runtime-compiled, vs NumPy")
            return
    with jit_mode(0):
        compare(row, run_group(row, built), want, "group, interpreted, vs NumPy")
        compare(row, run_singles(row, built), want, "single calls, interpreted, vs NumPy")


# ---- accumulation order ---------------------------------------------------------------------------------------------------------------
def sequential(case, ops, beta, dt):
    """The loop the accumulation order defines, in dtype dt (the loop of tests/test_gpu_contract.py::sequential): acc = -0.0; over q
    ascending, over k ascending: acc = acc + a * b (a separate multiply and add); C = old * beta + acc.  The reduced dims in the
    planner's canonical order: describe() lists the canonical extents, kept dims first."""
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


@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("tn", ["f32", "f64"])
def test_accumulation_order_is_the_sequential_loop(tn, tile):
    """Random non-integer data (fixed seed), beta = 2 + i % 3 per member: every member bit for bit the sequential loop, on both tiles.
    A pairwise (tree) order over k differs from it in some member for this seed (asserted on the host first)."""
    dt = GC.TYPES[tn][0]
    row = GC.Row("order/%s/t%d" % (tn, tile), tn, GC.TYPES[tn], GC.specs_for(tn, 37)[:11] + GC.specs_for(tn, 2)[1:], "scale", tile)
    built = row.build()
    rng = np.random.default_rng(20261020)
    want, differs = [], False
    for i, (case, ops) in enumerate(zip(row.members, built)):
        for a in ops:
            u = np.unique(GC.W.element_index(a).ravel())
            a.parent[u] = rng.standard_normal(u.size).astype(dt)
        beta = row.initop(i)[1]
        view = sequential(case, ops, beta, dt)
        A, B = (x.toarray().astype(dt) for x in ops[1:])
        mapped = (np.broadcast_to(A, case.dims) * np.broadcast_to(B, case.dims)).astype(dt)
        flat = np.moveaxis(mapped, case.rdims, tuple(range(-len(case.rdims), 0))).reshape(view.size, -1)
        while flat.shape[1] > 1:  # halving tree
            h = (flat.shape[1] + 1) // 2
            lo, hi = flat[:, :h].copy(), flat[:, h:]
            lo[:, :hi.shape[1]] = lo[:, :hi.shape[1]] + hi
            flat = lo
        tree = (ops[0].toarray().astype(dt).ravel() * dt(beta) + flat[:, 0]).astype(dt)
        differs = differs or not np.array_equal(tree.view(np.uint8), view.ravel().view(np.uint8))
        w = ops[0].parent.copy()
        w[GC.W.element_index(ops[0]).ravel()] = view.ravel()
        want.append(w)
    assert differs, "the seed does not tell the orders apart"
    compare(row, run_group(row, built), want, "sequential order")


# ---- dispatch -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct_available():
    """Does a sequence of one plain plan replay as AQL packets in this process?  (No: the direct path is switched off or failed.)"""
    import torch
    a = S.StridedView(torch.zeros(64, dtype=torch.float64, device="cuda"), (8, 8), (1, 8), 0)
    q = S.Sequence().add(S.make_plan(lambda x: x, None, None, a.size, (a.similar(), a)))
    return CC.field(q.info(), "backend") == "aql"


def dispatch_row(kind):
    if kind == "native":
        return GC.row("f32/mul/n300/t32")       # initop none: beta = 1, every execution accumulates
    return GC.Row("f32/dist/n120/t16", "f32", GC.TYPES["f32"], GC.specs_for("f32", 300)[:119] + GC.specs_for("f32", 2)[1:], "none", 16, f="dist")


@pytest.mark.parametrize("kind", ["native", "runtime-compiled"])
def test_dispatch_paths_give_the_same_bytes(kind):
    row = dispatch_row(kind)
    assert row.kind == "none"
    built = row.build()
    once, twice = run_singles(row, built, 1), run_singles(row, built, 2)
    compare(row, once, row.expected(built), "single calls vs NumPy")
    compare(row, run_group(row, built), once, "plain HIP")

    def owned(g):
        with S.Stream() as st:
            g.execute(st.handle)
        st.close()

    compare(row, run_group(row, built, owned), once, "library-owned stream")
    infos = {}

    def sequence(slices):
        def run(g):
            lay = g.layout()
            grid = lay[-1][1] + lay[-1][2]
            if slices > 1:   # the cuts (csrc/smr_sched.cpp: slice_range): ceil(grid / slices) rounded up to a multiple of 8
                per = ((grid + slices - 1) // slices + 7) & ~7
                cuts = [per * k for k in range(1, slices) if per * k < grid]
                assert grid >= 64 * slices and len(cuts) == slices - 1 and any(x not in {r[1] for r in lay} for x in cuts), (grid, cuts)
            q = S.Sequence().add_group(g)
            q.set("slices", slices)
            q.run(2, stream())
            q.wait()
            sync()
            infos[slices] = q.info()
            del q
        return run

    compare(row, run_group(row, built, sequence(1)), twice, "sequence replayed twice")
    compare(row, run_group(row, built, sequence(3)), twice, "sequence replayed twice, three block ranges")
    for slices, info in infos.items():
        assert CC.field(info, "items") == "1" and CC.field(info, "groups") == "1", info
        if direct_available():
            assert CC.field(info, "backend") == "aql", info
            assert CC.field(info, "packets") == str(slices) and CC.field(info, "sliced") == ("1" if slices > 1 else "0"), info


# ---- the front ------------------------------------------------------------------------------------------------------------------------
def test_front_37_products_fed_by_37_permutedims_are_two_launches():
    import torch
    shapes = [(GC.MN[(3 * i + 1) % 8], GC.MN[(5 * i + 2) % 8], 3 + (7 * i) % 40) for i in range(37)]
    shapes = [(max(m, 3), max(n, 3), k) for m, n, k in shapes]

    def operands():
        out = []
        r = np.random.default_rng(11)
        for m, n, k in shapes:
            mk = lambda *s: S.StridedView(torch.from_numpy(r.integers(-3, 4, size=int(np.prod(s))).astype(np.float64)).cuda(), s,  # noqa: E731
                                          tuple(int(np.prod(s[:d])) for d in range(len(s))), 0)
            out.append((mk(m, n), mk(m, k), mk(k, n), mk(k, m)))
        return out

    def calls(ops):
        for Cm, A, B, X in ops:
            S.permutedims_(A, X, (1, 0))
        for i, (Cm, A, B, X) in enumerate(ops):
            S.mul_(Cm, A, B, 1, 2 + i % 5)

    plain, grouped = operands(), operands()
    with CC.option("contract", 2):
        calls(plain)
    sync()
    before = S.get_option("launches")
    with S.group(contract=True) as g:
        calls(grouped)
    sync()
    assert S.get_option("launches") == before + 2, [x.describe() for x in g.groups]
    assert g.singles == 0 and [x.count for x in g.groups] == [37, 37]
    assert "kind=contract" in g.groups[1].describe() and "f=mul2" in g.groups[1].describe()
    for (Cp, Ap, *_), (Cg, Ag, *_), shp in zip(plain, grouped, shapes):
        assert np.array_equal(Cp.toarray().view(np.uint8), Cg.toarray().view(np.uint8)), shp
        assert np.array_equal(Ap.toarray(), Ag.toarray()), shp
    # the default block still runs every product on its own
    before = S.get_option("launches")
    with S.group() as g:
        calls(grouped)
    sync()
    assert S.get_option("launches") >= before + 1 + 37 and [x.count for x in g.groups] == [37] and g.singles == 0
