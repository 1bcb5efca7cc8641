"""GPU: reduction groups (SMR_GROUP_REDUCE, csrc/smr_k_greduce.hip) on the table of tests/group_reduce_cases.py.

  1. every row: the WHOLE destination parent (the K-vector and the random bits around its elements), byte for byte, against the exact
     expected values and against the members run one by one under "reduce_blocks" = 64; rows whose f is a program run
     runtime-compiled (asserted from the library's counters) and interpreted, with the same bytes;
  2. order: random Float32 / Float64 / ComplexF64 data -- order-dependent sums -- over members of W = 1, 2, 3 and 64 workgroups on both
     bodies: bit-identical to the single calls under "reduce_blocks" = 64;
  3. repeated execution: one group executed three times onto one destination (initop none accumulates, scale applies three times) on
     the plain HIP stream and on a library-owned stream -- the arrival counters come back to zero;
  4. recorded sequences: replayed twice under 1 and 4 queues and under "slices" = 3 (the launch stays whole), as AQL packets; a map
     group that writes the blocks followed by the reduction group that reads them;
  5. the front: `with S.group(reduce=True, independent=True):` around 37 mapreducedim_ calls into a 37-vector is one launch."""
import functools

import numpy as np
import pytest

import contract_cases as CC
import group_reduce_cases as GR
import strided_jl_amd as S
from reduce_exact_cases import _index
from strided_jl_amd import _lib as L
from test_gpu_group_contract import jit_mode

pytestmark = pytest.mark.gpu
ROWS = GR.table()


def sync():
    import torch
    torch.cuda.synchronize()


def cur():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def cuda(a):
    import torch
    if a.dtype == np.bool_:
        return torch.from_numpy(a.view(np.uint8).copy()).cuda().view(torch.bool)
    return torch.from_numpy(a.copy()).cuda()


def download(t):
    import torch
    sync()
    if t.dtype == torch.bool:
        return t.view(torch.uint8).cpu().numpy().view(np.bool_)
    return t.cpu().numpy()


def run_group(row, how=None, independent=False):
    """The destination parent after `how(group)` (default: one execution on the current stream) on fresh device copies."""
    dpar, views = row.views(cuda)
    g = row.group(views, independent=independent, stream=cur())
    (how or (lambda grp: grp.execute(cur())))(g)
    out = download(dpar)
    g.close()
    return out


def run_singles(row, times=1):
    """Every member alone, `times` rounds, under "reduce_blocks" = 64; also the plans' describe() lines."""
    dpar, views = row.views(cuda)
    members, _ = row.build()
    descs = []
    with CC.option("reduce_blocks", 64):
        plans = [S.make_plan(row.fn(), row.op, m.initop, m.dims, v) for m, v in zip(members, views)]
        for _ in range(times):
            for p in plans:
                p.execute(cur())
        out = download(dpar)
        for p in plans:
            descs.append(p.describe())
            p.close()
    return out, descs


def check(row, got, want, what):
    err = GR.mismatch(row, got, want, what)
    assert err is None, err


# ---- 1. every row ----------------------------------------------------------------------------------------------------------------------
def exact_and_single(row, what):
    want = row.expected_parent(1)
    check(row, run_group(row), want, "group vs exact" + what)
    singles, _ = run_singles(row)
    check(row, singles, want, "single calls vs exact" + what)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_member_is_exact_and_the_single_calls_bytes(row):
    if row.f not in ("prog", "amc"):
        exact_and_single(row, "")
        return
    with jit_mode(1):   # a runtime-compiled kernel ran: the launchers fall back to the interpreter silently, with the same results
        exact_and_single(row, ", runtime-compiled")
    with jit_mode(0):
        exact_and_single(row, ", interpreted")


# ---- 2. accumulation order -------------------------------------------------------------------------------------------------------------
def order_row(t):
    V = GR.RF.VMAX[t]
    f, nin, conjs = {"f32": ("abs2", 1, None), "f64": ("ident", 1, None), "c64": ("mul", 2, (True, False))}[t]
    lin = functools.partial(GR.lin, nin=nin)
    specs = [lin(1000, lo=1), lin(8192, vec=V > 1), lin(4097, step=2), lin(8193), lin(12288, lo=2 * V, vec=V > 1), lin(262144, vec=V > 1), lin(262145),
             lin(262144, lo=1), lin(70000, step=3), lin(5000, lo=3)]
    return GR.Row("order/%s" % t, t, "+", f, "scale", specs, conjs=conjs)


@pytest.mark.parametrize("t", ["f32", "f64", "c64"])
def test_random_sums_are_bit_identical_to_the_single_calls_under_64_blocks(t):
    """Non-integer random data: the sums depend on the order.  Every member must give the single call's bits under "reduce_blocks" = 64
    (every member is of rank 1: the single call runs family REDUCE_ALL, asserted), and the data tell orders apart: under "reduce_blocks"
    = 1 -- one workgroup walks everything -- some member's bits differ (asserted, so that equal bytes above mean an equal order)."""
    row = order_row(t)
    members, _ = row.build()
    rng = np.random.default_rng(20261021)
    for m in members:   # (a private row: its parents are this test's to fill)
        for o in m.ins:
            e = tuple(1 if s == 0 else n for n, s in zip(m.dims, o.strides))
            idx = _index(o.offset, e, o.strides).ravel()
            v = rng.standard_normal(idx.size) + (1j * rng.standard_normal(idx.size) if t == "c64" else 0)
            o.parent[idx] = v.astype(o.parent.dtype)
    assert {sp.W for sp in row.specs} >= {1, 2, 3, 64}
    got = run_group(row)
    singles, descs = run_singles(row)
    assert all(CC.family(d) == "reduce_all" for d in descs), descs
    assert {CC.field(d, "vec") for d in descs} == ({"1"} if t == "c64" else {"1", str(GR.RF.VMAX[t])}), descs
    check(row, got, singles, "group vs single calls, random data")
    with CC.option("reduce_blocks", 1):
        dpar, views = row.views(cuda)
        plans = [S.make_plan(row.fn(), row.op, m.initop, m.dims, v) for m, v in zip(members, views)]
        for p in plans:
            p.execute(cur())
        one = download(dpar)
        for p in plans:
            p.close()
    assert GR.mismatch(row, one, singles, "") is not None, "the data do not tell accumulation orders apart"


# ---- 3. repeated execution -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["hip-stream", "library-stream"])
@pytest.mark.parametrize("name", ["edges/cap/f64", "edges/block/f32", "types/c32", "ops/prod/f64"])
def test_three_executions_onto_one_destination(name, where):
    """initop none accumulates three times, scale applies three times: three rounds of single calls, and the exact value.  A counter
    left nonzero by the first execution would end the second one's fold early or never."""
    row = GR.row(name)
    assert row.kind in ("none", "scale") and any(sp.W > 1 for sp in row.specs)

    def thrice(g):
        if where == "hip-stream":
            for _ in range(3):
                g.execute(cur())
            return
        with S.Stream() as st:
            for _ in range(3):
                g.execute(st.handle)
        st.close()

    got = run_group(row, thrice)
    check(row, got, row.expected_parent(3), "three executions vs exact, " + where)
    singles, _ = run_singles(row, 3)
    check(row, got, singles, "three executions vs three rounds of single calls, " + where)


# ---- 4. recorded sequences -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct_available():
    """Does a sequence of one plain plan replay as AQL packets in this process?"""
    import torch
    a = S.StridedView(torch.zeros(64, dtype=torch.float64, device="cuda"), (8, 8), (1, 8), 0)
    q = S.Sequence().add(S.make_plan(lambda x: x, None, None, a.size, (a.similar(), a)))
    return CC.field(q.info(), "backend") == "aql"


@pytest.mark.parametrize("queues,slices", [(1, 1), (4, 1), (None, 3)])
@pytest.mark.parametrize("name", ["edges/cap/f64", "types/f64"])
def test_recorded_group_replayed_twice_stays_one_packet(name, queues, slices):
    row = GR.row(name)
    infos = []

    def replay(g):
        lay = g.layout()
        if name == "edges/cap/f64":   # large enough that a sliceable launch would be cut (csrc/smr_sched.cpp: ranges of at least 64 workgroups)
            assert lay[-1][1] + lay[-1][2] >= 64 * 3
        q = S.Sequence().add_group(g)
        if queues is not None:
            q.set("queues", queues)
        q.set("slices", slices)
        q.run(2, cur())
        q.wait()
        sync()
        infos.append(q.info())
        del q

    got = run_group(row, replay)
    check(row, got, row.expected_parent(2), "sequence replayed twice (queues %s, slices %d)" % (queues, slices))
    info = infos[0]
    assert CC.field(info, "items") == "1" and CC.field(info, "groups") == "1", info
    if direct_available():
        assert CC.field(info, "backend") == "aql", info
        assert CC.field(info, "packets") == "1" and CC.field(info, "sliced") == "0", info     # never cut into block ranges


def test_a_map_group_that_writes_the_blocks_then_the_reduction_group_that_reads_them():
    import torch
    K = 9
    rng = np.random.default_rng(5)
    shapes = [(3 + i, 4 + (3 * i) % 5) for i in range(K - 1)] + [(96, 97)]          # the last block has three workgroups
    mk = lambda a: S.StridedView(torch.from_numpy(np.asfortranarray(a).ravel(order="F").copy()).cuda(), a.shape, (1, a.shape[0]), 0)   # noqa: E731
    hostA = [rng.integers(-5, 6, size=s).astype(np.float64) for s in shapes]
    A = [mk(a) for a in hostA]
    B = [mk(np.full(s, np.nan)) for s in shapes]
    out = S.StridedView(torch.full((K,), 7.0, dtype=torch.float64, device="cuda"), (K,), (1,), 0)
    scale = lambda x: x * 2   # noqa: E731
    maps = [S.build_problem(scale, None, None, b.size, (b, a), stream=cur()) for a, b in zip(A, B)]
    reds = [S.build_problem(S.fn.abs2, "+", "zero", b.size, S.promoteshape(b.size, S.StridedView(out.parent, (1, 1), (0, 0), i), b), stream=cur()) for i, b in enumerate(B)]
    gm = L.Group([p[0] for p in maps], keepalive=maps)
    gr = L.Group([p[0] for p in reds], keepalive=reds, reduce=True)
    assert [r[2] for r in gr.layout()] == [1] * (K - 1) + [3]
    q = S.Sequence().add_group(gm).add_group(gr)
    assert q.components() == [0, 0] and q.fences()[0] == [0, 1]
    for rep in range(2):
        q.run(1, cur())
        q.wait()
        sync()
        want = np.array([float((4 * a * a).sum()) for a in hostA])
        assert np.array_equal(out.parent.cpu().numpy(), want), (rep, q.info())
        hostA = [a + 1 for a in hostA]                       # other blocks for the second replay
        for a, h in zip(A, hostA):
            a.parent.copy_(torch.from_numpy(np.asfortranarray(h).ravel(order="F").copy()))
        sync()
    info = q.info()
    assert CC.field(info, "items") == "2" and CC.field(info, "groups") == "2", info
    del q
    gm.close()
    gr.close()


# ---- 5. the front ----------------------------------------------------------------------------------------------------------------------
def test_front_37_reductions_into_a_vector_are_one_launch():
    import torch
    K = 37
    rng = np.random.default_rng(3)
    shapes = [(2 + (5 * i) % 9, 1 + (3 * i) % 7) for i in range(K - 2)] + [(70, 61), (4096,)]
    hosts = [rng.integers(-6, 7, size=s).astype(np.float64) for s in shapes]

    def operands():
        xs = [S.StridedView(torch.from_numpy(np.asfortranarray(h).ravel(order="F").copy()).cuda(), h.shape,
                            tuple(int(np.prod(h.shape[:d])) for d in range(h.ndim)), 0) for h in hosts]
        out = S.StridedView(torch.arange(K, dtype=torch.float64, device="cuda"), (K,), (1,), 0)
        return xs, out

    def calls(xs, out):
        for i, x in enumerate(xs):
            S.mapreducedim_(S.fn.abs2, "+", S.StridedView(out.parent, (1,) * x.ndim, (0,) * x.ndim, i), x)

    xs, plain = operands()
    with CC.option("reduce_blocks", 64):
        calls(xs, plain)
    sync()
    xs2, grouped = operands()
    before = S.get_option("launches")
    with S.group(reduce=True, independent=True) as g:
        calls(xs2, grouped)
    sync()
    assert len(g.groups) == 1 and g.singles == 0 and g.groups[0].count == K, [x.describe() for x in g.groups]
    assert S.get_option("launches") == before + 1
    assert "kind=reduce members=37 " in g.groups[0].describe() and "f=abs2" in g.groups[0].describe()
    want = np.array([i + float((h * h).sum()) for i, h in enumerate(hosts)])
    assert np.array_equal(grouped.parent.cpu().numpy().view(np.uint8), plain.parent.cpu().numpy().view(np.uint8))
    assert np.array_equal(plain.parent.cpu().numpy(), want)
    # without reduce=True every reduction still runs alone
    xs3, alone = operands()
    before = S.get_option("launches")
    with S.group(independent=True) as g:
        calls(xs3, alone)
    sync()
    assert not g.groups and S.get_option("launches") >= before + K
    assert np.array_equal(alone.parent.cpu().numpy(), want)
