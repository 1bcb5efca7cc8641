"""GPU: partial reduction groups (SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART, csrc/smr_k_greduce_part.hip) on the table of
tests/group_reduce_part_cases.py.

  1. every row: the WHOLE destination parent (the members' windows and the random bits around them), byte for byte, against the exact
     expected values: executed once, again on a fresh parent, and three times onto one parent; rows whose f is a program run
     runtime-compiled (asserted from the library's counters) and interpreted, with the same bytes;
  2. recorded sequences: rows replayed twice; a grid of a few hundred workgroups under "slices" = 1 and 3 with identical bytes, cut into
     block ranges (asserted from the sequence's description);
  3. the guarantee: random Float32 / Float64 / ComplexF64 data -- order-dependent sums -- over members of TR = 1, 2, 32, 64, 128 and 256:
     bit-identical to the single calls under "reduce_part_kind" = 0, which differ from the default planner's ROW / COL forms (the control);
  4. native, runtime-compiled and interpreted f of one row agree bit for bit;
  5. the front: `with S.group(reduce=True, reduce_part=True, independent=True):` around K mapreducedim_ calls is one launch per bucket."""
import functools

import numpy as np
import pytest

import contract_cases as CC
import group_reduce_part_cases as GP
import strided_jl_amd as S
from reduce_exact_cases import _index
from strided_jl_amd import _lib as L
from test_gpu_group_contract import jit_mode

pytestmark = pytest.mark.gpu
ROWS = GP.table()


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


def run_singles(row, **options):
    """Every member alone under `options`; also the plans' describe() lines."""
    dpar, views = row.views(cuda)
    members, _ = row.build()
    old = {k: L.get_option(k) for k in options}
    for k, v in options.items():
        L.set_option(k, v)
    try:
        plans = [S.make_plan(row.fn(), row.op, m.initop, m.dims, v) for m, v in zip(members, views)]
        for p in plans:
            p.execute(cur())
        out = download(dpar)
        descs = [p.describe() for p in plans]
        for p in plans:
            p.close()
    finally:
        for k, v in old.items():
            L.set_option(k, v)
    return out, descs


def check(row, got, want, what):
    err = GP.mismatch(row, got, want, what)
    assert err is None, err


def thrice(g):
    for _ in range(3):
        g.execute(cur())


# ---- 1. every row ----------------------------------------------------------------------------------------------------------------------
def exact(row, what):
    check(row, run_group(row), row.expected_parent(1), "group vs exact" + what)
    check(row, run_group(row), row.expected_parent(1), "group on a fresh parent vs exact" + what)
    check(row, run_group(row, thrice), row.expected_parent(3), "three executions onto one parent vs exact" + what)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_member_is_exact(row):
    if row.f not in ("prog", "amc"):
        exact(row, "")
        return
    with jit_mode(1):   # a runtime-compiled kernel ran: the launchers fall back to the interpreter silently, with the same results
        exact(row, ", runtime-compiled")
    with jit_mode(0):
        exact(row, ", interpreted")


# ---- 2. recorded sequences -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct_available():
    """Does a sequence of one plain plan replay as AQL packets in this process?"""
    import torch
    a = S.StridedView(torch.zeros(64, dtype=torch.float64, device="cuda"), (8, 8), (1, 8), 0)
    q = S.Sequence().add(S.make_plan(lambda x: x, None, None, a.size, (a.similar(), a)))
    return CC.field(q.info(), "backend") == "aql"


def replayed(row, slices, infos):
    def replay(g):
        q = S.Sequence().add_group(g)
        q.set("slices", slices)
        q.run(2, cur())
        q.wait()
        sync()
        infos.append(q.info())
        del q
    return run_group(row, replay)


@pytest.mark.parametrize("name", ["edges/1-33/f64", "edges/128-255/c64", "dims/rank4/f32", "bcast/matvec/f64", "ops/min/f64", "types/f32-into-f64", "count/257"])
def test_recorded_group_replayed_twice(name):
    row = GP.row(name)
    infos = []
    check(row, replayed(row, 1, infos), row.expected_parent(2), "sequence replayed twice")
    info = infos[0]
    assert CC.field(info, "items") == "1" and CC.field(info, "groups") == "1", info
    if direct_available():
        assert CC.field(info, "backend") == "aql" and CC.field(info, "packets") == "1", info     # one group = one packet


def test_recorded_group_is_cut_into_block_ranges_under_slices():
    row = GP.row("wide/f32")
    assert sum(sp.W for sp in row.specs) >= 64 * 3          # (csrc/smr_sched.cpp: ranges of at least 64 workgroups)
    whole, cut = [], []
    a = replayed(row, 1, whole)
    b = replayed(row, 3, cut)
    check(row, a, row.expected_parent(2), "sequence replayed twice, slices 1")
    check(row, b, row.expected_parent(2), "sequence replayed twice, slices 3")
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if direct_available():
        assert CC.field(whole[0], "packets") == "1" and CC.field(whole[0], "sliced") == "0", whole[0]
        assert CC.field(cut[0], "sliced") == "1" and CC.field(cut[0], "packets") == "3", cut[0]


# ---- 3. the guarantee ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ["f32", "f64", "c64"])
def test_random_sums_are_bit_identical_to_the_single_calls_general_form(t):
    """Non-integer random data: the sums depend on the order.  Every member must give the single call's bits under "reduce_part_kind" =
    0, where every member's plan reads form=general lanes_per_out=TR split=1 (asserted here and, without a device, in
    tests/test_group_reduce_part_host.py: no member is left out), and the data tell orders apart: under the default planner -- ROW and
    COL forms -- some member's bits differ (asserted, so that equal bytes above mean an equal order)."""
    row = GP.order_row(t)
    members, _ = row.build()
    rng = np.random.default_rng(20261021)
    for m in members:   # (a private row: its parents are this test's to fill)
        for o in m.ins:
            e = tuple(1 if s == 0 else n for n, s in zip(m.dims, o.strides))
            idx = _index(o.offset, e, o.strides).ravel()
            v = rng.standard_normal(idx.size) + (1j * rng.standard_normal(idx.size) if t == "c64" else 0)
            o.parent[idx] = v.astype(o.parent.dtype)
    before = L.get_option("reduce_part_kind")
    got = run_group(row)
    singles, descs = run_singles(row, reduce_part_kind=0)
    assert L.get_option("reduce_part_kind") == before
    skipped = [d for d, m in zip(descs, members)
               if not (d.startswith("family=reduce_part ") and CC.field(d, "form") == "general" and CC.field(d, "split") == "1" and int(CC.field(d, "lanes_per_out")) == m.spec.tr)]
    assert not skipped, skipped
    check(row, got, singles, "group vs single calls under reduce_part_kind = 0, random data")
    default, ddescs = run_singles(row)
    assert {CC.field(d, "form") for d in ddescs} & {"row", "col"}, ddescs
    assert GP.mismatch(row, default, singles, "") is not None, "the data do not tell accumulation orders apart"


# ---- 4. how f runs ---------------------------------------------------------------------------------------------------------------------
class ProgRow(GP.Row):
    """the row's members with x * y * 1 for f: the same values, but a program with a constant instead of the native product"""

    def fn(self):
        return lambda x, y: x * y * 1


def test_native_runtime_compiled_and_interpreted_f_agree():
    native = GP.row("f/mul/f64")
    prog = ProgRow("f/mul/f64", native.t, native.op, native.f, native.kind, native.specs)
    want = native.expected_parent(1)
    dpar, views = native.views(cuda)
    g = native.group(views, stream=cur())
    assert CC.field(g.describe(), "f") == "mul2" and CC.field(g.describe(), "jit") == "0"
    g.execute(cur())
    a = download(dpar)
    g.close()
    check(native, a, want, "native f")
    for jit in (1, 0):
        with jit_mode(jit):
            dpar, views = prog.views(cuda)
            g = prog.group(views, stream=cur())
            assert CC.field(g.describe(), "f") == "prog" and CC.field(g.describe(), "jit") == str(jit), g.describe()
            g.execute(cur())
            b = download(dpar)
            g.close()
        check(native, b, want, "f as a program, jit = %d" % jit)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 5. the front ----------------------------------------------------------------------------------------------------------------------
def test_front_one_launch_per_bucket():
    import torch
    K = 24
    rng = np.random.default_rng(3)
    shapes = [(2 + (5 * i) % 9, 1 + (3 * i) % 7) for i in range(K - 2)] + [(70, 61), (32, 32)]
    hosts = [rng.integers(-6, 7, size=s).astype(np.float64) for s in shapes]
    xs_host = [rng.integers(-3, 4, size=s[1]).astype(np.float64) for s in shapes]
    nrow = sum(s[0] for s in shapes)

    def operands():
        mk = lambda h: torch.from_numpy(np.asfortranarray(h).ravel(order="F").copy()).cuda()   # noqa: E731
        As = [S.StridedView(mk(h), h.shape, (1, h.shape[0]), 0) for h in hosts]
        xs = [S.StridedView(mk(x), (h.shape[0], x.size), (0, 1), 0) for h, x in zip(hosts, xs_host)]
        y = torch.arange(2 * nrow, dtype=torch.float64, device="cuda")          # y[2 r]: row sums of abs2; y[2 r + 1]: A x  (interleaved)
        return As, xs, y

    def calls(As, xs, y):
        r = 0
        for A, x in zip(As, xs):
            n = A.size[0]
            S.mapreducedim_(S.fn.abs2, "+", S.StridedView(y, (n, 1), (2, 0), 2 * r), A)
            S.mapreducedim_(lambda u, v: u * v, "+", S.StridedView(y, (n, 1), (2, 0), 2 * r + 1), A, x)
            r += n

    As, xs, plain = operands()
    calls(As, xs, plain)
    sync()
    As2, xs2, grouped = operands()
    before = S.get_option("launches")
    with S.group(reduce=True, reduce_part=True, independent=True) as g:
        calls(As2, xs2, grouped)
    sync()
    descs = [x.describe() for x in g.groups]
    assert len(g.groups) == 2 and g.singles == 0 and [x.count for x in g.groups] == [K, K], descs     # one launch per bucket
    assert S.get_option("launches") == before + 2
    assert all("kind=reduce_part members=%d " % K in d for d in descs) and {CC.field(d, "f") for d in descs} == {"abs2", "mul2"}, descs
    want = np.arange(2 * nrow, dtype=np.float64)
    r = 0
    for h, x in zip(hosts, xs_host):
        n = h.shape[0]
        want[2 * r:2 * (r + n):2] += (h * h).sum(axis=1)
        want[2 * r + 1:2 * (r + n):2] += h @ x
        r += n
    assert np.array_equal(plain.cpu().numpy(), want)
    assert np.array_equal(grouped.cpu().numpy().view(np.uint8), plain.cpu().numpy().view(np.uint8))
    # with reduce=True alone every partial reduction still runs alone
    As3, xs3, alone = operands()
    before = S.get_option("launches")
    with S.group(reduce=True, independent=True) as g:
        calls(As3, xs3, alone)
    sync()
    assert not g.groups and S.get_option("launches") >= before + 2 * K
    assert np.array_equal(alone.cpu().numpy(), want)
