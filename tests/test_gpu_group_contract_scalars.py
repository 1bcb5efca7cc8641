"""GPU: contraction groups with per-member constants of f (SMR_GROUP_CONTRACT_SCALARS; csrc/smr_k_gcontract.hip, the varc bodies) on the
table of tests/group_contract_scalar_cases.py.

  1. every row: each member's WHOLE destination parent, byte for byte, against NumPy (the member's own constants) and against the
     same member run alone under contract = 2 (a split member: also contract_tile = the group's tile, contract_split = its slices);
     rows whose f is a program run runtime-compiled (asserted from the library's counters) and interpreted, with the same bytes;
  2. the runtime-compiled text does not depend on the constants: a second group with other values is a cache hit, no compilation;
  3. order: random Float32 / Float64 data and a random alpha per member against the sequential loop acc = acc + (a * b) * alpha;
  4. dispatch: plain HIP, a library-owned stream, a recorded sequence replayed twice and the same sequence in three block ranges;
  5. the front: 37 mul_ calls with 37 alphas inside `with S.group(contract=True, contract_scalars=True):` are ONE launch."""
import functools

import numpy as np
import pytest

import contract_cases as CC
import group_contract_scalar_cases as GS
import strided_jl_amd as S
import window_cases as W
from util import to_device

pytestmark = pytest.mark.gpu
ROWS = GS.table()


class jit_mode:
    """with jit_mode(jit): the "jit" option set and restored; under jit = 1 the block must have run a runtime-compiled kernel (a code
    object compiled or found in the cache, and no failure), under jit = 0 none (tests/test_gpu_group_contract.py: jit_mode)."""

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
    devs, caches = [], []
    for ops in built:
        cache = {}
        devs.append(tuple(to_device(a, cache) for a in ops))
        caches.append(cache)
    return devs, caches


def parents(built, caches):
    sync()
    return [cache[ops[0].parent.ctypes.data].cpu().numpy() for ops, cache in zip(built, caches)]


def run_group(row, built, how=lambda g: g.execute(stream()), check=None):
    devs, caches = upload(built)
    g = row.group(devs, stream=stream())
    d = g.describe()
    assert d.endswith(" scalars=shared" if row.shared else " scalars=member") and CC.field(d, "f") == row.f_tag, d
    if check:
        check(g)
    how(g)
    out = parents(built, caches)
    g.close()
    return out


def slices_of(row, built):
    """(the group's tile, slices per member) as planned: what the single calls of split members are run under."""
    g = row.group(built)
    tile = int(CC.field(g.describe(), "tile"))
    sl = [s[0] for s in g.split_layout()] or [1] * len(row.members)
    g.close()
    return tile, sl


def run_singles(row, built, times=1):
    """Every member alone with its own constants, `times` times, under contract = 2 -- a split member also under the group's tile and
    its own number of slices."""
    tile, sl = slices_of(row, built)
    devs, caches = upload(built)
    with CC.option("contract", 2):
        for _ in range(times):
            for i, (c, dev) in enumerate(zip(row.members, devs)):
                if sl[i] >= 2:
                    with CC.option("contract_tile", tile), CC.option("contract_split", sl[i]):
                        c.call(dev, row.initop(i))
                else:
                    c.call(dev, row.initop(i))
    return parents(built, caches)


def compare(row, got, want, what):
    for c, g, w in zip(row.members, got, want):
        msg = GS.mismatch(c, g, w, "%s | %s" % (row.name, what))
        assert msg is None, msg


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_member_is_exact_and_the_single_calls_bytes(row):
    built = row.build()
    want = row.expected(built)
    if row.split:
        assert max(slices_of(row, built)[1]) >= 2 and min(slices_of(row, built)[1]) == 1, "the row mixes split and unsplit members"
    if row.f_tag == "mul2scale":   # the native functor; the single calls run x * y * alpha as a program, runtime-compiled and interpreted
        compare(row, run_group(row, built), want, "group, native, vs NumPy")
        with jit_mode(1):
            compare(row, run_singles(row, built), want, "single calls, runtime-compiled, vs NumPy")
        if len(row.members) <= 300:   # (the 2049 single calls once: the suite stays quick)
            with jit_mode(0):
                compare(row, run_singles(row, built), want, "single calls, interpreted, vs NumPy")
        return
    with jit_mode(1):
        compare(row, run_group(row, built), want, "group, runtime-compiled, vs NumPy")
        compare(row, run_singles(row, built), want, "single calls, runtime-compiled, vs NumPy")
    with jit_mode(0):
        compare(row, run_group(row, built), want, "group, interpreted, vs NumPy")
        compare(row, run_singles(row, built), want, "single calls, interpreted, vs NumPy")


def test_other_constants_reuse_the_runtime_compiled_code_object():
    """The text of the runtime-compiled kernel depends on f's structure only: after one group has run, a group of the same shape with
    other values in its table adds a cache hit and no compilation -- unsplit and split."""
    for name in ("f32/dist2/n12/t16/distinct", "f32/dist2/split4/t32/distinct"):
        row = GS.row(name)
        built = row.build()
        with CC.option("jit", 1):
            compare(row, run_group(row, built), row.expected(built), "first group")
            other = GS.SRow(row.name + "/other", row.tn, [(c.dims, c.axes, c.layouts, None) for c in row.members], row.kind, row.tile, f=row.fname,
                            split=row.split, consts=[tuple(type(v)(v * 2 + 1) for v in cs) for cs in reversed(row.consts)])
            built2 = other.build()
            before = [S.get_option(k) for k in ("jit_compiles", "jit_hits", "jit_failures")]
            compare(other, run_group(other, built2), other.expected(built2), "second group, other constants")
            after = [S.get_option(k) for k in ("jit_compiles", "jit_hits", "jit_failures")]
        assert after[0] == before[0] and after[1] > before[1] and after[2] == before[2], (name, before, after)


# ---- accumulation order ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("tn", ["f32", "f64"])
def test_accumulation_order_is_the_sequential_loop_with_alpha_inside(tn, tile):
    """Random non-integer data and a random alpha per member (fixed seed), 12 members, beta = 2 + i % 3: every member bit for bit
    acc = -0.0; k ascending: acc = acc + (a * b) * alpha; C = old * beta + acc.  Scaling the finished sum, (sum of a * b) * alpha,
    differs from it in some member for this seed (asserted on the host first)."""
    dt = GS.TYPES[tn][0]
    rng = np.random.default_rng(20261021)
    specs = [s for s in GS.specs_for(tn, 37)[:-1] if len(s[0]) == 3][:11] + GS.specs_for(tn, 2)[1:]   # plain products: (m, n, k)
    assert len(specs) == 12
    alphas = [(dt(rng.standard_normal()),) for _ in specs]
    row = GS.SRow("order/%s/t%d" % (tn, tile), tn, specs, "scale", tile, consts=alphas)
    built = row.build()
    want, differs = [], False
    for i, (case, ops) in enumerate(zip(row.members, built)):
        for a in ops:
            u = np.unique(W.element_index(a).ravel())
            a.parent[u] = rng.standard_normal(u.size).astype(dt)
        beta, alpha = dt(row.initop(i)[1]), alphas[i][0]
        m, n, k = case.dims
        A, B = (np.broadcast_to(x.toarray().astype(dt), case.dims) for x in ops[1:])
        acc, plain = np.full((m, n), -0.0, dtype=dt), np.full((m, n), -0.0, dtype=dt)
        for kk in range(k):
            prod = (A[:, :, kk] * B[:, :, kk]).astype(dt)
            acc = (acc + (prod * alpha).astype(dt)).astype(dt)
            plain = (plain + prod).astype(dt)
        old = ops[0].toarray().astype(dt).reshape(m, n)
        view = (old * beta + acc).astype(dt)
        outside = (old * beta + (plain * alpha).astype(dt)).astype(dt)
        differs = differs or not np.array_equal(view.view(np.uint8), outside.view(np.uint8))
        w = ops[0].parent.copy()
        w[W.element_index(ops[0]).ravel()] = view.ravel()
        want.append(w)
    assert differs, "the seed does not tell alpha inside the sum from alpha outside"
    compare(row, run_group(row, built), want, "sequential order")


# ---- dispatch -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct_available():
    """Does a sequence of one plain plan replay as AQL packets in this process?  (No: the direct path is switched off or failed.)"""
    import torch
    a = S.StridedView(torch.zeros(64, dtype=torch.float64, device="cuda"), (8, 8), (1, 8), 0)
    q = S.Sequence().add(S.make_plan(lambda x: x, None, None, a.size, (a.similar(), a)))
    return CC.field(q.info(), "backend") == "aql"


@pytest.mark.parametrize("name", ["f32/mula/n300/t32/distinct", "f64/dist2/n120/t0/distinct"])
def test_dispatch_paths_give_the_same_bytes(name):
    row = GS.row(name)
    assert row.kind == "none"   # beta = 1: every execution accumulates
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
                # a cut inside a member: the range behind it starts with that member's later tiles, and finds the member's row
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
def test_front_37_products_with_37_alphas_are_one_launch():
    import torch
    MN = (2, 15, 16, 17, 31, 32, 33, 48)
    shapes = [(max(MN[(3 * i + 1) % 8], 3), max(MN[(5 * i + 2) % 8], 3), 3 + (7 * i) % 40) for i in range(37)]
    # (none integer-valued: whether all constants are is part of the bucket key, as for maps under member_scalars)
    alphas = [GS.alpha_of("f64", i, 37, "distinct") + 0.125 for i in range(37)]
    assert len(set(alphas)) == 37

    def operands():
        out = []
        r = np.random.default_rng(11)
        for m, n, k in shapes:
            mk = lambda *s: S.StridedView(torch.from_numpy(r.integers(-3, 4, size=int(np.prod(s))).astype(np.float64)).cuda(), s,  # noqa: E731
                                          tuple(int(np.prod(s[:d])) for d in range(len(s))), 0)
            out.append((mk(m, n), mk(m, k), mk(k, n)))
        return out

    def calls(ops):
        for i, (Cm, A, B) in enumerate(ops):
            S.mul_(Cm, A, B, alphas[i], 2 + i % 5)

    plain, grouped = operands(), operands()
    with CC.option("contract", 2):
        calls(plain)
    sync()
    before = S.get_option("launches")
    with S.group(contract=True, contract_scalars=True) as g:
        calls(grouped)
    sync()
    assert S.get_option("launches") == before + 1, [x.describe() for x in g.groups]
    assert g.singles == 0 and [x.count for x in g.groups] == [37]
    d = g.groups[0].describe()
    assert "kind=contract" in d and " f=mul2scale " in d and d.endswith(" scalars=member"), d
    for (Cp, *_), (Cg, *_), shp in zip(plain, grouped, shapes):
        assert np.array_equal(Cp.toarray().view(np.uint8), Cg.toarray().view(np.uint8)), shp
    # without the keyword the same calls are 37 groups of one member
    before = S.get_option("launches")
    with S.group(contract=True) as g:
        calls(grouped)
    sync()
    assert S.get_option("launches") == before + 37 and [x.count for x in g.groups] == [1] * 37
