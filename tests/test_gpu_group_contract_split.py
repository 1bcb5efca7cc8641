"""GPU: split contraction groups (csrc/smr_k_gcontract.hip: k_group_contract_split, k_group_contract_fold; option
"group_contract_split") on the table of tests/group_contract_split_cases.py: a forced tile and forced slices per row.

  1. every row: each member's WHOLE destination parent, byte for byte, against NumPy's result (Case.expected);
  2. ... and against the same member run alone under contract = 2, contract_tile = the group's tile and contract_split = S_i (plain
     contract = 2 for the members the group leaves unsplit); rows whose f is a program run runtime-compiled and, for `dist`, interpreted;
  3. order: random Float32 / Float64 data against the host loop the split form's order defines (the loop of
     tests/test_gpu_contract_split.py), bit for bit, with a beta per member;
  4. one group executed twice on one destination, after a first run on NaN inputs that leaves NaN in every partial;
  5. on a library-owned stream;
  6. recorded with Sequence.add_group and replayed twice, uncut and cut into three block ranges ("slices" 1 and 3) under 1 and 4
     queues: one item, one group; two launches per replay uncut, the three ranges and the fold on one queue when cut;
  7. the front: `with S.group(contract=True)` under group_contract_split = 2 around a few mul_ calls is two launches."""
import numpy as np
import pytest

import contract_cases as CC
import contract_split_cases as SC
import group_contract_cases as GC
import group_contract_split_cases as GS
import strided_jl_amd as S
import test_gpu_contract_split as TS
import test_gpu_group_contract as TG
from util import to_device

pytestmark = pytest.mark.gpu
ROWS = GS.table()
sync, stream, upload, parents, compare, jit_mode = TG.sync, TG.stream, TG.upload, TG.parents, TG.compare, TG.jit_mode


def run_group(row, built, how=lambda g: g.execute(stream())):
    """(parents, split_layout) of the row's group executed by `how` on fresh device copies."""
    devs, caches = upload(built)
    g = row.group(devs, stream=stream())
    sl = g.split_layout()
    assert sl and int(CC.field(g.describe(), "tile")) == row.tile, g.describe()
    how(g)
    out = parents(built, caches)
    g.close()
    return out, sl


def run_singles(row, built, sl, times=1):
    """Every member alone, `times` times, as the single call the contract names: contract = 2, the group's tile, contract_split = S_i
    (0 for an unsplit member); a split member's plan must have exactly S_i slices of cps_i chunks."""
    devs, caches = upload(built)
    for i, (c, dev, (Si, cps, _, _)) in enumerate(zip(row.members, devs, sl)):
        with SC.split_options(row.tile, Si if Si >= 2 else 0):
            p = c.plan(dev, row.initop(i))
            d = p.describe()
            p.close()
            assert CC.family(d) == CC.CONTRACT and CC.tile_of(d)[1] == row.tile, d
            assert SC.slices(d)[:2] == ((Si, cps) if Si >= 2 else (1, 0)), (d, Si, cps)
            for _ in range(times):
                c.call(dev, row.initop(i))
    return parents(built, caches)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_member_is_exact_and_the_split_single_calls_bytes(row):
    built = row.build()
    want = row.expected(built)

    def check(what):
        got, sl = run_group(row, built)
        compare(row, got, want, "group vs NumPy, " + what)
        compare(row, run_singles(row, built, sl), got, "single calls vs group, " + what)

    if not row.needs_prog:
        check("native")
        return
    with jit_mode(1):
        check("runtime-compiled")
    if row.fname == "dist":
        with jit_mode(0):
            check("interpreted")


# ---- 3. order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", GS.TILES)
@pytest.mark.parametrize("tn", ["f32", "f64"])
def test_accumulation_order_of_split_members_is_the_sliced_sequential_loop(tn, tile):
    """dest = old * beta_i + (((P_0 + P_1) + P_2) ...), P_s the sequential sum from -0.0 over the chunks of slice s; an unsplit member
    is the plain sequential loop.  In some member the sliced loop differs from the plain one for this seed (asserted on the host)."""
    dt = GS.TYPES[tn][0]
    tk = GC.tk_of(tn)
    row = GS.Row("order/%s/t%d" % (tn, tile), tn, GS.TYPES[tn], GS.members_mixed(tile, tk, 10), "scale", tile, 3)
    built = row.build()
    rng = np.random.default_rng(20261020)
    for ops in built:
        for a in ops:
            u = np.unique(GC.W.element_index(a).ravel())
            a.parent[u] = rng.standard_normal(u.size).astype(dt)
    got, sl = run_group(row, built)
    want, differs = [], False
    for i, (c, ops, (Si, cps, _, _)) in enumerate(zip(row.members, built, sl)):
        beta = row.initop(i)[1]
        old = ops[0].toarray().astype(dt)
        case = SC.SplitCase(c.name, c.dims, c.axes, c.dts, tile, Si if Si >= 2 else 0, layouts=c.layouts)
        A, B = (x.toarray().astype(dt) for x in ops[1:])
        Af, Bf = np.broadcast_to(A, c.dims), np.broadcast_to(B, c.dims)
        rd, tk_, kparts, cps_ = TS._reduced_order(case, ops)
        chunks = TS._chunks(case, rd, tk_)
        plain = TS._accumulate(case, Af, Bf, rd, [x for ch in chunks for x in ch], dt)
        if Si >= 2:
            assert (kparts, cps_) == (Si, cps)
            parts = [TS._accumulate(case, Af, Bf, rd, [x for ch in chunks[s * cps:(s + 1) * cps] for x in ch], dt) for s in range(Si)]
            total = parts[0]
            for p in parts[1:]:
                total = (total + p).astype(dt)
            differs = differs or not np.array_equal(total.view(np.uint8), plain.view(np.uint8))
        else:
            assert kparts == 1
            total = plain
        w = ops[0].parent.copy()
        w[GC.W.element_index(ops[0]).ravel()] = (old * dt(beta) + total).astype(dt).ravel()
        want.append(w)
    assert differs, "the seed does not tell the sliced loop from the plain one"
    assert sum(s[0] >= 2 for s in sl) >= 4 and sum(s[0] == 1 for s in sl) >= 3
    compare(row, got, want, "sliced sequential order")


# ---- 4. again, and stale partials ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32/t16/n17_mixed_s3", "f64/t32/n3_3tk+1_s64"])
def test_twice_on_one_destination_after_a_run_that_left_nan_in_the_partials(name):
    import torch
    base = GS.row(name)
    row = GS.Row("again/" + name, base.tn, base.dts, [(c.dims, c.axes, c.layouts, c.conjs) for c in base.members], "none", base.tile, base.S)
    built = row.build()
    poisoned = [(ops[0],) + tuple(S.StridedView(np.full_like(a.parent, np.nan), a.size, a.strides, a.offset, a.op) for a in ops[1:]) for ops in built]
    devs, caches = [], []
    for ops in poisoned:
        cache = {}
        devs.append(tuple(to_device(a, cache) for a in ops))
        caches.append(cache)
    g = row.group(devs, stream=stream())
    sl = g.split_layout()
    g.execute(stream())                      # every partial, and every destination, is NaN now
    sync()
    assert all(np.isnan(cache[ops[0].parent.ctypes.data].cpu().numpy()[GC.W.element_index(ops[0]).ravel()]).all() for ops, cache in zip(poisoned, caches))
    for real, fake, dev, cache in zip(built, poisoned, devs, caches):   # the real data into the same device buffers
        for a, b in zip(real, fake):
            cache[b.parent.ctypes.data].copy_(torch.from_numpy(a.parent))
    sync()
    g.execute(stream())
    g.execute(stream())
    got = parents(poisoned, caches)
    g.close()
    compare(row, got, run_singles(row, built, sl, times=2), "two executions after a NaN run")


# ---- 5. / 6. dispatch ----------------------------------------------------------------------------------------------------------------
def dispatch_row(kind):
    if kind == "native":
        return GS.row("f64/t16/n257_tiny_s2")
    return GS.row("f32/t16/n4_dist_s3")


@pytest.mark.parametrize("kind", ["native", "runtime-compiled"])
def test_dispatch_paths_give_the_same_bytes(kind):
    row = dispatch_row(kind)
    built = row.build()
    with CC.option("jit", 1):
        ref, sl = run_group(row, built)
        compare(row, ref, row.expected(built), "plain HIP vs NumPy")
        once, twice = run_singles(row, built, sl, 1), run_singles(row, built, sl, 2)
        compare(row, ref, once, "plain HIP")

        def owned(g):
            with S.Stream() as st:
                g.execute(st.handle)
            st.close()

        compare(row, run_group(row, built, owned)[0], once, "library-owned stream")
        infos = {}

        def sequence(slices, queues):
            def run(g):
                lay = g.layout()
                grid = lay[-1][1] + lay[-1][2]
                cut = slices > 1 and grid >= 64 * slices
                if kind == "native":   # the main launch is cut in three, inside members: workgroups run with wg0 > 0
                    per = ((grid + slices - 1) // slices + 7) & ~7
                    cuts = [per * k for k in range(1, slices) if per * k < grid]
                    assert slices == 1 or (cut and len(cuts) == slices - 1 and any(x not in {r[1] for r in lay} for x in cuts)), (grid, cuts)
                q = S.Sequence().add_group(g)
                q.set("slices", slices)
                q.set("queues", queues)
                before = S.get_option("launches")
                q.run(2, stream())
                q.wait()
                sync()
                infos[(slices, queues)] = (q.info(), S.get_option("launches") - before, cut)
                del q
            return run

        for slices in (1, 3):
            for queues in (1, 4):
                compare(row, run_group(row, built, sequence(slices, queues))[0], twice, "sequence replayed twice, slices=%d queues=%d" % (slices, queues))
    for (slices, queues), (info, launches, cut) in infos.items():
        assert CC.field(info, "items") == "1" and CC.field(info, "groups") == "1", info
        if TG.direct_available() and kind == "native":
            assert CC.field(info, "backend") == "aql", info
        if CC.field(info, "backend") == "aql":
            # uncut: the main launch and the fold; cut: the block ranges back to back on the item's one queue, then the fold
            assert CC.field(info, "packets") == str(slices + 1 if cut else 2) and CC.field(info, "sliced") == ("1" if cut else "0"), (slices, queues, info)
            assert CC.field(info, "queues") == "1", info
        else:
            assert launches == 4, (slices, queues, info, launches)


# ---- 7. the front --------------------------------------------------------------------------------------------------------------------
def test_front_a_few_long_products_are_two_launches():
    import torch
    tk = GC.tk_of("f64")
    shapes = [(17, 15, 3 * tk + 1), (16, 16, 2 * tk), (33, 31, 5 * tk), (12, 10, 7), (20, 24, tk + 1)]

    def operands():
        out = []
        r = np.random.default_rng(11)
        for m, n, k in shapes:
            mk = lambda *s: S.StridedView(torch.from_numpy(r.integers(-3, 4, size=int(np.prod(s))).astype(np.float64)).cuda(), s,  # noqa: E731
                                          tuple(int(np.prod(s[:d])) for d in range(len(s))), 0)
            out.append((mk(m, n), mk(m, k), mk(k, n)))
        return out

    grouped, plain = operands(), operands()
    sync()
    before = S.get_option("launches")
    with GS.split_option(2):
        with S.group(contract=True) as g:
            for i, (Cm, A, B) in enumerate(grouped):
                S.mul_(Cm, A, B, 1, 2 + i % 3)
    sync()
    (grp,) = g.groups
    d, sl = grp.describe(), grp.split_layout()
    assert S.get_option("launches") == before + 2 and g.singles == 0, d
    assert CC.field(d, "split") == "4" and CC.field(d, "kparts") == "2" and [s[0] for s in sl] == [2, 2, 2, 1, 2], d
    for i, ((Cm, A, B), (Si, _, _, _)) in enumerate(zip(plain, sl)):
        with SC.split_options(int(CC.field(d, "tile")), Si if Si >= 2 else 0):
            S.mul_(Cm, A, B, 1, 2 + i % 3)
    sync()
    for (Cp, *_), (Cg, *_), shp in zip(plain, grouped, shapes):
        assert np.array_equal(Cp.toarray().view(np.uint8), Cg.toarray().view(np.uint8)), shp
    r = np.random.default_rng(11)   # ... and exact: integer data
    for (m, n, k), (Cg, *_), i in zip(shapes, grouped, range(5)):
        c0, a, b = (r.integers(-3, 4, size=s).astype(np.float64).reshape(sh, order="F") for s, sh in ((m * n, (m, n)), (m * k, (m, k)), (k * n, (k, n))))
        assert np.array_equal(Cg.toarray(), (2 + i % 3) * c0 + a @ b), (m, n, k)
