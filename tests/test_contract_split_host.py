"""The split form of the CONTRACT family without a device: the options "contract_split" and "contract_tile", the rule and the gate,
the slice arithmetic, and the case table of tests/contract_split_cases.py (smr_plan_create and describe() need no device).

describe() of every row of tests/contract_cases.py is taken when this module is imported, before either option is touched."""
import numpy as np
import pytest

import contract_cases as CC
import contract_split_cases as SC
import group_contract_cases as GC
import strided_jl_amd as S
from test_contract_host import describe_named, mul_plan_desc, sample_names

ROWS = CC.table()
SPLIT_ROWS = SC.table()


def _describe_all(contract):
    out = []
    with CC.option("contract", contract):
        for case in ROWS:
            p = case.plan(case.build(), "zero" if case.op else None)
            out.append(p.describe())
            p.close()
    return out


BEFORE = {c: _describe_all(c) for c in (2, 1)}  # (only the "contract" option has been set so far)


def test_defaults_and_values():
    assert S.get_option("contract_split") == 0 and S.get_option("contract_tile") == 0
    for name, bad in (("contract_split", -1), ("contract_split", -7), ("contract_tile", 8), ("contract_tile", 48), ("contract_tile", -16),
                      ("contract_tile", 128), ("contract_tile", 1)):
        with pytest.raises(Exception) as e:
            S.set_option(name, bad)
        assert name in str(e.value), str(e.value)
        assert S.get_option(name) == 0
    for name, good in (("contract_split", 1), ("contract_split", 2), ("contract_split", 1000), ("contract_tile", 16), ("contract_tile", 32),
                       ("contract_tile", 64)):
        with CC.option(name, good):
            assert S.get_option(name) == good
        assert S.get_option(name) == 0


@pytest.mark.parametrize("contract", [2, 1])
def test_with_both_options_at_zero_every_plan_is_the_one_from_before(contract):
    # set and restored once: the options' code has run, the values are the defaults again
    with CC.option("contract_split", 4), CC.option("contract_tile", 32):
        pass
    assert S.get_option("contract_split") == 0 and S.get_option("contract_tile") == 0
    now = _describe_all(contract)
    assert now == BEFORE[contract]
    assert not any("kparts=" in d for d in now)


def _mul(m, n, k, dt, **opts):
    ctx = [CC.option(k_, v) for k_, v in opts.items()]
    for c in ctx:
        c.__enter__()
    try:
        return mul_plan_desc(m, n, k, dt)
    finally:
        for c in reversed(ctx):
            c.__exit__(None, None, None)


def test_the_rule_splits_few_outputs_with_a_long_reduced_range():
    assert S.get_option("contract") == 1
    for dt in (np.float32, np.float64):
        d = _mul(64, 64, 4096, dt, contract_split=1)
        assert CC.family(d) == "contract" and SC.slices(d)[0] >= 2, d
        assert "split=" not in d and CC.field(d, "fold") == "second-launch", d
        assert int(CC.field(d, "grid")) * SC.slices(d)[0] >= 256, d
        assert CC.family(_mul(64, 64, 4096, dt)) == "reduce_part"


def test_the_rule_leaves_everything_else_alone():
    assert S.get_option("contract") == 1
    for m, n, k, dt in ((1024, 1024, 1024, np.float32), (512, 512, 512, np.float64), (256, 256, 256, np.float32), (128, 128, 64, np.float32),
                        (40, 40, 40, np.float32)):
        d0, d1 = _mul(m, n, k, dt), _mul(m, n, k, dt, contract_split=1)
        assert d0 == d1, (d0, d1)
    assert CC.family(_mul(40, 40, 40, np.float32, contract_split=1)) == "reduce_part"
    assert CC.family(_mul(128, 128, 64, np.float32, contract_split=1)) == "reduce_part"
    # min-plus and an interpreted f stay with REDUCE_PART at the shape the rule splits: the gate's other conditions are unchanged
    minplus = CC.Case("gate", (64, 64, 4096), CC.MM, CC.TYPES["f64"], CC.CONTRACT, layouts=("whole",) * 3, f="plus", op="min")
    dist = CC.Case("gate", (64, 64, 4096), CC.MM, CC.TYPES["f32"], CC.CONTRACT, layouts=("whole",) * 3, f="dist")

    def desc(case):
        p = case.plan(case.build())
        d = p.describe()
        p.close()
        return d

    with CC.option("contract_split", 1):
        assert CC.family(desc(minplus)) == "reduce_part"
        d = desc(dist)
        assert CC.family(d) == "contract" and SC.slices(d)[0] >= 2, d  # (runtime-compiled: the gate lets it through)
        with CC.option("jit", 0):
            assert CC.family(desc(dist)) == "reduce_part"


def test_the_rule_steals_nothing_from_the_fuzz_tables():
    names = sample_names()
    assert len(names) >= 30
    moved = []
    for name in names:
        with CC.option("contract_split", 1):
            d1 = describe_named(name)
        d0 = describe_named(name)
        if d1 != d0:
            assert CC.family(d1) == "contract", (name, d1, d0)
            moved.append(name)
    print("[contract_split] %d pinned rows planned under contract_split = 1 and 0, %d moved" % (len(names), len(moved)))
    assert moved == [], moved


# ---- slice arithmetic ----------------------------------------------------------------------------------------------------------------
def check_slices(case, tile, want_s, es):
    """The tokens of the plan of `case` under (tile, want_s) against the arithmetic of the issue; returns (kparts, cps, nchunks, nkc, vec)."""
    ops = case.build()
    with SC.split_options(tile, want_s):
        p = case.plan(ops)
        d = p.describe()
        p.close()
    with SC.split_options(tile, 0):
        p = case.plan(ops)
        d0 = p.describe()
        p.close()
    assert CC.family(d) == "contract" and CC.family(d0) == "contract", (d, d0)
    assert "kparts=" not in d0 and "split=" not in d, (d, d0)
    for key in ("grid", "tile", "k", "lds", "vec", "dims"):
        assert CC.field(d, key) == CC.field(d0, key), (key, d, d0)
    _, ti, _, tj, tk = CC.tile_of(d)
    assert ti == tile and tj == tile, d
    cdims = [int(x) for x in CC.field(d, "dims").split("x")]
    nred = len([r for r in case.rdims if case.dims[r] > 1])
    red = cdims[len(cdims) - nred:]
    K, Q = red[0], int(np.prod(red[1:], dtype=np.int64))
    nkc = -(-K // tk)
    nchunks = Q * nkc
    kparts, cps, scratch = SC.slices(d)
    if nchunks == 1 or want_s < 2:
        assert kparts == 1 and "kparts=" not in d and "fold=" not in d, d
        return 1, 0, nchunks, nkc, int(CC.field(d, "vec"))
    assert kparts >= 2, d
    assert (kparts - 1) * cps < nchunks <= kparts * cps, (nchunks, d)
    assert kparts <= want_s, d
    assert cps == -(-nchunks // min(want_s, nchunks)), (nchunks, d)
    assert scratch == int(CC.field(d, "grid")) * kparts * tile * tile * es, d
    assert CC.field(d, "fold") == "second-launch", d
    return kparts, cps, nchunks, nkc, int(CC.field(d, "vec"))


def _es(dts):
    return max(np.dtype(dts[0]).itemsize, 8 if np.dtype(dts[0]).kind in "ib" else 0)  # (integers and Bool compute in Int64)


@pytest.mark.parametrize("case", SPLIT_ROWS, ids=[c.name for c in SPLIT_ROWS])
def test_slices_of_the_table(case):
    kparts, cps, nchunks, _, _ = check_slices(case, case.tile, case.S, _es(case.dts))
    assert kparts >= 2, "every row of the table is split"


def test_slices_of_random_shapes():
    rng = np.random.default_rng(20261020)
    types = ["f32", "f64", "c64", "i64"]
    seen = set()
    for it in range(200):
        tn = types[it % 4]
        tile = SC.TILES[int(rng.integers(0, 3))]
        tk = CC.tile_numbers(tn, tile)[2]
        m, n = int(rng.integers(2, 80)), int(rng.integers(2, 80))
        k = int(rng.integers(2, 6 * tk))
        want = int((2, 3, 4, 5, 7, 8, 16, 64, 1000)[int(rng.integers(0, 9))])
        if it % 3 == 0:
            dims, axes = (m, n, k, int(rng.integers(2, 5))), ((0, 1), (0, 2, 3), (1, 2, 3))
        else:
            dims, axes = (m, n, k), CC.MM
        case = CC.Case("random%d" % it, dims, axes, CC.TYPES[tn], CC.CONTRACT)
        kparts, cps, nchunks, _, _ = check_slices(case, tile, want, _es(CC.TYPES[tn]))
        seen.add((kparts == 1, kparts == want, nchunks < want))
    assert len(seen) >= 3, seen  # unsplit (one chunk), the slices asked for, and clamped ones


def test_contract_tile_is_honoured_and_subject_to_the_lds_budget():
    for dt in (np.float32, np.float64, np.complex128):
        rule = CC.tile_of(_mul(64, 64, 16, dt, contract=2))[1]
        assert rule == 16
        for tile in (16, 32, 64):
            d = _mul(64, 64, 16, dt, contract=2, contract_tile=tile)
            assert CC.family(d) == "contract" and CC.tile_of(d)[1] == tile and CC.tile_of(d)[3] == tile, d
            d = _mul(2048, 2048, 64, dt, contract=2, contract_tile=tile)
            assert CC.family(d) == "contract" and CC.tile_of(d)[1] == tile, d
            ds = _mul(64, 64, 4096, dt, contract=2, contract_tile=tile, contract_split=1)
            assert CC.family(ds) == "contract" and CC.tile_of(ds)[1] == tile, ds
        # a forced tile beyond the budget is not exchanged for a smaller one: the family is refused
        lds64 = int(CC.field(_mul(64, 64, 16, dt, contract=2, contract_tile=64), "lds"))
        d = _mul(64, 64, 16, dt, contract=2, contract_tile=64, max_lds_bytes=lds64 - 1)
        assert CC.family(d) == "reduce_part", d
        d = _mul(64, 64, 4096, dt, contract=2, contract_tile=64, contract_split=4, max_lds_bytes=lds64 - 1)
        assert CC.family(d) == "reduce_part", d


def test_the_table_reaches_every_mechanism_on_every_tile():
    """Per tile and type: a row with one chunk per slice, one with unequal slices, one whose slice starts inside an outer reduced
    index (kc != 0), and -- where the type has a vector -- vector loads past the first slice."""
    for tile in SC.TILES:
        for tn in CC.TYPES:
            rows = [c for c in SPLIT_ROWS if c.name.startswith("%s/t%d/" % (tn, tile))]
            seen = []
            for c in rows:
                kparts, cps, nchunks, nkc, vec = check_slices(c, c.tile, c.S, _es(c.dts))
                seen.append((kparts, cps, nchunks, nkc, vec, c.name))
            assert any(cps == 1 for _, cps, *_ in seen), (tn, tile, "no row with one chunk per slice")
            assert any(kp * cps != nch for kp, cps, nch, *_ in seen), (tn, tile, "no row with unequal slices")
            assert any(nkc > 1 and cps % nkc != 0 and nch > nkc for _, cps, nch, nkc, *_ in seen), (tn, tile, "no slice starts inside a q")
            assert any(kp < c.S for (kp, *_), c in zip(seen, rows)), (tn, tile, "no row whose forced slices are clamped")
            if tn not in ("c64", "mixed", "i32_i64"):  # (16-byte elements are their own vector; converting loads are element loads)
                assert any(vec > 1 and kp > 1 for kp, _, _, _, vec, _ in seen), (tn, tile, "no vector-load row past the first slice")


JIT_PLANS = [(tile, tn, f) for tile in SC.TILES for tn, f in (("f32", "dist"), ("f64", "asym"), ("mixed", "mul"))]


@pytest.mark.parametrize("tile,tn,f", JIT_PLANS, ids=["t%d-%s-%s" % p for p in JIT_PLANS])
def test_the_split_entry_compiles_at_run_time(tile, tn, f):
    tk = CC.tile_numbers(tn, tile)[2]
    kept = (64, 64) if tile == 16 else CC.TILE_SHAPES[tile][0]
    case = CC.Case("jit/%s" % tn, kept + (3 * tk + 1,), CC.MM if tile == 16 else CC.BATCH, CC.TYPES[tn], CC.CONTRACT, f=f)
    with SC.split_options(tile, 2):
        p = case.plan(case.build(), None)
        d = p.describe()
        assert CC.family(d) == "contract" and CC.tile_of(d)[1] == tile and SC.slices(d)[0] == 2, d
        before = [S.get_option(k) for k in ("jit_failures", "jit_compiles", "jit_hits")]
        n = p.jit_compile()
        p.close()
    assert n > 1000, d
    assert S.get_option("jit_failures") == before[0]
    assert S.get_option("jit_compiles") + S.get_option("jit_hits") > before[1] + before[2]


def test_contraction_groups_do_not_read_the_options():
    for name in ("f64/mul/n37/t0", "f32/mul/n3/t32", "c64/dist/n3/t32"):
        row = GC.row(name)
        built = row.build()
        g = row.group(built)
        want = (g.describe(), g.layout())
        with CC.option("contract_split", 4), CC.option("contract_tile", 32):
            g2 = row.group(built)
            got = (g2.describe(), g2.layout())
        assert got == want, name
        assert "kparts=" not in got[0]
