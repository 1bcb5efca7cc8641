"""The table of tests/reduce_fuzz_cases.py, checked without a device: every case through the CPU oracle with 1 and 4 threads must give
exactly the expected bits after one application and after three and leave the destination's parent alone around its elements; the
exactness bound the table relies on is recomputed from every case's data; the whole-parent checker reports each kind of wrong result;
and the kernel paths the table reaches are counted from describe() of plans made on the host (64-byte aligned parents, like device
allocations) and asserted per cell.  This proves the table and its semantics before any GPU time is spent on test_gpu_reduce_fuzz.py."""
import collections
import functools

import numpy as np
import pytest

import oraclelib
import reduce_fuzz_cases as RF
import strided_jl_amd as S

from reduce_fuzz_cases import F, GROUPS, host_describe, with_options


@functools.lru_cache(maxsize=None)
def survey(recipe, t):
    """every case of a group through the oracle: (failures, [(case name, type, describe, cells)], exactness bounds)"""
    bad, plans, bounds = [], [], []
    for case in RF.cases(recipe, t):
        for nthreads in case.threads:
            for times in (1, RF.APPLICATIONS):
                arrs = RF.views(case, S)
                p, keep = S.build_problem(F[case.f], case.op, case.initop, case.dims, arrs, stream=0)
                for _ in range(times):
                    oraclelib.mapreduce(p, nthreads)
                err = case.mismatch(arrs[0].parent, times)
                if err:
                    bad.append("oracle, %d threads, %d applications: %s" % (nthreads, times, err))
        d = host_describe(case)
        plans.append((case.name, t, d, RF.cells(d, case)))
        b = RF.bound(case)
        if b is not None:
            bounds.append((case.name,) + b)
        if case.op == "*" and not RF.is_int(t):
            xs = RF.seen_values(case)
            v = xs[0] if case.f == "ident" else xs[0] * xs[1]
            rows = RF.to_rows(np.abs(v), case.rdims)
            assert set(np.unique(rows)) <= {0.25, 0.5, 1.0, 2.0, 4.0}, case.name
            e = np.log2(rows)
            bounds.append((case.name + " (twos)", int(np.where(e > 0, e, 0).sum(axis=1).max()), 17))
            bounds.append((case.name + " (halves)", int(np.where(e < 0, -e, 0).sum(axis=1).max()), 17))
        if case.op in ("min", "max") and not RF.is_int(t):
            for x in RF.seen_values(case):
                fin = x[np.isfinite(x)]
                assert np.array_equal(fin, np.rint(fin)) and (np.abs(fin) < 4096).all(), case.name   # (f of them stays below 2^24)
    return bad, plans, bounds


@pytest.mark.parametrize("recipe,t", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_oracle_gives_the_expected_bits_after_one_and_three_applications(recipe, t):
    bad, plans, bounds = survey(recipe, t)
    assert not bad, "%d of %d runs differ, the first: %s" % (len(bad), 4 * len(plans), bad[0])


@pytest.mark.parametrize("recipe,t", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_every_partial_result_is_exactly_representable(recipe, t):
    """from the data: three applications of the sum of magnitudes plus the destination stay below 2^24 / 2^53; at most 16 twos and 16 halves
    per output of a product"""
    bad, plans, bounds = survey(recipe, t)
    for name, reached, limit in bounds:
        assert reached < limit, (name, reached, limit)


def test_the_table_has_the_size_the_gpu_test_must_run():
    n = RF.table_size()
    assert 700 <= n <= 1000 and n == sum(1 for r, t in GROUPS for _ in RF.seeds(r, t)), n


def test_cases_are_pure_functions_of_recipe_seed_and_type():
    a, b = RF.build("row", 5, "c32"), RF.build("row", 5, "c32")
    assert a.dims == b.dims and a.op == b.op and a.initop == b.initop and np.array_equal(a.dest.parent.view(np.uint8), b.dest.parent.view(np.uint8))
    assert all(np.array_equal(x.parent.view(np.uint8), y.parent.view(np.uint8)) for x, y in zip(a.ins, b.ins))
    assert all(o.parent.ctypes.data % 64 == 0 for o in a.ins + [a.dest])


# ---- the checker -------------------------------------------------------------------------------------------------------------------
def _ulp_off(parent, e):
    """element e of `parent` moved by one unit in the last place (of its real part)"""
    dt = parent.dtype
    out = parent.copy()
    if dt.kind == "c":
        r = out.view(np.float32 if dt.itemsize == 8 else np.float64)
        r[2 * e] = np.nextafter(r[2 * e], np.inf)
    elif dt.kind == "f":
        out[e] = np.nextafter(out[e], dt.type(np.inf))
    else:
        out[e] += 1
    return out


@pytest.mark.parametrize("recipe,seed,t", [("row", 0, "f32"), ("col", 2, "c32"), ("all", 1, "f64"), ("general", 1, "i64"), ("split", 1, "c64"), ("row", 7, "f32")])
def test_checker_reports_every_mutation(recipe, seed, t):
    case = RF.build(recipe, seed, t)
    if case.op != "+":   # the dropped addend needs a sum: the next seed that has one
        case = next(c for c in (RF.build(recipe, s, t) for s in range(seed, RF.SEEDS)) if c.op == "+")
    for times in (1, 2, 3):
        good = case.expected_parent(times)
        assert case.mismatch(good, times) is None
        idx = RF._index(case.dest.offset, case.oshape, case._ostrides()).ravel()
        inside = np.zeros(good.size, dtype=bool)
        inside[idx] = True
        e = int(idx[len(idx) // 2])
        # one element off by one unit in the last place
        msg = case.mismatch(_ulp_off(good, e), times)
        assert msg is not None and "parent index [%d]" % e in msg, msg
        # one addend dropped: every addend is a nonzero integer, so the element moves by at least one
        xs = RF.seen_values(case)
        full = [tuple(np.broadcast_to(c, case.dims) for c in x) if RF.is_cx(t) else np.broadcast_to(x, case.dims) for x in xs]
        fv = RF.apply_f(case.f, full, t)
        first = (RF.to_rows(fv[0], case.rdims)[len(idx) // 2, 0] + 1j * RF.to_rows(fv[1], case.rdims)[len(idx) // 2, 0]) if RF.is_cx(t) else RF.to_rows(fv, case.rdims)[len(idx) // 2, 0]
        dropped = good.copy()
        tgt = int(rows_to_parent_index(case)[len(idx) // 2])
        with np.errstate(over="ignore"):
            dropped[tgt] = dropped[tgt] - (np.conj(first) if case.dest.conj else first)
        if first != 0:
            msg = case.mismatch(dropped, times)
            assert msg is not None and "parent index [%d]" % tgt in msg, msg
        # one byte changed outside the destination
        outside = np.flatnonzero(~inside)
        if outside.size:
            for x in (int(outside[0]), int(outside[-1])):
                b = good.copy()
                b.view(np.uint8)[x * good.itemsize] ^= 0x01
                msg = case.mismatch(b, times)
                assert msg is not None and "outside the destination" in msg, msg
        # NaN where a number is due
        if good.dtype.kind in "fc":
            b = good.copy()
            b[e] = np.nan
            msg = case.mismatch(b, times)
            assert msg is not None and "parent index [%d]" % e in msg, msg
    # the destination as allocated, and the result of one application where three are due
    assert case.mismatch(case.dest.parent) is not None
    if case.initop not in ("zero",) and not (isinstance(case.initop, tuple) and case.initop[0] == "const"):
        assert case.mismatch(case.expected_parent(1), 3) is not None


def rows_to_parent_index(case):
    """parent index of every destination element, in the order of reduce_fuzz_cases.to_rows"""
    idx = RF._index(case.dest.offset, case.oshape, case._ostrides())
    return RF.to_rows(np.broadcast_to(idx, case.oshape), case.rdims)[:, 0]


def test_checker_wants_a_nan_where_the_table_has_one():
    case = next(c for c in (RF.build("row", s, "f64") for s in range(200)) if "plant=nan" in c.note)
    good = case.expected_parent()
    assert np.isnan(good[RF._index(case.dest.offset, case.oshape, case._ostrides())]).any()
    assert case.mismatch(good) is None
    bad = good.copy()
    nanpos = np.flatnonzero(np.isnan(good))
    bad[nanpos[0]] = 1.0
    assert "expected NaN" in case.mismatch(bad)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_every_cell_is_reached_often_enough():
    reached, exact_tx, fam = collections.defaultdict(list), set(), collections.Counter()
    for recipe, t in GROUPS:
        for name, typ, d, cells in survey(recipe, t)[1]:
            fam[RF.token(d, "family") + ("/" + RF.token(d, "form") if RF.token(d, "form") else "")] += 1
            for c in cells:
                reached[c].append(typ)
            if "col:exact" in cells:
                exact_tx.add(RF.token(d, "tx").split("(")[0])
    print("[reduce fuzz] families: " + ", ".join("%s x%d" % kv for kv in sorted(fam.items())))
    print("[reduce fuzz] cells: " + ", ".join("%s x%d/%d types" % (c, len(v), len(set(v))) for c, v in sorted(reached.items())))
    print("[reduce fuzz] exact lane maps, TX: " + " ".join(sorted(exact_tx, key=int)))
    RF.check_cells(reached, exact_tx)


def test_split_cases_reach_their_fold_form_under_default_options():
    """at least a third of the split recipe folds as the library decides by itself"""
    n = default = 0
    for t in RF.TYPES:
        for case in RF.cases("split", t):
            n += 1
            default += "reduce_single" not in case.options
    assert 3 * default >= n, (default, n)


NEGZERO_PATHS = {"all:epilogue": ("family=reduce_all", "fold=epilogue"), "all:in-launch": ("family=reduce_all", "fold=in-launch"),
                 "all:second-launch": ("family=reduce_all", "fold=second-launch"), "row": ("form=row", "split=1 "), "row:split": ("form=row", "fold=in-launch"),
                 "row:split:empty": ("form=row", "fold=second-launch"), "col": ("form=col", "split=1 "), "col:split": ("form=col",),
                 "general": ("form=general", "split=1 "), "general:split": ("form=general",), "accumulate": ("form=general", "split=1 ")}


def test_negzero_cases_cover_every_form_with_and_without_a_split():
    for t in RF.FLOATS:
        for seed in RF.seeds("negzero", t):
            case = RF.build("negzero", seed, t)
            form = case.note.split(":  every")[0].split(": every")[0]
            d = host_describe(case) + " "
            for s in NEGZERO_PATHS[form]:
                assert s in d, (case.name, form, s, d)
            if form.endswith(":split") or form.endswith(":empty"):
                assert RF.token(d, "split") != "1", (case.name, d)
            if form.endswith(":empty"):
                assert RF.empty_chunks(d), (case.name, d)
            assert case.threads == (1,) and "1-thread oracle only" in case.note
            neg = np.signbit(case.expected_parent().view(np.float32 if np.dtype(case.dest.dtype).itemsize in (4, 8) and t in ("f32", "c32") else np.float64)[
                RF._index(case.dest.offset, case.oshape, case._ostrides()).ravel() * (2 if RF.is_cx(t) else 1)])
            assert neg.all() if case.initop is None else not neg.any(), case.name
