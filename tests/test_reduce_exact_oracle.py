"""CPU check of the bit-exact reduction table (reduce_exact_cases.py): every case through the CPU oracle with 1 and 4
threads must give exactly the expected bits and leave the destination's parent untouched around its elements, and the
planner must put every case on the kernel path named in the table (describe(), host-only planning).  This proves the
table and its semantics -- initop, conjugated and strided destinations, MIXED typing, signed zeros, NaN and Inf --
before any GPU time is spent on test_gpu_reduce_exact.py."""
import numpy as np
import pytest

import oraclelib
import reduce_exact_cases as RC
import strided_jl_amd as S
from strided_jl_amd import _lib as L

TABLE = RC.table()

F = {"ident": lambda x: x, "abs2": S.fn.abs2, "mul": lambda x, y: x * y, "prog": lambda x, y: 2 * x - y + 1}


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


def views(case, wrap=lambda a: a):
    """(destination, inputs...) as StridedViews over the case's parents (wrapped by `wrap`: NumPy here, torch on the GPU)."""
    d = case.dest
    dest = S.StridedView(wrap(d.parent.copy()), case.dims, case._ostrides(), d.offset, "conj" if d.conj else "identity")
    ins = tuple(S.StridedView(wrap(o.parent.copy()), case.dims, o.strides, o.offset) for o in case.ins)
    return (dest,) + ins


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_case_on_the_oracle(name, option):
    case = TABLE[name]()
    for k, v in case.options.items():
        option(k, v)
    for nthreads in (1, 4):
        arrs = views(case)
        p, keep = S.build_problem(F[case.f], case.op, case.initop, case.dims, arrs, stream=0)
        oraclelib.mapreduce(p, nthreads)
        err = case.mismatch(arrs[0].parent)
        assert err is None, f"oracle, {nthreads} threads: {err}"
    d = S.make_plan(F[case.f], case.op, case.initop, case.dims, views(case)).describe()
    for s in case.expect:
        assert s in d + " ", (name, s, d)


def test_table_is_exact_by_construction():
    """The bounds the table relies on: sums of magnitudes below 2^24 (32-bit types) / 2^53 (64-bit), and the MIXED case
    really needs Float64 accumulation."""
    for name, build in TABLE.items():
        if not name.startswith(("all_1000", "all_4100", "all_capped", "all_mixed", "col_exact_split", "row_second64")):
            continue
        case = build()
        for o in case.ins:
            v = o.parent[RC._index(o.offset, case.dims, o.strides)]
            mag = np.abs(v.real.astype(np.float64)).sum() + np.abs(v.imag.astype(np.float64)).sum()
            lim = 2.0 ** 24 if np.dtype(case.dest.dtype).itemsize // (2 if np.dtype(case.dest.dtype).kind == "c" else 1) == 4 else 2.0 ** 53
            assert mag < lim, (name, mag)
    mixed = TABLE["all_mixed_f32_to_f64"]()
    total = int(mixed.want.ravel()[0])
    assert total > 2 ** 24 and total % 2 == 1 and float(np.float32(total)) != total


def test_every_cell_is_in_the_table():
    cells = {build().cell for build in TABLE.values()}
    assert set(RC.CELLS) <= cells, sorted(set(RC.CELLS) - cells)
