"""The table of tests/window_cases.py, checked without a device: the whole-parent checker reports what it should; the CPU oracle agrees
with NumPy bit for bit on every case and leaves every parent outside the destination view alone; and the table reaches the kernel
variants it is meant to reach, counted from describe() of plans made on the host views (whose roots are 64-byte aligned, so the 16-byte
tests on the bases come out as for device allocations)."""
import collections
import functools

import numpy as np
import pytest

import oraclelib
import strided_jl_amd as S
import window_cases as W


def test_aligned_roots_are_their_own_allocation():
    from util import host_flat
    c = W.build("tiled", 5, np.float32)
    for a in c.arrays:
        flat, shift = host_flat(a)
        assert shift == 0 and flat.ctypes.data == a.parent.ctypes.data and flat.size == a.parent.size and flat.ctypes.data % 64 == 0


def test_pads_include_none_and_an_odd_start_in_the_unit_stride_dim():
    lows, whole = collections.Counter(), 0
    for seed in range(W.SEEDS):
        c = W.build("tiled", seed, np.float32)
        d = c.arrays[0]
        lows[d.offset % 4] += 1
        whole += int(c.inside.all())
        if c.inside.all():
            assert c.inside[0] and c.inside[-1]
    assert whole >= 3 and lows[1] + lows[3] >= 3 and lows[0] >= 3, (whole, lows)


@pytest.mark.parametrize("dt", [np.float32, np.complex128, np.int32])
def test_checker_reports_where_the_first_wrong_element_lies(dt):
    c = W.build("tiled", 5, dt)   # (seed 5: the view starts at an odd element of its parent)
    assert not c.inside.all() and c.inside.any()
    good = c.expected.copy()
    assert c.mismatch(good) is None
    assert c.mismatch(good.view(np.uint8)) is None
    isz = good.dtype.itemsize
    outside, inside = np.flatnonzero(~c.inside), np.flatnonzero(c.inside)
    for e, label in ((int(outside[0]), "outside"), (int(outside[-1]), "outside"), (int(inside[0]), "inside"), (int(inside[-1]), "inside"),
                     (int(inside[len(inside) // 2]), "inside")):
        for byte in (0, isz - 1):
            bad = good.copy()
            bad.view(np.uint8)[e * isz + byte] ^= 0x10
            msg = c.mismatch(bad, "DESCRIBE-TEXT")
            assert msg is not None and msg.startswith("element %d " % e) and "(%s the view)" % label in msg and "DESCRIBE-TEXT" in msg and c.name in msg, msg
            assert "1 of %d elements differ" % good.size in msg, msg
    # an input's poison (NaN; the minimum of an integer type) that reached the view
    src = c.arrays[1]
    stray = src.parent[np.flatnonzero(src.parent != src.parent)[0]] if dt is not np.int32 else src.parent.min()
    assert stray != stray or stray == np.iinfo(np.int32).min
    bad = good.copy()
    e = int(inside[3])
    bad[e] = stray
    msg = c.mismatch(bad)
    assert msg is not None and msg.startswith("element %d " % e) and "(inside the view)" in msg, msg
    # the first of several, and a parent of another size
    bad = good.copy()
    bad[int(inside[5])] = stray
    bad.view(np.uint8)[int(outside[0]) * isz] ^= 1
    first = min(int(inside[5]), int(outside[0]))
    assert c.mismatch(bad).startswith("element %d " % first) and "2 of" in c.mismatch(bad)
    assert "bytes, expected" in c.mismatch(good[:-1])
    # the destination as allocated is not the expected result
    assert c.mismatch(c.before) is not None and "(inside the view)" in c.mismatch(c.before)


@functools.lru_cache(maxsize=None)
def survey(recipe):
    """Every case of a recipe through the CPU oracle: (failures, paths counted from describe(), (functor, type) pairs used)."""
    bad, counts, used = [], W.new_counter(), set()
    for c in W.cases(recipe):
        plan = c.plan()
        c.desc = plan.describe()
        W.count(counts, c.desc)
        used.add((c.fname, np.dtype(c.arrays[0].dtype).name))
        p, keep = S.build_problem(c.f, None, None, c.dims, c.arrays, stream=0)
        oraclelib.mapreduce(p, 4)
        msg = c.mismatch(c.arrays[0].parent) or c.inputs_changed({a.parent.ctypes.data: a.parent for a in c.arrays[1:]})
        if msg:
            bad.append(msg)
        plan.close()
    return bad, counts, used


@pytest.mark.parametrize("recipe", sorted(W.RECIPES))
def test_oracle_agrees_with_numpy_bit_for_bit_and_leaves_the_padding_alone(recipe):
    bad, counts, used = survey(recipe)
    print("[window cases] %s: %s" % (recipe, ", ".join("%s x%d" % kv for kv in sorted(counts.items()))))
    assert not bad, "%d cases differ, the first: %s" % (len(bad), bad[0])


def test_every_functor_is_used_with_every_type_it_is_defined_for():
    used = set()
    for recipe in W.RECIPES:
        used |= survey(recipe)[2]
    want = {(name, np.dtype(dt).name) for dt in W.FLOATS + W.INTS for name, _, _, _ in W.functors_for(dt)}
    assert want <= used, sorted(want - used)


def test_the_table_reaches_every_path_often_enough():
    # W.MINIMUMS: every family 24 times, every special path 8 times.  Not reachable by a small windowed shape and so not among them:
    # TILED's persistent form (` pipe`), which starts at 32 rounds of 4 workgroups per CU -- 32768 tiles, 32 Mi elements.
    counts = W.new_counter()
    for recipe in W.RECIPES:
        counts.update(survey(recipe)[1])
    print("[window cases] total: " + ", ".join("%s x%d" % kv for kv in sorted(counts.items())))
    W.check_minimums(counts)


def test_describe_names_the_tiled_variant():
    """vec, element alignment, MODE, wide offsets: the tokens stand in front of algbytes=, the older ones stay."""
    seen = set()
    for seed, dt in ((0, np.float32), (5, np.float32), (2, np.float64), (4, np.float32), (9, np.complex128)):
        for recipe in ("tiled", "tiled_reversed"):
            d = W.build(recipe, seed, dt).plan().describe()
            if W.family(d) != "tiled":
                continue
            toks = d.split()
            i = [k for k, t in enumerate(toks) if t.startswith("vec=")][0]
            assert toks[i + 1].startswith("mode=") and toks[-1].startswith("algbytes=") and "family=tiled ct=" in d and " threads=" in d, d
            assert toks[i] in ("vec=1", "vec=2", "vec=4", "vec=2(element-aligned)", "vec=4(element-aligned)"), d
            assert toks[i + 1] in ("mode=0", "mode=1", "mode=2", "mode=7", "mode=9"), d
            assert toks[i + 2:-1] in ([], ["wide"], ["pipe"], ["wide", "pipe"]) or toks[i + 2].startswith("int_wraps="), d
            if toks[i + 1] == "mode=9":
                assert toks[i] != "vec=1", d   # partial vectors exist in the vector variants only
            seen.add((toks[i], toks[i + 1]))
    assert len(seen) >= 3, seen
