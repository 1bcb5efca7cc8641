"""Groups recorded in sequences, host side (no device): smr_seq_add_group, the footprint of a group item (the merged bounding byte
ranges of its members' operands: reads = every input, writes = every destination) and what the dependency and fence analyses
(smr_seq_components, smr_seq_fences) make of sequences that mix plan items and group items.  All of it is host arithmetic."""
import ctypes as C

import numpy as np

import strided_jl_amd as S
from strided_jl_amd import _lib as L

SHAPE = (6, 5)
NBYTES = 6 * 5 * 8  # one Float64 array of SHAPE


def ident(x):
    return x


def fresh(shape=SHAPE):
    return S.StridedView(np.zeros(shape, order="F"))


def copy_plan(dst, src):
    return S.make_plan(ident, None, None, dst.size, (dst, src))


def group_of(pairs, independent=False):
    """A group of copies dst <- src, one member per (dst, src) pair."""
    built = [S.build_problem(ident, None, None, d.size, (d, s), stream=0) for d, s in pairs]
    return L.Group([b[0] for b in built], independent, keepalive=(built, pairs))


def four_copies():
    A = [fresh() for _ in range(4)]
    B = [fresh() for _ in range(4)]
    return A, B, group_of(list(zip(B, A)))


def test_add_group_returns_the_sequence_and_refuses_null():
    _, _, g = four_copies()
    q = S.Sequence()
    assert q.add_group(g) is q
    assert q.components() == [0]
    lib = L.load()
    assert lib.smr_seq_add_group(None, g._h) == L.SMR_EINVAL
    assert lib.smr_seq_add_group(q._h, None) == L.SMR_EINVAL
    assert q.components() == [0]  # nothing was added by the refused calls


def test_a_plan_reading_a_member_destination_joins_the_group():
    A, B, g = four_copies()
    Cc = fresh()
    assert S.Sequence().add_group(g).add(copy_plan(Cc, B[1])).components() == [0, 0]
    acq, fp, resident = S.Sequence().add_group(g).add(copy_plan(Cc, B[1])).fences()
    assert acq == [0, 1] and resident    # the plan reads what the group writes; nobody writes the group's inputs
    assert fp == 9 * NBYTES              # A1..A4, B1..B4 and C, once each


def test_a_plan_on_unrelated_arrays_is_a_component_of_its_own():
    _, _, g = four_copies()
    X, Y = fresh(), fresh()
    q = S.Sequence().add_group(g).add(copy_plan(Y, X))
    assert q.components() == [0, 1]
    assert q.fences()[0] == [0, 0]


def test_a_plan_writing_a_member_input_orders_the_group_behind_it():
    A, _, g = four_copies()
    X = fresh()
    q = S.Sequence().add(copy_plan(A[2], X)).add_group(g)
    assert q.components() == [0, 0]
    assert q.fences()[0] == [0, 1]       # the group item acquires: it reads bytes the sequence writes


def test_two_groups_on_disjoint_arrays_are_two_components():
    _, _, g1 = four_copies()
    _, _, g2 = four_copies()
    q = S.Sequence().add_group(g1).add_group(g2)
    assert q.components() == [0, 1]
    assert q.fences()[1] == 16 * NBYTES
    # the same group twice conflicts with itself (both executions write B1..B4)
    assert S.Sequence().add_group(g1).add_group(g1).components() == [0, 0]
    # a group reading what another one writes
    A, B, _ = four_copies()
    D = [fresh() for _ in range(2)]
    first, second = group_of(list(zip(B[:2], A[:2]))), group_of(list(zip(D, B[:2])))
    q = S.Sequence().add_group(first).add_group(second)
    assert q.components() == [0, 0] and q.fences()[0] == [0, 1]


def test_independent_group_keeps_its_conservative_ranges():
    """Even and odd columns of one 8 x 8 parent copied into those of another: created with SMR_GROUP_INDEPENDENT, where the byte-range
    check is skipped -- the footprint is computed all the same."""
    src, dst = fresh((8, 8)), fresh((8, 8))
    pairs = [(dst.sview(slice(None), slice(k, None, 2)), src.sview(slice(None), slice(k, None, 2))) for k in (0, 1)]
    g = group_of(pairs, independent=True)
    # even columns span elements 0..55, odd columns 8..63: together each parent once, 64 elements of 8 bytes
    acq, fp, _ = S.Sequence().add_group(g).fences()
    assert acq == [0] and fp == 2 * 64 * 8
    other = fresh((8, 1))
    reads_dst = copy_plan(other, dst.sview(slice(None), slice(7, 8)))       # column 7 of the destination parent
    writes_src = copy_plan(src.sview(slice(None), slice(0, 1)), other)      # column 0 of the source parent
    unrelated = copy_plan(fresh((8, 1)), fresh((8, 1)))
    assert S.Sequence().add_group(g).add(reads_dst).components() == [0, 0]
    assert S.Sequence().add_group(g).add(reads_dst).fences()[0] == [0, 1]
    assert S.Sequence().add(writes_src).add_group(g).components() == [0, 0]
    assert S.Sequence().add(writes_src).add_group(g).fences()[0] == [0, 1]
    assert S.Sequence().add_group(g).add(unrelated).components() == [0, 1]
    # a member's bounding range covers the columns BETWEEN its own: a plan that writes only column 1 of the destination parent
    # (elements 8..15, no element of the even member) still joins a group of the even member alone
    even = group_of(pairs[:1], independent=True)
    col1 = copy_plan(dst.sview(slice(None), slice(1, 2)), other)
    assert S.Sequence().add_group(even).add(col1).components() == [0, 0]
    assert S.Sequence().add_group(even).fences()[1] == 2 * 56 * 8


def test_footprint_is_the_union_of_the_merged_ranges():
    """Inputs that overlap, destinations that touch: pool[0:100] -> out[0:100] and pool[50:150] -> out[100:200] (Float64)."""
    pool, out = np.zeros(1000), np.zeros(1000)

    def vec(a, lo, n):
        return S.StridedView(a, (n,), (1,), lo)

    g = group_of([(vec(out, 0, 100), vec(pool, 0, 100)), (vec(out, 100, 100), vec(pool, 50, 100))])
    acq, fp, resident = S.Sequence().add_group(g).fences()
    assert acq == [0] and resident
    assert fp == 150 * 8 + 200 * 8       # pool[0:150] read once, out[0:200] written
    # a plan inside the merged ranges adds nothing, one next to them adds its own bytes
    inside = copy_plan(vec(out, 150, 10), vec(pool, 20, 10))
    beside = copy_plan(vec(out, 500, 10), vec(pool, 500, 10))
    assert S.Sequence().add_group(g).add(inside).fences()[1] == fp
    assert S.Sequence().add_group(g).add(inside).components() == [0, 0]
    assert S.Sequence().add_group(g).add(beside).fences()[1] == fp + 2 * 10 * 8
    assert S.Sequence().add_group(g).add(beside).components() == [0, 1]
    # the gap between out[200:] and the group's writes is respected: out[200:210] is written by nobody in the group
    after = copy_plan(vec(out, 200, 10), vec(pool, 600, 10))
    assert S.Sequence().add_group(g).add(after).components() == [0, 1]


def test_mixed_items_have_one_entry_each_in_order():
    A, B, g1 = four_copies()
    _, _, g2 = four_copies()
    X, Y, Z = fresh(), fresh(), fresh()
    q = S.Sequence().add(copy_plan(Y, X)).add_group(g1).add(copy_plan(Z, B[3])).add_group(g2).add(copy_plan(X, Z)).add_group(g1)
    # plan X->Y | g1 | plan B4->Z (joins g1) | g2 alone | plan Z->X (writes what item 0 reads, reads what item 2 wrote) | g1 again
    assert q.components() == [0, 0, 0, 1, 0, 0]
    acq, fp, _ = q.fences()
    assert acq == [1, 0, 1, 0, 1, 0]
    assert fp == (8 + 8 + 3) * NBYTES
    arr = (C.c_int32 * 6)()
    assert L.load().smr_seq_components(q._h, arr, 6) == 2 and list(arr) == [0, 0, 0, 1, 0, 0]
