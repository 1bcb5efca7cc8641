"""CPU: the replay scheduler of recorded sequences (csrc/smr_sched.cpp: schedule()) on synthetic executions, through the host-only
entry smr_debug_seq_schedule.  This is the function smr_seq.cpp builds its packets from: which hardware queue an execution goes to,
which launch is cut into block ranges, which packets carry the barrier bit and which acquire.  Every expected value below is derived
from the scheduler's rules, stated next to it."""
import ctypes as C

import strided_jl_amd as S

U = 1 << 20  # bytes of one buffer of the synthetic steps


def ex(rd, wr, nlaunch=1, grid=4096, sliceable=True, all_self=False, same_as=None):
    return dict(rd=rd, wr=wr, nlaunch=nlaunch, grid=grid, sliceable=sliceable, all_self=all_self, same_as=same_as)


def sched(execs, max_queues=4, slices=-1, all_ordered=False, max_total=128 << 20, comp_slices=()):
    lib = S._lib.load()
    f = lib.smr_debug_seq_schedule
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int]
    n = len(execs)
    nspans, spans, launches = [], [], []
    for i, e in enumerate(execs):
        nspans += [len(e["rd"]), len(e["wr"])]
        for lo, hi in list(e["rd"]) + list(e["wr"]):
            spans += [lo, hi]
        launches += [e["nlaunch"], e["grid"], int(e["sliceable"]), int(e["all_self"]), i if e["same_as"] is None else e["same_as"]]
    cs = [v for pair in comp_slices for v in pair]
    knobs = [max_queues, slices, int(all_ordered), max_total, len(comp_slices)]
    per = (C.c_int32 * (4 * max(1, n)))()
    tot = (C.c_int32 * 4)()
    fp = C.c_int64(0)
    cap = 256
    pk = (C.c_int32 * (8 * cap))()
    npk = f(n, (C.c_int32 * max(1, len(nspans)))(*nspans), (C.c_int64 * max(1, len(spans)))(*spans), (C.c_int32 * max(1, len(launches)))(*launches),
            (C.c_int64 * 5)(*knobs), (C.c_int32 * max(1, len(cs)))(*cs), per, tot, C.byref(fp), pk, cap)
    assert 0 <= npk <= cap
    rows = [tuple(pk[8 * r:8 * r + 8]) for r in range(npk)]
    queues = {}
    for q, *rest in rows:  # (exec, launch, slice, lo, hi, barrier, acquire) per queue, in submission order
        queues.setdefault(q, []).append(tuple(rest))
    cols = [[per[4 * i + c] for i in range(n)] for c in range(4)]
    return dict(comp=cols[0], acquire=cols[1], queue=cols[2], nslices=cols[3], ncomp=tot[0], nsliced=tot[1], nq=tot[2], resident=bool(tot[3]),
                footprint=fp.value, queues=queues)


def span(k, n=1):  # buffer number k, n units long
    return (k * 64 * U, k * 64 * U + n * U)


def bench_step(**kw):
    # execution 0 reads U and writes V (2u bytes); execution 1 reads U through four views and writes W (5u bytes: every view counts)
    u, v, w = span(0), span(1), span(2)
    return [ex([u], [v], **kw), ex([u, u, u, u], [w], **kw)]


def test_bench_step_default_knobs():
    r = sched(bench_step())
    # nobody writes U: two components, nothing acquires; the footprint counts U once
    assert r["comp"] == [0, 1] and r["ncomp"] == 2 and r["acquire"] == [0, 0] and r["footprint"] == 3 * U and r["resident"]
    # 2 + 1 <= min(4, 3) queues and 5u * 2 >= 2u * 3: the heavy component (1) is cut in two; sliced components take their queues
    # first (0 and 1), the whole one gets the next (2)
    assert r["nslices"] == [1, 2] and r["nsliced"] == 1 and r["nq"] == 3 and r["queue"] == [2, 0]
    # grid 4096 in two: 2048 each.  Every queue holds one execution, which conflicts with itself across replays (it rewrites its
    # destination): every packet carries the barrier bit; no packet acquires
    assert r["queues"] == {0: [(1, 0, 0, 0, 2048, 1, 0)], 1: [(1, 0, 1, 2048, 4096, 1, 0)], 2: [(0, 0, 0, 0, 4096, 1, 0)]}


def test_bench_step_all_self_released():
    r = sched(bench_step(all_self=True))
    # a further packet costs no write-back: both components are cut, 2 + 2 <= min(4, 4); queues in component order
    assert r["nslices"] == [2, 2] and r["nsliced"] == 2 and r["nq"] == 4 and r["queue"] == [0, 2]
    assert r["queues"] == {0: [(0, 0, 0, 0, 2048, 1, 0)], 1: [(0, 0, 1, 2048, 4096, 1, 0)],
                           2: [(1, 0, 0, 0, 2048, 1, 0)], 3: [(1, 0, 1, 2048, 4096, 1, 0)]}


def test_bench_step_one_queue():
    r = sched(bench_step(), max_queues=1)
    # no queue to spare: nothing is cut, recorded order on queue 0.  Steady state (second simulated replay): execution 0 rewrites V,
    # which is in the window left by the previous replay -> ordered; execution 1 shares nothing written with execution 0 -> unordered
    assert r["nslices"] == [1, 1] and r["nsliced"] == 0 and r["nq"] == 1 and r["ncomp"] == 2
    assert r["queues"] == {0: [(0, 0, 0, 0, 4096, 1, 0), (1, 0, 0, 0, 4096, 0, 0)]}
    # "order" = 0: the barrier bit everywhere
    r = sched(bench_step(), max_queues=1, all_ordered=True)
    assert [p[5] for p in r["queues"][0]] == [1, 1]
    # a second launch of one execution (a folding pass) depends on the first and reads its partials: barrier and acquire, although
    # the execution's own ranges ask for neither
    steps = bench_step()
    steps[1]["nlaunch"] = 2
    r = sched(steps, max_queues=1)
    assert r["queues"][0] == [(0, 0, 0, 0, 4096, 1, 0), (1, 0, 0, 0, 4096, 0, 0), (1, 1, 0, 0, 0, 1, 1)]


def test_bench_step_never_sliced():
    r = sched(bench_step(), slices=1)
    # one queue per component; the heavier component is placed first (longest processing time first)
    assert r["nslices"] == [1, 1] and r["nq"] == 2 and r["queue"] == [1, 0]


def ranges(grid, ns):
    r = sched([ex([span(0)], [span(1)], grid=grid)], slices=ns, max_queues=8)
    return [(p[3], p[4]) for q in sorted(r["queues"]) for p in r["queues"][q]]


def test_slice_range_cuts_at_multiples_of_8():
    # per slice: ceil(grid / ns) rounded up to a multiple of 8 (a slice that starts at a multiple of 8 keeps its workgroups' XCDs)
    assert ranges(1000, 2) == [(0, 504), (504, 1000)]
    assert ranges(130, 2) == [(0, 72), (72, 130)]
    assert ranges(200, 3) == [(0, 72), (72, 144), (144, 200)]
    assert ranges(256, 4) == [(0, 64), (64, 128), (128, 192), (192, 256)]
    assert ranges(127, 2) == [(0, 127)]  # below 64 workgroups per slice: not cut


def test_a_component_of_several_executions_is_cut_only_when_they_are_one_execution_repeated():
    a, b, c = span(0), span(1), span(2)
    same = sched([ex([a], [b]), ex([a], [b], same_as=0)], slices=2)
    assert same["comp"] == [0, 0] and same["nslices"] == [2, 2] and same["nq"] == 2
    # slice k of the second follows slice k of the first on queue k
    assert [[p[:3] for p in same["queues"][k]] for k in (0, 1)] == [[(0, 0, 0), (1, 0, 0)], [(0, 0, 1), (1, 0, 1)]]
    other = sched([ex([a], [b]), ex([c], [b])], slices=2)  # two different plans that write one buffer
    assert other["comp"] == [0, 0] and other["nslices"] == [1, 1] and other["nq"] == 1
    grids = sched([ex([a], [b]), ex([a], [b], same_as=0, grid=2048)], slices=2)
    assert grids["nslices"] == [1, 1]


def test_nothing_is_cut_unless_every_component_keeps_a_queue():
    steps = [ex([span(0)], [span(k)]) for k in (1, 2, 3)]
    r = sched(steps, slices=2, max_queues=4)  # 3 components x 2 slices = 6 queues > 4
    assert r["ncomp"] == 3 and r["nslices"] == [1, 1, 1] and r["nsliced"] == 0 and r["nq"] == 3 and sorted(r["queue"]) == [0, 1, 2]


def test_unsliced_components_are_placed_longest_first():
    sizes = [1, 5, 9, 3, 7]  # recorded order; each execution writes a buffer of its own
    r = sched([ex([], [span(k, n)], sliceable=False) for k, n in enumerate(sizes)], max_queues=2)
    # 9 -> queue 0, 7 -> queue 1, 5 -> queue 1 (7 < 9), 3 -> queue 0 (9 < 12), 1 -> queue 0 (12 = 12: the first): 9+3+1 | 7+5
    assert r["nq"] == 2 and r["queue"] == [0, 1, 0, 0, 1]
    assert [p[0] for p in r["queues"][0]] == [0, 2, 3] and [p[0] for p in r["queues"][1]] == [1, 4]  # recorded order inside a queue


def test_acquire_flags_follow_read_after_write():
    a, b, c = span(0), span(1), span(2)
    r = sched([ex([a], [b]), ex([b], [c]), ex([c], [c])])  # A -> B, B -> C, C in place
    assert r["acquire"] == [0, 1, 1] and r["comp"] == [0, 0, 0]
    assert [p[6] for p in r["queues"][0]] == [0, 1, 1]


def test_footprint_counts_bytes_once_and_cache_residency_flips_at_the_limit():
    steps = [ex([(0, 100), (50, 150)], [(60, 70)]), ex([(200, 300)], [(250, 260)])]  # overlapping, nested, disjoint
    assert sched(steps)["footprint"] == 250
    assert sched(steps, max_total=250)["resident"] and not sched(steps, max_total=249)["resident"]
