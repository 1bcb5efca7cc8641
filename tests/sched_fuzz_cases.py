"""Synthetic execution lists for the replay scheduler (csrc/smr_sched.cpp), as pure functions of (recipe, seed): what
tests/test_seq_schedule_fuzz.py runs and tools/seq_schedule_search.py searches.  No torch, no device, no library.

  wide(seed)    1-8 executions over 2-7 base buffers with whole, nested, partially overlapping and adjacent sub-ranges, up to four
                reads each, one or two launches, six grids, sliceable / all_self / same_as drawn (a repeat copies an earlier
                execution), every knob drawn.
  chains(seed)  one queue, 4-7 executions over 3-6 whole buffers, one or two reads and one write each: long dependency chains whose
                barrier bits depend on what the previous replay left in the queue.

Both return (execs, knobs): the dicts of test_seq_schedule.ex() and the keyword arguments of test_seq_schedule.sched()."""
import numpy as np

U = 1 << 20          # bytes of one base buffer
GRIDS = (8, 64, 127, 130, 1000, 4096)
# sub-ranges of a base buffer in quarters: whole, halves (adjacent), the middle (overlaps both halves), nested quarters
PARTS = ((0, 4), (0, 4), (0, 4), (0, 2), (2, 4), (1, 3), (1, 2), (0, 1), (3, 4))


def span(k, part=(0, 4)):
    base = k * 64 * U
    return (base + part[0] * (U // 4), base + part[1] * (U // 4))


def ex(rd, wr, nlaunch=1, grid=4096, sliceable=True, all_self=False, same_as=None):
    return dict(rd=list(rd), wr=list(wr), nlaunch=nlaunch, grid=grid, sliceable=sliceable, all_self=all_self, same_as=same_as)


def _pick(rng, xs):
    return xs[int(rng.integers(0, len(xs)))]


def wide(seed):
    rng = np.random.default_rng([1, seed])
    n = int(rng.integers(1, 9))
    nb = int(rng.integers(2, 8))
    # a third of the lists keep every execution to buffers of its own half, so that several components are common
    split = rng.integers(0, 3) == 0
    free_parts = rng.integers(0, 2) == 0
    all_self = bool(rng.integers(0, 4) == 0)
    one_launch = rng.integers(0, 2) == 0
    execs = []
    for i in range(n):
        if i and rng.integers(0, 4) == 0:   # a repeat: the same ranges; the same plan and pointers (same_as) two times in three
            j = int(rng.integers(0, i))
            e = dict(execs[j], rd=list(execs[j]["rd"]), wr=list(execs[j]["wr"]))
            first = j if execs[j]["same_as"] is None else execs[j]["same_as"]
            if rng.integers(0, 3):
                e["same_as"] = first
            else:
                e.update(same_as=None, grid=_pick(rng, GRIDS), sliceable=bool(rng.integers(0, 2)))
            execs.append(e)
            continue
        mine = [k for k in range(nb) if not split or k % 2 == i % 2] or [0]
        part = lambda: _pick(rng, PARTS) if free_parts else (0, 4)  # noqa: E731
        rd = [span(_pick(rng, mine), part()) for _ in range(int(rng.integers(0, 5)))]
        wr = [span(_pick(rng, mine), part())]
        if split and rng.integers(0, 2):    # many small components: an execution of its own buffer
            rd, wr = [], [span(8 + i)]
        execs.append(ex(rd, wr, nlaunch=1 if one_launch or rng.integers(0, 3) else 2, grid=_pick(rng, GRIDS), sliceable=bool(rng.integers(0, 4)),
                        all_self=all_self or bool(rng.integers(0, 2))))
    knobs = dict(max_queues=int(rng.integers(1, 9)), slices=_pick(rng, (-1, 1, 2, 3, 4)), all_ordered=bool(rng.integers(0, 8) == 0),
                 max_total=_pick(rng, (128 << 20, 3 * U, U // 2)))
    if rng.integers(0, 4) == 0:
        knobs["comp_slices"] = tuple((int(c), _pick(rng, (1, 2, 3, 4))) for c in sorted({int(rng.integers(0, n)) for _ in range(2)}))
    return execs, knobs


def chains(seed):
    rng = np.random.default_rng([2, seed])
    n = int(rng.integers(4, 8))
    nb = int(rng.integers(3, 7))
    execs = []
    for _ in range(n):
        rd = sorted({int(rng.integers(0, nb)) for _ in range(int(rng.integers(1, 3)))})
        execs.append(ex([span(k) for k in rd], [span(int(rng.integers(0, nb)))], nlaunch=1 if rng.integers(0, 8) else 2, grid=_pick(rng, GRIDS),
                        sliceable=bool(rng.integers(0, 2))))
    return execs, dict(max_queues=1, slices=_pick(rng, (-1, 1, 2)))


def key(execs):
    """What distinguishes two chains for the scheduler's barrier rule: buffers read and written per execution, and the launches."""
    return tuple((tuple(sorted(s[0] // (64 * U) for s in e["rd"])), tuple(sorted(s[0] // (64 * U) for s in e["wr"])), e["nlaunch"]) for e in execs)


def from_rows(rows):
    """[(buffers read, buffers written) or (buffers read, buffers written, launches), ...] -> executions over whole buffers."""
    return [ex([span(k) for k in row[0]], [span(k) for k in row[1]], nlaunch=row[2] if len(row) > 2 else 1) for row in rows]
