"""CPU: the replay scheduler (csrc/smr_sched.cpp: schedule(), through smr_debug_seq_schedule) against the independent checker
tests/sched_model.py, which knows byte-range conflicts only.

1. The checker is checked first: hand-written correct schedules pass, and one planted defect per rule is named by that rule alone.
2. Pinned lists: one-queue chains whose barrier bits were unsound while the bits were those of the second of two simulated replays
   (the window at the start of that simulated replay can be smaller than the one the chosen bits really leave behind): found by
   tools/seq_schedule_search.py (profiles/seq_schedule_fuzz.txt), kept as literal rows with their seeds.
3. Fuzz with fixed seeds, recipes "wide" and "chains" of tests/sched_fuzz_cases.py, WIDE and CHAINS cases each, none skipped, and the
   corpus itself is asserted not to be empty of what it is for (several queues, cut components, two-launch executions, free packets)."""
import collections
import copy

import pytest

import sched_fuzz_cases as G
import sched_model as M
from test_seq_schedule import U, ex, sched, span

WIDE = 10000
CHAINS = 12000


def broken(execs, r, **knobs):
    return M.rules_broken(M.check(execs, r, **knobs))


# ---- 1. the checker ---------------------------------------------------------------------------------------------------------------------
def chain_schedule():
    """A -> B in one launch, B -> C in two (a folding pass): one component on one queue, written by hand from the rules."""
    a, b, c = span(0), span(1), span(2)
    execs = [ex([a], [b]), ex([b], [c], nlaunch=2)]
    r = dict(comp=[0, 0], acquire=[0, 1], queue=[0, 0], nslices=[1, 1], ncomp=1, nsliced=0, nq=1, resident=True, footprint=3 * U,
             queues={0: [(0, 0, 0, 0, 4096, 1, 0), (1, 0, 0, 0, 4096, 1, 1), (1, 1, 0, 0, 0, 1, 1)]})
    return execs, r, dict(max_queues=4)


def cut_schedule():
    """One launch of 1000 workgroups cut in two at ceil(1000 / 2) rounded up to a multiple of 8."""
    execs = [ex([span(0)], [span(1)], grid=1000)]
    r = dict(comp=[0], acquire=[0], queue=[0], nslices=[2], ncomp=1, nsliced=1, nq=2, resident=True, footprint=2 * U,
             queues={0: [(0, 0, 0, 0, 504, 1, 0)], 1: [(0, 0, 1, 504, 1000, 1, 0)]})
    return execs, r, dict(max_queues=4, slices=2)


def free_schedule():
    """The bench step on one queue: the second execution shares nothing written with the first and goes out unordered."""
    u, v, w = span(0), span(1), span(2)
    execs = [ex([u], [v]), ex([u], [w])]
    r = dict(comp=[0, 1], acquire=[0, 0], queue=[0, 0], nslices=[1, 1], ncomp=2, nsliced=0, nq=1, resident=True, footprint=3 * U,
             queues={0: [(0, 0, 0, 0, 4096, 1, 0), (1, 0, 0, 0, 4096, 0, 0)]})
    return execs, r, dict(max_queues=1)


def edit(r, q, k, **fields):
    names = dict(exec=M.EXEC, launch=M.LAUNCH, slice=M.SLICE, lo=M.LO, hi=M.HI, barrier=M.BARRIER, acquire=M.ACQUIRE)
    p = list(r["queues"][q][k])
    for name, v in fields.items():
        p[names[name]] = v
    r["queues"][q][k] = tuple(p)


def plant_boundary_barrier(r):   # execution 0 rewrites B while the previous replay's execution 1 may still read it
    edit(r, 0, 0, barrier=0)


def plant_two_queues(r):         # execution 1 reads what execution 0 writes, from another queue
    r["queues"][1] = r["queues"][0][1:]
    r["queues"][0] = r["queues"][0][:1]
    r["queue"], r["nq"] = [0, 1], 2


def plant_slice_gap(r):          # workgroups 496..503 run nowhere
    edit(r, 0, 0, hi=496)


def plant_odd_cut(r):            # 500 is no multiple of 8: the second slice's workgroups change their XCD
    edit(r, 0, 0, hi=500)
    edit(r, 1, 0, lo=500)


def plant_missing_acquire(r):    # execution 1 reads B, which execution 0 wrote
    edit(r, 0, 1, acquire=0)


def plant_dropped_launch(r):     # the folding pass of execution 1
    del r["queues"][0][2]


def plant_footprint(r):
    r["footprint"] += 1


def plant_not_resident(r):
    r["resident"] = False


def plant_free_conflict(r):      # inside one replay: execution 1 of the chain reads what execution 0 writes
    edit(r, 0, 1, barrier=0)


PLANTED = [("barriers", chain_schedule, plant_boundary_barrier), ("barriers", chain_schedule, plant_free_conflict),
           ("components", chain_schedule, plant_two_queues), ("slices", cut_schedule, plant_slice_gap), ("slices", cut_schedule, plant_odd_cut),
           ("acquire", chain_schedule, plant_missing_acquire), ("completeness", chain_schedule, plant_dropped_launch),
           ("footprint", chain_schedule, plant_footprint), ("footprint", cut_schedule, plant_not_resident)]


@pytest.mark.parametrize("base", [chain_schedule, cut_schedule, free_schedule], ids=lambda f: f.__name__)
def test_hand_written_schedules_pass_and_are_what_the_scheduler_gives(base):
    execs, r, knobs = base()
    assert M.check(execs, r, **knobs) == []
    assert sched(execs, **knobs) == r


@pytest.mark.parametrize("rule,base,plant", PLANTED, ids=[p[2].__name__ for p in PLANTED])
def test_a_planted_defect_is_named_by_its_rule_and_no_other(rule, base, plant):
    execs, r, knobs = base()
    r = copy.deepcopy(r)
    plant(r)
    v = M.check(execs, r, **knobs)
    assert M.rules_broken(v) == [rule], v


def test_every_rule_has_a_planted_defect():
    assert {p[0] for p in PLANTED} == set(M.RULES)


def test_all_ordered_asks_for_every_bit():
    execs, r, knobs = free_schedule()
    assert broken(execs, r, all_ordered=True, **knobs) == ["barriers"]


# ---- 2. pinned lists --------------------------------------------------------------------------------------------------------------------
# (buffers read, buffers written) per execution, whole disjoint buffers, one launch each, one queue
FIVE = [((1, 2), (1,)), ((3,), (3,)), ((0, 1), (0,)), ((1, 3), (2,)), ((3,), (0,))]
# every distinct failing chain of seeds 0..299999 of the "chains" recipe before the closure (profiles/seq_schedule_fuzz.txt): (seed, rows);
# a third entry of a row is its number of launches
PINNED = [
    (361, [((1,), (2,)), ((0, 3), (3,)), ((0, 2), (1,)), ((2, 5), (3,)), ((4,), (0,))]),
    (366, [((0, 3), (2,), 2), ((0, 1), (1,)), ((3,), (2,)), ((0,), (0,), 2), ((1, 2), (1,)), ((0,), (3,), 2), ((0,), (1,))]),
    (678, [((0,), (1,)), ((0,), (2,)), ((1, 4), (3,)), ((4,), (0,)), ((2, 3), (2,))]),
    (11664, [((2,), (3,)), ((4, 5), (1,)), ((0, 3), (2,)), ((3, 4), (5,)), ((2,), (1,))]),
    (15103, [((1,), (0,)), ((3, 4), (4,)), ((0,), (2,)), ((0,), (3,)), ((2,), (4,))]),
    (21553, [((4,), (2,)), ((0, 4), (0,)), ((2, 3), (1,)), ((3, 4), (4,)), ((1,), (0,))]),
    (32757, [((3,), (1,)), ((0,), (2,)), ((1,), (3,)), ((1,), (2,)), ((3,), (0,))]),
    (38385, [((3,), (1,)), ((4,), (2,)), ((0,), (1,)), ((2, 3), (3,), 2), ((2, 4), (0,))]),
    (50599, [((0,), (1,)), ((4,), (4,)), ((5,), (5,)), ((0, 3), (0,)), ((2, 5), (4,)), ((5,), (3,))]),
    (57822, [((1, 2), (2,)), ((1,), (4,)), ((2,), (2,), 2), ((0, 3), (3,)), ((0,), (1,)), ((4,), (3,))]),
    (83947, [((1, 2), (1,)), ((2, 5), (5,)), ((4,), (4,)), ((1, 3), (3,)), ((0,), (2,)), ((3, 5), (5,))]),
    (91449, [((2,), (0,)), ((2, 3), (3,)), ((0,), (1,)), ((2,), (2,)), ((3,), (1,))]),
    (92778, [((2, 4), (3,)), ((0,), (0,)), ((4, 5), (4,)), ((0,), (3,)), ((0, 1), (5,))]),
    (94996, [((4,), (4,)), ((0, 5), (5,), 2), ((3, 4), (2,)), ((0, 5), (1,)), ((3, 5), (2,)), ((4,), (0,)), ((1, 5), (3,))]),
    (99308, [((3,), (1,)), ((0,), (0,)), ((1, 4), (1,)), ((0,), (3,)), ((0,), (4,))]),
    (112598, [((0,), (2,), 2), ((0,), (3,)), ((2,), (4,)), ((0, 1), (0,)), ((4,), (3,)), ((0,), (2,)), ((3,), (4,))]),
    (112971, [((1,), (2,)), ((4,), (5,)), ((0, 2), (1,)), ((2,), (4,), 2), ((1, 3), (5,))]),
    (116710, [((0,), (2,)), ((1,), (3,), 2), ((2,), (0,)), ((2,), (3,)), ((0, 1), (1,))]),
    (118348, [((4, 5), (4,)), ((2,), (3,)), ((2,), (1,)), ((0, 4), (0,)), ((1, 4), (3,)), ((0,), (2,))]),
    (119484, [((4,), (1,)), ((0,), (2,)), ((0, 4), (4,)), ((2,), (1,)), ((4,), (0,))]),
    (125480, [((3,), (0,)), ((1,), (1,)), ((0,), (2,)), ((1,), (3,)), ((1,), (0,)), ((2, 3), (3,)), ((1,), (1,))]),
    (130298, [((2, 3), (0,), 2), ((1, 3), (1,)), ((0, 5), (4,)), ((3,), (3,)), ((0, 1), (2,)), ((1,), (5,))]),
    (142869, [((1,), (0,)), ((1,), (2,)), ((0,), (3,), 2), ((0,), (1,)), ((2, 3), (3,))]),
    (152904, [((1, 5), (5,)), ((0, 1), (2,)), ((4,), (3,)), ((2, 4), (5,)), ((2, 3), (1,)), ((0, 4), (4,))]),
    (161095, [((3,), (1,)), ((5,), (2,)), ((0, 3), (0,)), ((2, 3), (5,), 2), ((0, 2), (1,)), ((0, 5), (4,))]),
    (180557, [((2, 5), (4,)), ((1, 3), (0,)), ((5,), (2,), 2), ((0, 4), (3,)), ((2,), (1,))]),
    (189212, [((0, 4), (3,)), ((4,), (1,), 2), ((3,), (0,)), ((3,), (4,)), ((0, 1), (2,))]),
    (193009, [((1, 4), (0,)), ((1, 4), (3,)), ((2, 4), (0,)), ((4,), (1,)), ((3,), (2,))]),
    (193445, [((1,), (0,), 2), ((2, 3), (5,)), ((2, 4), (1,)), ((0, 5), (5,)), ((3, 4), (4,)), ((1,), (2,))]),
    (204988, [((1, 5), (4,)), ((3,), (0,)), ((2, 3), (5,)), ((0,), (1,)), ((3,), (3,))]),
    (211157, [((0, 2), (2,), 2), ((1,), (1,)), ((3,), (0,)), ((1, 2), (1,)), ((3,), (3,)), ((2,), (2,)), ((1,), (3,))]),
    (215583, [((1, 3), (3,), 2), ((0,), (2,)), ((0,), (4,)), ((1,), (1,)), ((2, 3), (0,)), ((1,), (4,))]),
    (224795, [((2,), (1,)), ((3,), (0,)), ((1, 2), (2,)), ((1, 3), (3,)), ((2,), (0,))]),
    (242097, [((1, 3), (3,)), ((0, 4), (5,)), ((2,), (1,)), ((2, 3), (5,)), ((0, 1), (4,))]),
    (248221, [((4,), (1,)), ((0, 4), (3,)), ((2,), (1,)), ((0,), (4,)), ((2, 3), (2,))]),
    (265987, [((0, 2), (2,)), ((3,), (4,)), ((1,), (0,)), ((2,), (4,)), ((0,), (3,))]),
    (266204, [((3, 5), (2,)), ((1, 4), (4,)), ((5,), (3,)), ((1,), (0,)), ((2,), (4,)), ((0, 3), (1,))]),
    (270721, [((1,), (4,), 2), ((1,), (2,)), ((0, 1), (3,), 2), ((4, 5), (5,)), ((4,), (1,)), ((2, 5), (5,)), ((3,), (3,))]),
    (272355, [((4,), (2,)), ((4,), (3,)), ((0, 2), (0,)), ((1,), (4,)), ((3,), (0,))]),
    (284728, [((1,), (5,)), ((0, 2), (3,)), ((5,), (1,)), ((5,), (2,)), ((1,), (0,))]),
    (291393, [((3,), (0,)), ((4,), (1,)), ((0,), (2,)), ((1,), (3,)), ((1, 2), (4,))]),
    (298015, [((3,), (1,)), ((3,), (0,)), ((1,), (2,)), ((1,), (3,)), ((2,), (0,))]),
]


def test_the_smallest_case_found():
    """Execution 3 writes buffer 2; execution 4 and execution 0 of the next replay conflict with nothing in between, and execution 0
    reads buffer 2.  Bits 0,1,0,1,0 let it overlap execution 3 of the previous replay; closed, execution 0 carries the bit and the
    other four are as before."""
    execs = G.from_rows(FIVE)
    r = sched(execs, max_queues=1)
    assert M.check(execs, r, max_queues=1) == []
    assert [p[M.BARRIER] for p in r["queues"][0]] == [1, 1, 0, 1, 0]


@pytest.mark.parametrize("seed,rows", PINNED, ids=[str(s) for s, _ in PINNED])
def test_pinned_chains(seed, rows):
    execs = G.from_rows(rows)
    r = sched(execs, max_queues=1)
    assert M.check(execs, r, max_queues=1) == []
    assert 0 in [p[M.BARRIER] for p in r["queues"][0]]   # (closing the rule did not order everything)


def test_at_least_five_pinned_chains_and_all_distinct():
    assert len(PINNED) >= 5 and len({tuple(rows) for _, rows in PINNED} | {tuple(FIVE)}) == len(PINNED) + 1


# ---- 3. fuzz ----------------------------------------------------------------------------------------------------------------------------
def run(recipe, count):
    stats = collections.Counter()
    failures = []
    for seed in range(count):
        execs, knobs = recipe(seed)
        r = sched(execs, **knobs)
        v = M.check(execs, r, **knobs)
        if v:
            failures.append((seed, M.rules_broken(v), v[0][1]))
        pk = [p for q in r["queues"].values() for p in q]
        stats["cases"] += 1
        stats["two queues"] += r["nq"] >= 2
        stats["cut"] += r["nsliced"] >= 1
        stats["two launches"] += any(p[M.LAUNCH] == 1 for p in pk)
        stats["free packet"] += any(not p[M.BARRIER] for p in pk)
        stats["several components"] += r["ncomp"] >= 2
        stats["acquire"] += any(p[M.ACQUIRE] for p in pk)
    return stats, failures


def test_fuzz_wide():
    stats, failures = run(G.wide, WIDE)
    print(dict(stats))
    assert stats["cases"] == WIDE >= 10000
    assert stats["two queues"] >= 1000 and stats["cut"] >= 300 and stats["two launches"] >= 300, dict(stats)
    assert stats["free packet"] >= 1000 and stats["several components"] >= 1000, dict(stats)
    assert not failures, "%d of %d schedules break a rule; first (seed, rules, what): %s" % (len(failures), WIDE, failures[:5])


def test_fuzz_chains():
    stats, failures = run(G.chains, CHAINS)
    print(dict(stats))
    assert stats["cases"] == CHAINS >= 10000
    assert stats["free packet"] >= 1000 and stats["two launches"] >= 300, dict(stats)
    assert not failures, "%d of %d schedules break a rule; first (seed, rules, what): %s" % (len(failures), CHAINS, failures[:5])
