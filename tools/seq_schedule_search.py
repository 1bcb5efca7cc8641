#!/usr/bin/env python3
"""Device-free search for replay schedules that break a rule of tests/sched_model.py.

    python tools/seq_schedule_search.py --seeds 300000 LIB [LIB2]

Runs the "chains" generator of tests/sched_fuzz_cases.py (one queue, 4-7 executions over 3-6 whole buffers) over seeds 0..N-1 through
smr_debug_seq_schedule of LIB (a libstrided_hip.so; it loads without a GPU) and prints every distinct failing list, as rows
(buffers read, buffers written) with its first seed, the barrier bits and the rules broken.  With LIB2 it also prints how many schedules
differ between the two libraries and whether any differing schedule was sound in the first.  profiles/seq_schedule_fuzz.txt is its
output for the build before and the build after the closure of the barrier rule (csrc/smr_sched.cpp: order_packets, step 5)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import sched_fuzz_cases as G  # noqa: E402
import sched_model as M  # noqa: E402


def sched_on(lib, execs, max_queues=4, slices=-1, all_ordered=False, max_total=128 << 20, comp_slices=()):
    """smr_debug_seq_schedule of `lib` (layout: include/strided_hip.h); returns the dict of tests/test_seq_schedule.py: sched()."""
    f = lib.smr_debug_seq_schedule
    f.restype = C.c_int
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    f.argtypes = [C.c_int, i32, i64, i32, i64, i32, i32, i32, i64, i32, C.c_int]
    n = len(execs)
    nspans, spans, launches = [], [], []
    for i, e in enumerate(execs):
        nspans += [len(e["rd"]), len(e["wr"])]
        for lo, hi in list(e["rd"]) + list(e["wr"]):
            spans += [lo, hi]
        launches += [e["nlaunch"], e["grid"], int(e["sliceable"]), int(e["all_self"]), i if e["same_as"] is None else e["same_as"]]
    cs = [v for pair in comp_slices for v in pair]
    per, tot, fp, cap = (C.c_int32 * (4 * max(1, n)))(), (C.c_int32 * 4)(), C.c_int64(0), 256
    pk = (C.c_int32 * (8 * cap))()
    npk = f(n, (C.c_int32 * max(1, len(nspans)))(*nspans), (C.c_int64 * max(1, len(spans)))(*spans), (C.c_int32 * max(1, len(launches)))(*launches),
            (C.c_int64 * 5)(max_queues, slices, int(all_ordered), max_total, len(comp_slices)), (C.c_int32 * max(1, len(cs)))(*cs), per, tot, C.byref(fp), pk, cap)
    assert 0 <= npk <= cap
    queues = {}
    for r in range(npk):
        queues.setdefault(pk[8 * r], []).append(tuple(pk[8 * r + 1:8 * r + 8]))
    cols = [[per[4 * i + c] for i in range(n)] for c in range(4)]
    return dict(comp=cols[0], acquire=cols[1], queue=cols[2], nslices=cols[3], ncomp=tot[0], nsliced=tot[1], nq=tot[2], resident=bool(tot[3]),
                footprint=fp.value, queues=queues)


def bits(r):
    return [p[M.BARRIER] for q in sorted(r["queues"]) for p in r["queues"][q]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seeds", type=int, default=100000)
    ap.add_argument("libs", nargs="+", help="one or two libstrided_hip.so")
    a = ap.parse_args()
    libs = [C.CDLL(os.path.abspath(p)) for p in a.libs[:2]]
    for k, lib in enumerate(libs):
        print("library %d: %s" % (k + 1, os.path.basename(a.libs[k])))
    print("recipe chains, seeds 0..%d" % (a.seeds - 1))
    failing = [0] * len(libs)
    distinct = [dict() for _ in libs]
    differ = differ_sound_in_first = 0
    for seed in range(a.seeds):
        execs, knobs = G.chains(seed)
        rs = [sched_on(lib, execs, **knobs) for lib in libs]
        vs = [M.check(execs, r, **knobs) for r in rs]
        for k, v in enumerate(vs):
            if v:
                failing[k] += 1
                distinct[k].setdefault(G.key(execs), (seed, execs, bits(rs[k]), M.rules_broken(v)))
        if len(libs) == 2 and rs[0] != rs[1]:
            differ += 1
            differ_sound_in_first += not vs[0]
    for k in range(len(libs)):
        print("library %d: %d of %d schedules break a rule, %d distinct lists" % (k + 1, failing[k], a.seeds, len(distinct[k])))
        for seed, execs, b, rules in sorted(distinct[k].values(), key=lambda t: t[0]):
            rows = [(tuple(s[0] // (64 * G.U) for s in e["rd"]), tuple(s[0] // (64 * G.U) for s in e["wr"])) for e in execs]
            print("  seed %d rules %s launches %s barrier bits %s rows %s" % (seed, ",".join(rules), [e["nlaunch"] for e in execs], b, rows))
    if len(libs) == 2:
        print("%d of %d schedules differ between library 1 and library 2; %d of them were sound in library 1" % (differ, a.seeds, differ_sound_in_first))
        if differ_sound_in_first == 0:
            print("no schedule that was sound at the parent changed (%d schedules compared)" % a.seeds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
