#!/usr/bin/env python3
"""K small matrix products C_i = A_i * B_i (the generic mul! box, initop zero) issued five ways, warm, on one MI355X:

  (a) single        K plan executions one by one on a HIP stream, default options (what a loop over blocks gets without a group:
                    a block below the CONTRACT gate runs REDUCE_PART)
  (b) single c=2    the same K calls planned under option "contract" = 2: the CONTRACT kernel for every block, one launch each
  (c) sequence      the K plans of (a) recorded into a Sequence and replayed by the library
  (d) group         ONE launch of the contraction group of the K members through HIP (smr_group_execute, csrc/smr_k_gcontract.hip)
  (e) recorded      that group recorded into a Sequence (smr_seq_add_group): one kernel and one pre-built packet per execution

Rows: K in {16, 128, 1024} blocks of 32^3 in Float64 and in Float32; a block-sparse mix of 256 Float64 blocks with extents drawn
from {8, 16, 24, 40, 64} (fixed seed); 64 blocks of 64^3 Float64 with the group's tile forced to 16 and to 32 (option
"group_contract_tile"): the one row on which both tiles are timed on the same problem.

All forms run in one process; a round times `reps` executions of each form between two device events (the sequence forms wait
for their replay before the second event is recorded), at least --target-ms of work per window; rounds alternate the forms; the
table gives the median over the rounds and the spread (min..max) in us per execution of all K members.  The data is
integer-valued: after the timing the destinations of (d) are compared with those of (a), exactly.

    python tools/group_contract_vs_single.py [--rounds 7] [--target-ms 200] [--out profiles/group_contract.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strided_jl_amd as S  # noqa: E402
from strided_jl_amd import _lib as L  # noqa: E402

MUL = lambda a, b: a * b  # noqa: E731


class option:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = S.get_option(self.name)
        S.set_option(self.name, self.value)

    def __exit__(self, *a):
        S.set_option(self.name, self.old)


def field(desc, key):
    for tok in desc.split():
        if tok.startswith(key + "="):
            return tok.split("=", 1)[1]
    return "?"


def rows():
    out = []
    for dt in (np.float64, np.float32):
        for K in (16, 128, 1024):
            out.append(("32^3 %s" % np.dtype(dt).name, dt, [(32, 32, 32)] * K, 0))
    rng = np.random.default_rng(20261020)
    ext = (8, 16, 24, 40, 64)
    out.append(("mix{8..64} float64", np.float64, [tuple(int(rng.choice(ext)) for _ in range(3)) for _ in range(256)], 0))
    out.append(("64^3 float64", np.float64, [(64, 64, 64)] * 64, 16))
    out.append(("64^3 float64", np.float64, [(64, 64, 64)] * 64, 32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--target-ms", type=float, default=200.0, help="length of one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("group_contract_vs_single.py needs the MI355X: nothing is measured without it")
    sync = torch.cuda.synchronize
    stream = int(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)

    def mat(m, n, dt, zero=False):
        h = np.zeros(m * n, dtype=dt) if zero else rng.integers(-3, 4, size=m * n).astype(dt)
        return S.StridedView(torch.from_numpy(h).cuda(), (m, n), (1, m), 0)

    def box(Cm, A, B):
        (m, n), k = Cm.size, A.size[1]
        A2 = S.StridedView(A.parent, (m, n, k), (A.strides[0], 0, A.strides[1]), A.offset, A.op)
        B2 = S.StridedView(B.parent, (m, n, k), (0, B.strides[1], B.strides[0]), B.offset, B.op)
        C2 = S.StridedView(Cm.parent, (m, n, k), (Cm.strides[0], Cm.strides[1], 0), Cm.offset, Cm.op)
        return (m, n, k), (C2, A2, B2)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        e0.record()
        fn(reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    lines = ["# %s, %d rounds of >= %.0f ms per form between device events, us per execution of all K members: median (min..max)" %
             (torch.cuda.get_device_name(0), args.rounds, args.target_ms),
             "# member = C_i = A_i * B_i (m, n, k), initop zero; (a) single calls, default options; (b) single calls under contract = 2;",
             "# (c) the plans of (a) in a recorded sequence; (d) ONE launch of the contraction group; (e) the group in a recorded sequence",
             "%-20s %5s %-9s %-12s %-28s %-28s %-28s %-28s %-28s %8s %8s  %s" % ("blocks", "K", "tile", "(a) family", "(a) single", "(b) single contract=2", "(c) sequence",
                                                                                "(d) group", "(e) recorded group", "(a)/(d)", "(b)/(d)", "note")]
    notes = []
    for name, dt, shapes, force in rows():
        K = len(shapes)
        As = [mat(m, k, dt) for m, n, k in shapes]
        Bs = [mat(k, n, dt) for m, n, k in shapes]
        dests = [[mat(m, n, dt, zero=True) for m, n, k in shapes] for _ in range(5)]   # a destination set per form
        boxes = [[box(Cm, A, B) for Cm, A, B in zip(ds, As, Bs)] for ds in dests]
        plans_a = [S.make_plan(MUL, "+", "zero", d, ops) for d, ops in boxes[0]]
        with option("contract", 2):
            plans_b = [S.make_plan(MUL, "+", "zero", d, ops) for d, ops in boxes[1]]
        plans_c = [S.make_plan(MUL, "+", "zero", d, ops) for d, ops in boxes[2]]
        fam_a = sorted({field(p.describe(), "family") for p in plans_a})
        assert {field(p.describe(), "family") for p in plans_b} == {"contract"}
        groups = []
        with option("group_contract_tile", force):
            for j in (3, 4):
                built = [S.build_problem(MUL, "+", "zero", d, ops, stream=stream) for d, ops in boxes[j]]
                groups.append(L.Group([b[0] for b in built], keepalive=built))
        gdesc = groups[0].describe()
        seq_c = S.Sequence()
        for p in plans_c:
            seq_c.add(p)
        seq_e = S.Sequence().add_group(groups[1])
        sync()

        def single(plans):
            def run(reps):
                for _ in range(reps):
                    for p in plans:
                        p.execute(stream)
            return run

        def replay(q):
            def run(reps):
                q.run(reps, stream)
                q.wait()
            return run

        def group(reps):
            for _ in range(reps):
                groups[0].execute(stream)

        forms = (single(plans_a), single(plans_b), replay(seq_c), group, replay(seq_e))
        for f in forms:   # warm: code objects, tables, packets
            f(3)
            sync()
        reps = [max(3, int(args.target_ms * 1e3 / max(timed(f, 3), 0.5))) for f in forms]
        samples = [[] for _ in forms]
        for _ in range(args.rounds):
            for i, f in enumerate(forms):
                samples[i].append(timed(f, reps[i]))
        sync()
        for j in (1, 2, 3, 4):   # exact on integer-valued data
            for x, y in zip(dests[0], dests[j]):
                assert torch.equal(x.parent, y.parent), "form %d differs from the single calls" % j
        med = [statistics.median(v) for v in samples]
        cell = ["%9.2f (%.2f..%.2f)" % (m, min(v), max(v)) for m, v in zip(med, samples)]
        note = ""
        if med[3] > med[0]:
            note = "(d) is SLOWER than (a)"
            notes.append("%s K=%d tile=%s" % (name, K, field(gdesc, "tile")))
        lines.append("%-20s %5d %-9s %-12s %-28s %-28s %-28s %-28s %-28s %8.2f %8.2f  %s" % (
            name, K, field(gdesc, "tile") + (" forced" if force else " rule"), "+".join(fam_a), *cell, med[0] / med[3], med[1] / med[3], note))
        print(lines[-1], flush=True)
        print("#   " + gdesc + " | " + seq_e.info().split(" last_replay")[0], flush=True)
        del plans_a, plans_b, plans_c, groups, seq_c, seq_e
    lines.append("")
    lines.append("# (d) slower than (a): " + (", ".join(notes) or "no row"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
