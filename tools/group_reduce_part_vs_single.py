#!/usr/bin/env python3
"""K partial reductions -- one per block of a block-sparse tensor, each keeping a dim: a matrix-vector product y_i = A_i x_i, row
norms, sum(A_i; dims=2), sum(A_i; dims=(1,3)), y_i = A_i' x_i in ComplexF64; initop zero -- issued six ways, warm, on one MI355X:

  (a) single        K plan executions one by one on a HIP stream, default planner (what a loop over blocks gets without a group)
  (b) sequence      the K plans of (a) recorded into a Sequence and replayed by the library
  (c) group         ONE launch of the partial reduction group of the K members through HIP (SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART,
                    csrc/smr_k_greduce_part.hip)
  (d) recorded      that group recorded into a Sequence (smr_seq_add_group): one kernel and one pre-built packet per execution
  (e) front single  the K calls through the Python front (`_mapreducedim_` with initop zero), one launch each
  (f) front group   the same K calls inside `with S.group(reduce=True, reduce_part=True, independent=True):` -- one launch per block

Rows: K in {16, 128, 1024} blocks; the members are listed in rows().

All forms run in one process; a round times `reps` executions of each form between two device events (the sequence forms wait
for their replay before the second event is recorded), at least --target-ms of work per window; rounds alternate the forms; the
table gives the median over the rounds and the spread (min..max) in us per execution of all K members.  The data is
integer-valued: after the timing the destinations of every form are compared with those of (a), exactly.

    python tools/group_reduce_part_vs_single.py [--rounds 5] [--target-ms 60] [--out profiles/group_reduce_part.txt]
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
NFORMS = 6


ABS2 = "abs2"


def members():
    """(name, dtype, dims, f, destination strides, per input (strides, conj))"""
    f64, c64 = np.float64, np.complex128
    return [("8x8 f64 y=A*x", f64, (8, 8), MUL, (1, 0), [((1, 8), False), ((0, 1), False)]),
            ("32x32 f64 y=A*x", f64, (32, 32), MUL, (1, 0), [((1, 32), False), ((0, 1), False)]),
            ("32x32 f64 sum_j abs2", f64, (32, 32), ABS2, (1, 0), [((1, 32), False)]),
            ("32^3 f64 sum(dims=2)", f64, (32, 32, 32), None, (1, 0, 32), [((1, 32, 1024), False)]),
            ("32^3 f64 sum(dims=(1,3))", f64, (32, 32, 32), None, (0, 1, 0), [((1, 32, 1024), False)]),
            ("32x32 c64 y=A'*x", c64, (32, 32), MUL, (1, 0), [((32, 1), True), ((0, 1), False)])]


def rows():
    return [m + (K,) for m in members() for K in (16, 128, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--target-ms", type=float, default=60.0, help="length of one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("group_reduce_part_vs_single.py needs the MI355X: nothing is measured without it")
    sync = torch.cuda.synchronize
    stream = int(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)

    def block(shape, dt, strides, conj=False):
        """a view of `shape` with `strides` over a fresh contiguous array that holds exactly the elements the view reaches"""
        n = 1 + sum((e - 1) * st for e, st in zip(shape, strides))
        h = rng.integers(-3, 4, size=n).astype(dt)
        if np.dtype(dt).kind == "c":
            h = h + 1j * rng.integers(-3, 4, size=n)
        return S.StridedView(torch.from_numpy(h.astype(dt)).cuda(), shape, strides, 0, "conj" if conj else "identity")

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        e0.record()
        fn(reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    names = ("(a) single", "(b) sequence", "(c) group", "(d) recorded group", "(e) front single", "(f) front group")
    lines = ["# %s, %d rounds of >= %.0f ms per form between device events, us per execution of all K members: median (min..max)" %
             (torch.cuda.get_device_name(0), args.rounds, args.target_ms),
             "# member = one partial reduction per block, initop zero; (a) K single plans under the default planner; (b) those plans in a recorded",
             "# sequence; (c) ONE launch of the partial reduction group; (d) the group in a recorded sequence; (e) K calls through the Python front; (f) the",
             "# same calls inside `with S.group(reduce=True, reduce_part=True, independent=True):`",
             ("%-26s %5s " + "%-28s " * NFORMS + "%8s %8s %8s  %s") % (("blocks", "K") + names + ("(a)/(c)", "(b)/(d)", "(e)/(f)", "note"))]
    notes = []
    for name, dt, shape, f, dstrides, inlays, K in rows():
        cx = np.dtype(dt).kind == "c"
        f = S.fn.abs2 if f is ABS2 else (f or (lambda v: v))
        nout = 1 + sum((e - 1) * st for e, st in zip(shape, dstrides))          # the destinations are dense: member i owns [i * nout, (i + 1) * nout)
        ins = [tuple(block(shape, dt, st, cj) for st, cj in inlays) for _ in range(K)]
        outs = [S.StridedView(torch.zeros(K * nout, dtype=torch.complex128 if cx else torch.float64, device="cuda"), (K * nout,), (1,), 0) for _ in range(NFORMS)]
        dest = lambda j, i: S.StridedView(outs[j].parent, shape, dstrides, i * nout)   # noqa: E731
        ops = [[(dest(j, i),) + ins[i] for i in range(K)] for j in range(NFORMS)]
        plans_a = [S.make_plan(f, "+", "zero", shape, o) for o in ops[0]]
        plans_b = [S.make_plan(f, "+", "zero", shape, o) for o in ops[1]]
        fam = sorted({p.describe().split()[0].split("=")[1] + ":" + [t for t in p.describe().split() if t.startswith("form=")][0][5:] for p in plans_a})
        groups = []
        for j in (2, 3):
            built = [S.build_problem(f, "+", "zero", shape, o, stream=stream) for o in ops[j]]
            groups.append(L.Group([b[0] for b in built], keepalive=built, reduce=True, reduce_part=True))
        gdesc = groups[0].describe()
        seq_b = S.Sequence()
        for p in plans_b:
            seq_b.add(p)
        seq_d = S.Sequence().add_group(groups[1])
        sync()

        def single(reps):
            for _ in range(reps):
                for p in plans_a:
                    p.execute(stream)

        def replay(q):
            def run(reps):
                q.run(reps, stream)
                q.wait()
            return run

        def group(reps):
            for _ in range(reps):
                groups[0].execute(stream)

        def front(j):
            for o in ops[j]:
                S._mapreducedim_(f, "+", "zero", shape, o)

        def front_single(reps):
            for _ in range(reps):
                front(4)

        def front_group(reps):
            for _ in range(reps):
                with S.group(reduce=True, reduce_part=True, independent=True):
                    front(5)

        forms = (single, replay(seq_b), group, replay(seq_d), front_single, front_group)
        for fn in forms:   # warm: code objects, tables, packets, the front's caches
            fn(3)
            sync()
        reps = [max(3, int(args.target_ms * 1e3 / max(timed(fn, 3), 0.5))) for fn in forms]
        samples = [[] for _ in forms]
        for _ in range(args.rounds):
            for i, fn in enumerate(forms):
                samples[i].append(timed(fn, reps[i]))
        sync()
        for j in range(1, NFORMS):   # exact on integer-valued data
            assert torch.equal(outs[0].parent, outs[j].parent), "form %s differs from the single calls" % names[j]
        med = [statistics.median(v) for v in samples]
        cell = ["%9.2f (%.2f..%.2f)" % (m, min(v), max(v)) for m, v in zip(med, samples)]
        slower = [x for x, bad in (("(c) is SLOWER than (a)", med[2] > med[0]), ("(d) is SLOWER than (b)", med[3] > med[1]), ("(f) is SLOWER than (e)", med[5] > med[4])) if bad]
        if slower:
            notes.append("%s K=%d: %s" % (name, K, ", ".join(slower)))
        lines.append(("%-26s %5d " + "%-28s " * NFORMS + "%8.2f %8.2f %8.2f  %s") % ((name, K) + tuple(cell) + (med[0] / med[2], med[1] / med[3], med[4] / med[5], "; ".join(slower))))
        print(lines[-1], flush=True)
        print("#   single: family=%s | %s | %s" % ("+".join(fam), gdesc, seq_d.info().split(" last_replay")[0]), flush=True)
        lines.append("#   single: family=%s | %s" % ("+".join(fam), gdesc))
        del plans_a, plans_b, groups, seq_b, seq_d
    lines.append("")
    lines.append("# a group slower than what it replaces: " + ("; ".join(notes) or "no row"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
