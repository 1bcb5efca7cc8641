#!/usr/bin/env python3
"""K complete reductions -- one per block of a block-sparse tensor: out[i] = sum(abs2, X_i) in Float64, out[i] = sum(conj(X_i) .* Y_i)
in ComplexF64, initop zero -- issued six ways, warm, on one MI355X:

  (a) single        K plan executions one by one on a HIP stream, default options (what a loop over blocks gets without a group)
  (b) sequence      the K plans of (a) recorded into a Sequence and replayed by the library
  (c) group         ONE launch of the reduction group of the K members through HIP (SMR_GROUP_REDUCE, csrc/smr_k_greduce.hip)
  (d) recorded      that group recorded into a Sequence (smr_seq_add_group): one kernel and one pre-built packet per execution
  (e) front single  the K calls through the Python front (`_mapreducedim_` with initop zero), one launch each
  (f) front group   the same K calls inside `with S.group(reduce=True, independent=True):` -- one launch per block

Rows: K in {16, 128, 1024} blocks of 8^2, 32^2 and 32^3 elements, in Float64 and in ComplexF64.

All forms run in one process; a round times `reps` executions of each form between two device events (the sequence forms wait
for their replay before the second event is recorded), at least --target-ms of work per window; rounds alternate the forms; the
table gives the median over the rounds and the spread (min..max) in us per execution of all K members.  The data is
integer-valued: after the timing the destinations of every form are compared with those of (a), exactly.

    python tools/group_reduce_vs_single.py [--rounds 7] [--target-ms 200] [--out profiles/group_reduce.txt]
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


def rows():
    out = []
    for dt in (np.float64, np.complex128):
        for shape in ((8, 8), (32, 32), (32, 32, 32)):
            for K in (16, 128, 1024):
                out.append(("%s %s" % ("x".join(map(str, shape)), np.dtype(dt).name), dt, shape, K))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--target-ms", type=float, default=200.0, help="length of one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("group_reduce_vs_single.py needs the MI355X: nothing is measured without it")
    sync = torch.cuda.synchronize
    stream = int(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)

    def block(shape, dt, conj=False):
        n = int(np.prod(shape))
        h = rng.integers(-3, 4, size=n).astype(dt)
        if np.dtype(dt).kind == "c":
            h = h + 1j * rng.integers(-3, 4, size=n)
        return S.StridedView(torch.from_numpy(h.astype(dt)).cuda(), shape, tuple(int(np.prod(shape[:d])) for d in range(len(shape))), 0, "conj" if conj else "identity")

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
             "# member = out[i] = sum(abs2, X_i) (Float64) or sum(conj(X_i) .* Y_i) (ComplexF64), initop zero; (a) K single plans; (b) those plans in a recorded",
             "# sequence; (c) ONE launch of the reduction group; (d) the group in a recorded sequence; (e) K calls through the Python front; (f) the same",
             "# calls inside `with S.group(reduce=True, independent=True):`",
             ("%-22s %5s " + "%-28s " * NFORMS + "%8s %8s %8s  %s") % (("blocks", "K") + names + ("(a)/(c)", "(b)/(d)", "(e)/(f)", "note"))]
    notes = []
    for name, dt, shape, K in rows():
        cx = np.dtype(dt).kind == "c"
        f = MUL if cx else S.fn.abs2
        N = len(shape)
        ins = [((block(shape, dt, conj=True), block(shape, dt)) if cx else (block(shape, dt),)) for _ in range(K)]
        outs = [S.StridedView(torch.zeros(K, dtype=torch.complex128 if cx else torch.float64, device="cuda"), (K,), (1,), 0) for _ in range(NFORMS)]
        dest = lambda j, i: S.StridedView(outs[j].parent, (1,) * N, (0,) * N, i)   # noqa: E731
        ops = [[S.promoteshape(shape, dest(j, i), *ins[i]) for i in range(K)] for j in range(NFORMS)]
        plans_a = [S.make_plan(f, "+", "zero", shape, o) for o in ops[0]]
        plans_b = [S.make_plan(f, "+", "zero", shape, o) for o in ops[1]]
        fam = sorted({p.describe().split()[0].split("=")[1] for p in plans_a})
        groups = []
        for j in (2, 3):
            built = [S.build_problem(f, "+", "zero", shape, o, stream=stream) for o in ops[j]]
            groups.append(L.Group([b[0] for b in built], keepalive=built, reduce=True))
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
                with S.group(reduce=True, independent=True):
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
        lines.append(("%-22s %5d " + "%-28s " * NFORMS + "%8.2f %8.2f %8.2f  %s") % ((name, K) + tuple(cell) + (med[0] / med[2], med[1] / med[3], med[4] / med[5], "; ".join(slower))))
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
