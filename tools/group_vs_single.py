#!/usr/bin/env python3
"""K small permutedims! calls issued four ways, warm, on one MI355X:

  (a) single   K plan executions one by one on a HIP stream (what a loop over blocks does today)
  (b) sequence the same K plans recorded into a Sequence and replayed by the library (default 4 queues)
  (c) group    ONE launch of a group of the K members through HIP (smr_group_execute, csrc/smr_k_group.hip)
  (d) recorded group  that group recorded into a Sequence (smr_seq_add_group): one kernel AND one pre-built packet per execution;
               with the default "slices", with "slices" = 1 (never cut) and with "slices" = 4 (the one launch cut into four block
               ranges on four hardware queues -- the scheduler cuts only launches of at least 64 workgroups per range)

Every member is a Float64 array of its own, permuted with the reversal permutation into an array of its own.  A round times
`reps` executions of each form between device synchronisations with the host clock (so launch cost on the host counts, as it does
for a user); rounds alternate the forms, the table gives the median over the rounds and the spread (min..max) in us per
execution of all K members.  The results of (c) and of every (d) are compared bit for bit with those of (a) before anything is timed.

    python tools/group_vs_single.py [--rounds 7] [--target-ms 250] [--out profiles/group_launch.txt]

--scalars: the per-member-scalar form (SMR_GROUP_MEMBER_SCALARS).  Every member is axpby!(a_i, permutedims(X_i, reverse), b_i, Y_i) in
place on Float64 arrays of its own, a_i = 1 + i/8 and b_i = 1/2 - i/512 (|b_i| < 1: repeated executions stay bounded), issued as

  (a)  single   the K plan executions one by one, each with its own scalars
  (c)  group    ONE launch of the group with SHARED scalars (every member a_0, b_0): the kernel as it was before the flag existed
  (c') group    ONE launch of the group with the flag: a row of the constant table per member
  (d') recorded the group of (c') recorded into a Sequence

with the same windows, rounds and alternation.  (c') and (d') are compared bit for bit with (a), (c) with single calls of the
shared scalars, after one execution from the same start, before anything is timed.  The last columns give (c') - (c), the larger
of the two forms' round-to-round spreads (max - min), whether the difference exceeds it, and (a) / (c').
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strided_jl_amd as S  # noqa: E402
from strided_jl_amd import _lib as L  # noqa: E402

SHAPES = [((8,) * 4, (2, 8, 32, 128)), ((16,) * 4, (2, 8, 32, 128)), ((4,) * 8, (2, 8, 32, 128)), ((32,) * 4, (8,))]


def dview(t, shape):
    st, s = [], 1
    for d in shape:
        st.append(s)
        s *= d
    return S.StridedView(t, shape, tuple(st), 0)


def timed(fn, reps, sync):
    sync()
    t0 = time.perf_counter()
    fn(reps)
    sync()
    return (time.perf_counter() - t0) / reps * 1e6


def scalars_main(args):
    import torch
    sync = torch.cuda.synchronize
    stream = int(torch.cuda.current_stream().cuda_stream)
    lines = ["# %s, %d rounds of >= %.0f ms per form, us per execution of all K members: median (min..max)" %
             (torch.cuda.get_device_name(0), args.rounds, args.target_ms),
             "# member = axpby!(a_i, permutedims(X_i, reverse), b_i, Y_i) in place, Float64; bytes = algorithmic bytes of one member",
             "# (c) = the group with shared scalars, (c') = with a row of scalars per member, (d') = (c') recorded in a sequence",
             "%-8s %9s %4s  %-28s %-26s %-26s %-26s %9s %8s %-7s %s" % ("shape", "bytes", "K", "(a) single", "(c) group shared", "(c') group member", "(d') recorded (c')",
                                                                    "(c')-(c)", "spread", "beyond", "(a)/(c')")]
    for shape in ((8,) * 4, (16,) * 4):
        n = int(np.prod(shape))
        perm = tuple(reversed(range(len(shape))))
        for K in (8, 32, 128):
            coef = [(1 + i / 8, 0.5 - i / 512) for i in range(K)]
            x = [dview(torch.randn(n, dtype=torch.float64, device="cuda"), shape) for _ in range(K)]
            y0 = [torch.randn(n, dtype=torch.float64, device="cuda") for _ in range(K)]
            ys = [[dview(t.clone(), shape) for t in y0] for _ in range(2)]   # [0]: the single calls, [1]: the groups

            def axpby(a, b):
                return lambda p, q: a * p + b * q

            def plans_of(y, cs):
                return [S.make_plan(axpby(a, b), None, None, shape, (d, s.permutedims(perm), d)) for d, s, (a, b) in zip(y, x, cs)]

            def group_of(y, cs, own):
                built = [S.build_problem(axpby(a, b), None, None, shape, (d, s.permutedims(perm), d), stream=stream) for d, s, (a, b) in zip(y, x, cs)]
                return L.Group([b[0] for b in built], keepalive=built, member_scalars=own)

            plans, plans0 = plans_of(ys[0], coef), plans_of(ys[0], coef[:1] * K)
            shared, member = group_of(ys[1], coef[:1] * K, False), group_of(ys[1], coef, True)
            assert "scalars=" not in shared.describe() and member.describe().endswith("scalars=member"), (shared.describe(), member.describe())
            seq = S.Sequence().add_group(member)
            sync()

            def single(reps):
                for _ in range(reps):
                    for p in plans:
                        p.execute(stream)

            def single0(reps):
                for _ in range(reps):
                    for p in plans0:
                        p.execute(stream)

            def group_shared(reps):
                for _ in range(reps):
                    shared.execute(stream)

            def group_member(reps):
                for _ in range(reps):
                    member.execute(stream)

            def recorded(reps):
                seq.run(reps, stream)
                seq.wait()

            def after_one(f, y):
                for d, t in zip(y, y0):
                    d.parent.copy_(t)
                sync()
                f(1)
                sync()
                return [d.parent.clone() for d in y]

            want, want0 = after_one(single, ys[0]), after_one(single0, ys[0])
            for f, w in ((group_member, want), (recorded, want), (group_shared, want0)):
                got = after_one(f, ys[1])
                assert all(torch.equal(a, b) for a, b in zip(got, w)), f.__name__ + " differs from the single calls"
            assert "backend=aql" in seq.info(), seq.info()
            forms = (single, group_shared, group_member, recorded)
            for f in forms:
                f(3)
            reps = [max(5, int(args.target_ms * 1e3 / max(timed(f, 5, sync), 0.5))) for f in forms]
            samples = [[] for _ in forms]
            for _ in range(args.rounds):
                for i, f in enumerate(forms):
                    samples[i].append(timed(f, reps[i], sync))
            med = [statistics.median(v) for v in samples]
            cell = ["%8.2f (%.2f..%.2f)" % (m, min(v), max(v)) for m, v in zip(med, samples)]
            diff = med[2] - med[1]
            spread = max(max(samples[1]) - min(samples[1]), max(samples[2]) - min(samples[2]))
            lines.append("%-8s %9d %4d  %-28s %-26s %-26s %-26s %+9.3f %8.3f %-7s %.1f" % ("%d^%d" % (shape[0], len(shape)), 2 * n * 8, K, *cell, diff, spread,
                                                                                    "yes" if abs(diff) > spread else "no", med[0] / med[2]))
            print(lines[-1], flush=True)
            del plans, plans0, shared, member, seq
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--target-ms", type=float, default=250.0, help="length of one timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--scalars", action="store_true", help="the per-member-scalar form: axpby! members, (a) / (c) / (c') / (d')")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("group_vs_single.py needs the MI355X: nothing is measured without it")
    if args.scalars:
        return scalars_main(args)
    sync = torch.cuda.synchronize
    stream = int(torch.cuda.current_stream().cuda_stream)
    lines = ["# %s, %d rounds of >= %.0f ms per form, us per execution of all K members: median (min..max)" %
             (torch.cuda.get_device_name(0), args.rounds, args.target_ms),
             "# member = permutedims!(dst, src, reverse) of a Float64 array; bytes = algorithmic bytes of one member",
             "# (d) = the group recorded in a sequence: slices default / 1 / 4 (sliced=0/1: whether the scheduler cut the launch)",
             "%-8s %9s %4s  %-26s %-26s %-26s %-26s %-26s %-28s %s" % ("shape", "bytes", "K", "(a) single", "(b) sequence", "(c) group", "(d) recorded group",
                                                                  "(d) slices=1", "(d) slices=4", "(d) beats (b) and (c)")]
    wins, dwins = [], []
    for shape, ks in SHAPES:
        n = int(np.prod(shape))
        perm = tuple(reversed(range(len(shape))))
        for K in ks:
            src = [dview(torch.randn(n, dtype=torch.float64, device="cuda"), shape) for _ in range(K)]
            dst = [dview(torch.zeros(n, dtype=torch.float64, device="cuda"), shape) for _ in range(K)]
            dst2 = [dview(torch.zeros(n, dtype=torch.float64, device="cuda"), shape) for _ in range(K)]
            plans = [S.make_plan(lambda x: x, None, None, shape, (d, s.permutedims(perm))) for d, s in zip(dst, src)]
            built = [S.build_problem(lambda x: x, None, None, shape, (d, s.permutedims(perm)), stream=stream) for d, s in zip(dst2, src)]
            grp = L.Group([b[0] for b in built], keepalive=built)
            seq = S.Sequence()
            for p in plans:
                seq.add(p)
            sync()

            def single(reps):
                for _ in range(reps):
                    for p in plans:
                        p.execute(stream)

            def sequence(reps):
                seq.run(reps, stream)
                seq.wait()

            def group(reps):
                for _ in range(reps):
                    grp.execute(stream)

            def recorded(q):
                def run(reps):
                    q.run(reps, stream)
                    q.wait()
                return run

            gseqs = []
            for slices in (None, 1, 4):
                q = S.Sequence().add_group(grp)
                if slices is not None:
                    q.set("slices", slices)
                gseqs.append(q)
            forms = (single, sequence, group) + tuple(recorded(q) for q in gseqs)
            for f in forms:  # warm: code objects, tables, packets; every form that writes dst2 is checked on zeroed destinations
                if f is not single and f is not sequence:
                    for e in dst2:
                        e.parent.zero_()
                    sync()
                f(3)
                sync()
                if f is not single and f is not sequence:
                    for d, e in zip(dst, dst2):
                        assert torch.equal(d.parent, e.parent), "group result differs from the single calls"
            how = [q.info() for q in gseqs]
            assert all("backend=aql" in h for h in how), how
            cut = ["sliced=1" in h for h in how]
            reps = []
            for f in forms:  # size every window from a short probe
                t = timed(f, 5, sync)
                reps.append(max(5, int(args.target_ms * 1e3 / max(t, 0.5))))
            samples = [[] for _ in forms]
            for _ in range(args.rounds):
                for i, f in enumerate(forms):
                    samples[i].append(timed(f, reps[i], sync))
            med = [statistics.median(x) for x in samples]
            cell = ["%8.2f (%.2f..%.2f)" % (m, min(x), max(x)) for m, x in zip(med, samples)]
            cell[5] += " sliced=%d" % cut[2]
            assert not cut[0] and not cut[1], how
            win = med[2] < med[0] and med[2] < med[1]
            wins.append((shape, K, 2 * n * 8, win, med[2] < med[0]))
            dwin = med[3] < med[1] and med[3] < med[2]
            dwins.append((shape, K, dwin, med[3] < med[1], med[3] < med[2], min(med[3:]) < med[1]))
            lines.append("%-8s %9d %4d  %-26s %-26s %-26s %-26s %-26s %-28s %s" % ("%d^%d" % (shape[0], len(shape)), 2 * n * 8, K, *cell, "yes" if dwin else "no"))
            print(lines[-1], flush=True)
            del plans, grp, seq, gseqs
    lines.append("")
    won = [(s, k, b) for s, k, b, w, _ in wins if w]
    if won:
        lines.append("# crossover: (c) beats both (a) and (b) at " + ", ".join("%d^%d K=%d" % (s[0], len(s), k) for s, k, _ in won))
        at8 = [b for s, k, b in won if k == 8]
        lines.append("# largest member at which (c) beats both at K = 8: " + ("%d bytes" % max(at8) if at8 else "none"))
    else:
        lines.append("# (c) does not beat both (a) and (b) at any row of this table")
    # the front replaces single calls, never a recorded sequence: the default of option group_max_bytes comes from this line
    a8 = [b for s, k, b, _, wa in wins if wa and k == 8]
    lines.append("# largest member at which (c) beats (a) at K = 8: " + ("%d bytes" % max(a8) if a8 else "none"))
    name = lambda s, k: "%d^%d K=%d" % (s[0], len(s), k)  # noqa: E731
    lines.append("# (d) beats both (b) and (c) at " + (", ".join(name(s, k) for s, k, w, _, _, _ in dwins if w) or "no row"))
    lines.append("# (d) does not beat (b) at " + (", ".join(name(s, k) for s, k, _, wb, _, _ in dwins if not wb) or "no row"))
    lines.append("# (d) does not beat (c) at " + (", ".join(name(s, k) for s, k, _, _, wc, _ in dwins if not wc) or "no row"))
    lines.append("# no slice setting of (d) beats (b) at " + (", ".join(name(s, k) for s, k, _, _, _, wany in dwins if not wany) or "no row"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
