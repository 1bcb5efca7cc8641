#!/usr/bin/env python3
"""K small matrix products C_i = alpha_i * A_i * B_i (the generic mul! box, f = x * y * alpha, initop zero) with a DISTINCT alpha per
block, issued six ways, warm, on one MI355X:

  (a) single         K plan executions one by one on a HIP stream under option "contract" = 2 (f is a program: runtime-compiled)
  (b) K groups       what the front did before SMR_GROUP_CONTRACT_SCALARS: another alpha is another bucket -- K one-member groups
  (c) shared group   ONE unflagged group, every member with member 0's alpha (a runtime-compiled program with the constant as a kernel
                     argument): the reference for what the table of constants costs
  (d) member group   ONE group under SMR_GROUP_CONTRACT_SCALARS, scalars=member: the natively compiled f=mul2scale, a row per member
  (e) member, prog   the same group with f written alpha * (x * y) -- the same values, a program the planner does not recognise as the
                     mul! form: the scalars=member group through the runtime-compiled body
  (f) recorded       (d) recorded into a Sequence (smr_seq_add_group): one pre-built packet per execution

Rows: K in {16, 128, 1024} blocks of 32^3 Float64 and of 16^3 ComplexF64.

The method is tools/group_contract_vs_single.py's: all forms in one process; a round times `reps` executions of each form between
two device events (the sequence form waits for its replay before the second event is recorded), at least --target-ms of work per
window; rounds alternate the forms; the table gives the median over the rounds and the spread (min..max) in us per execution of
all K members.  The data is integer-valued: after the timing the destinations of (b), (d), (e) and (f) are compared with those of
(a), exactly.

    python tools/group_contract_scalars_vs_single.py [--rounds 7] [--target-ms 200] [--out profiles/group_contract_scalars.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import strided_jl_amd as S  # noqa: E402
from strided_jl_amd import _lib as L  # noqa: E402


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


def mula(alpha):
    return lambda x, y: x * y * alpha


def mula_prog(alpha):
    return lambda x, y: alpha * (x * y)


def rows():
    out = []
    for name, dt, n in (("32^3 float64", np.float64, 32), ("16^3 complex128", np.complex128, 16)):
        for K in (16, 128, 1024):
            out.append((name, dt, [(n, n, n)] * K))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--target-ms", type=float, default=200.0, help="length of one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("group_contract_scalars_vs_single.py needs the MI355X: nothing is measured without it")
    sync = torch.cuda.synchronize
    stream = int(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)

    def mat(m, n, dt, zero=False):
        if zero:
            h = np.zeros(m * n, dtype=dt)
        else:
            h = rng.integers(-3, 4, size=m * n).astype(dt)
            if np.dtype(dt).kind == "c":
                h = h + 1j * rng.integers(-3, 4, size=m * n)
        return S.StridedView(torch.from_numpy(h.astype(dt)).cuda(), (m, n), (1, m), 0)

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

    names = ("(a) single contract=2", "(b) K groups of one", "(c) group, shared alpha", "(d) group, scalars=member", "(e) (d) as a program", "(f) (d) recorded")
    lines = ["# %s, %d rounds of >= %.0f ms per form between device events, us per execution of all K members: median (min..max)" %
             (torch.cuda.get_device_name(0), args.rounds, args.target_ms),
             "# member = C_i = alpha_i * A_i * B_i (m, n, k), f = x * y * alpha_i, initop zero, a distinct alpha per block;",
             "# (a) K single plans under contract = 2; (b) K one-member groups (the front without contract_scalars); (c) ONE unflagged group with",
             "# one shared alpha (runtime-compiled program); (d) ONE scalars=member group, native mul2scale; (e) the same group as a",
             "# runtime-compiled program (f written alpha * (x * y)); (f) (d) in a recorded sequence",
             ("%-16s %5s %-5s" + " %-28s" * 6 + " %8s %8s %8s  %s") % (("blocks", "K", "tile") + names + ("(d)/(c)", "(d)/(e)", "(a)/(d)", "note"))]
    notes = []
    for name, dt, shapes in rows():
        K = len(shapes)
        cx = np.dtype(dt).kind == "c"
        alphas = [complex(2 + i, 1 + i % 3) if cx else 0.5 * (i + 3) for i in range(K)]   # distinct, never 1
        As = [mat(m, k, dt) for m, n, k in shapes]
        Bs = [mat(k, n, dt) for m, n, k in shapes]
        dests = [[mat(m, n, dt, zero=True) for m, n, k in shapes] for _ in range(6)]   # a destination set per form
        boxes = [[box(Cm, A, B) for Cm, A, B in zip(ds, As, Bs)] for ds in dests]
        with option("contract", 2):
            plans_a = [S.make_plan(mula(al), "+", "zero", d, ops) for al, (d, ops) in zip(alphas, boxes[0])]
        assert {field(p.describe(), "family") for p in plans_a} == {"contract"}

        def build(j, f_of, shared=False):
            return [S.build_problem(f_of(alphas[0] if shared else al), "+", "zero", d, ops, stream=stream) for al, (d, ops) in zip(alphas, boxes[j])]

        built_b = build(1, mula)
        groups_b = [L.Group([b[0]], keepalive=[b]) for b in built_b]
        built_c = build(2, mula, shared=True)
        group_c = L.Group([b[0] for b in built_c], keepalive=built_c)
        built_d = build(3, mula)
        group_d = L.Group([b[0] for b in built_d], keepalive=built_d, contract_scalars=True)
        built_e = build(4, mula_prog)
        group_e = L.Group([b[0] for b in built_e], keepalive=built_e, contract_scalars=True)
        built_f = build(5, mula)
        group_f = L.Group([b[0] for b in built_f], keepalive=built_f, contract_scalars=True)
        dc, dd, de = group_c.describe(), group_d.describe(), group_e.describe()
        assert field(dc, "f") == "prog" and field(dc, "jit") == "1" and "scalars=" not in dc, dc
        assert field(dd, "f") == "mul2scale" and field(dd, "jit") == "0" and dd.endswith("scalars=member"), dd
        assert field(de, "f") == "prog" and field(de, "jit") == "1" and de.endswith("scalars=member"), de
        assert field(dc, "tile") == field(dd, "tile") == field(de, "tile") and field(dc, "grid") == field(dd, "grid")
        seq_f = S.Sequence().add_group(group_f)
        sync()

        def single(reps):
            for _ in range(reps):
                for p in plans_a:
                    p.execute(stream)

        def many(reps):
            for _ in range(reps):
                for g in groups_b:
                    g.execute(stream)

        def one(g):
            def run(reps):
                for _ in range(reps):
                    g.execute(stream)
            return run

        def replay(reps):
            seq_f.run(reps, stream)
            seq_f.wait()

        forms = (single, many, one(group_c), one(group_d), one(group_e), replay)
        for f in forms:   # warm: code objects, tables, packets
            f(3)
            sync()
        reps = [max(3, int(args.target_ms * 1e3 / max(timed(f, 3), 0.5))) for f in forms]
        samples = [[] for _ in forms]
        for _ in range(args.rounds):
            for i, f in enumerate(forms):
                samples[i].append(timed(f, reps[i]))
        sync()
        for j in (1, 3, 4, 5):   # exact on integer-valued data ((c) computes with another alpha)
            for x, y in zip(dests[0], dests[j]):
                assert torch.equal(x.parent, y.parent), "form %d differs from the single calls" % j
        med = [statistics.median(v) for v in samples]
        cell = ["%9.2f (%.2f..%.2f)" % (m, min(v), max(v)) for m, v in zip(med, samples)]
        note = ""
        if med[3] - med[2] > max(samples[2]) - min(samples[2]):
            note = "(d) is slower than (c) by more than (c)'s spread"
            notes.append("%s K=%d" % (name, K))
        lines.append(("%-16s %5d %-5s" + " %-28s" * 6 + " %8.3f %8.3f %8.2f  %s") % ((name, K, field(dd, "tile")) + tuple(cell) + (med[3] / med[2], med[3] / med[4], med[0] / med[3], note)))
        print(lines[-1], flush=True)
        print("#   " + dd + " | " + seq_f.info().split(" last_replay")[0], flush=True)
        del plans_a, groups_b, group_c, group_d, group_e, group_f, seq_f
    lines.append("")
    lines.append("# (d) slower than (c) by more than (c)'s run-to-run spread: " + (", ".join(notes) or "no row"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
