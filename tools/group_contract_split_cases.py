#!/usr/bin/env python3
"""Contraction groups with a few long members (C_i = A_i * B_i, the generic mul! box, initop zero): the unsplit group against the
split form (option "group_contract_split"), on the same arrays in one process on one MI355X.

Per row, warm, these forms:

  u          the unsplit group: option 0, the tile the unsplit rule picks (what a library without the option does)
  u16 / u32  the unsplit group with the tile forced
  rule       group_contract_split = 1
  S<n>/t<T>  n = 2, 8, 32, 64 slices forced on tile T = 16, 32
  singles    the K single calls, contract_split = 1 (default "contract" = 1), one by one on a HIP stream
  seq        the same K plans recorded as a sequence and replayed
  rec        the rule's group (the unsplit one where the rule does not split) recorded with smr_seq_add_group

Rows: K = 4, 16, 64, 128 blocks of (32, 32, 4096) Float64; 16 blocks of (64, 64, 4096) Float32, of (16, 16, 65536) Float32 and of
(64, 64, 4096) ComplexF64; a mixed group of 1000 x (32, 32, 32) plus 2 x (32, 32, 16384) Float64; 64 blocks of (64, 64, 4096) Float32,
whose unsplit plan has 256 workgroups: the rule must leave it alone.

Every form is warmed first; a round times `reps` executions of each form between two device events (a sequence form waits for its
replay before the second event), at least --target-ms per window; the rounds alternate the forms; the table gives the median over
the rounds in us per execution of the whole group, and the spread (min..max) of the unsplit group.  A row on which the rule's group
is slower than the unsplit one by more than that spread (max - min of u) is flagged.  The data is integer-valued: after the timing
every form's destinations are compared with those of u, exactly.

    python tools/group_contract_split_cases.py [--rounds 5] [--target-ms 60] [--out FILE]
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
FORCED = [(s, t) for t in (16, 32) for s in (2, 8, 32, 64)]


class options:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: S.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            S.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            S.set_option(k, v)


def field(desc, key, default="-"):
    for tok in desc.split():
        if tok.startswith(key + "="):
            return tok.split("=", 1)[1]
    return default


def rows():
    out = [("%dx(32,32,4096) f64" % K, np.float64, [(32, 32, 4096)] * K) for K in (4, 16, 64, 128)]
    out.append(("16x(64,64,4096) f32", np.float32, [(64, 64, 4096)] * 16))
    out.append(("16x(16,16,65536) f32", np.float32, [(16, 16, 65536)] * 16))
    out.append(("16x(64,64,4096) c64", np.complex128, [(64, 64, 4096)] * 16))
    out.append(("1000x(32,32,32)+2x(32,32,16384) f64", np.float64, [(32, 32, 32)] * 500 + [(32, 32, 16384)] + [(32, 32, 32)] * 500 + [(32, 32, 16384)]))
    out.append(("64x(64,64,4096) f32 [>=256 wgs]", np.float32, [(64, 64, 4096)] * 64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--target-ms", type=float, default=60.0, help="length of one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("group_contract_split_cases.py needs the MI355X: nothing is measured without it")
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

    names = ["u", "u16", "u32", "rule"] + ["S%d/t%d" % st for st in FORCED] + ["singles", "seq", "rec"]
    lines = ["# %s, %d rounds of >= %.0f ms per form between device events; us per execution of the whole group, median over the rounds" %
             (torch.cuda.get_device_name(0), args.rounds, args.target_ms),
             "# u = unsplit group (option 0); u16 / u32 = unsplit, tile forced; rule = group_contract_split 1; S<n>/t<T> = n slices forced on tile T;",
             "# singles = the K single calls under contract_split = 1; seq = those plans as a recorded sequence; rec = the rule's group recorded",
             "%-38s %-24s %-26s " % ("row", "u (min..max)", "rule: tile grid kparts") + " ".join("%9s" % n for n in names[1:]) + "  u/rule  note"]
    losers = []
    for name, dt, shapes in rows():
        As = [mat(m, k, dt) for m, n, k in shapes]
        Bs = [mat(k, n, dt) for m, n, k in shapes]

        def group(split, tile):
            dests = [mat(m, n, dt, zero=True) for m, n, k in shapes]
            built = [S.build_problem(MUL, "+", "zero", *box(Cm, A, B), stream=stream) for Cm, A, B in zip(dests, As, Bs)]
            with options(group_contract_tile=tile, group_contract_split=split):
                g = L.Group([b[0] for b in built], keepalive=built)
            return g, dests

        def run_group(g):
            def run(reps):
                for _ in range(reps):
                    g.execute(stream)
            return run

        def replay(q):
            def run(reps):
                q.run(reps, stream)
                q.wait()
            return run

        forms, dsets, descs = [], [], []
        for split, tile in [(0, 0), (0, 16), (0, 32), (1, 0)] + FORCED:
            g, dests = group(split, tile)
            forms.append(run_group(g))
            dsets.append(dests)
            descs.append(g.describe())
        dests = [mat(m, n, dt, zero=True) for m, n, k in shapes]
        with options(contract_split=1):
            plans = [S.make_plan(MUL, "+", "zero", *box(Cm, A, B)) for Cm, A, B in zip(dests, As, Bs)]
        fams = sorted({field(p.describe(), "family") + ("/split" if "kparts=" in p.describe() else "") for p in plans})

        def singles(reps):
            for _ in range(reps):
                for p in plans:
                    p.execute(stream)

        forms.append(singles)
        dsets.append(dests)
        dests = [mat(m, n, dt, zero=True) for m, n, k in shapes]
        with options(contract_split=1):
            plans_q = [S.make_plan(MUL, "+", "zero", *box(Cm, A, B)) for Cm, A, B in zip(dests, As, Bs)]
        seq = S.Sequence()
        for p in plans_q:
            seq.add(p)
        forms.append(replay(seq))
        dsets.append(dests)
        g_rec, dests = group(1, 0)
        rec = S.Sequence().add_group(g_rec)
        forms.append(replay(rec))
        dsets.append(dests)
        sync()
        for f in forms:   # warm: code objects, tables, partials, packets
            f(3)
            sync()
        reps = [max(3, int(args.target_ms * 1e3 / max(timed(f, 3), 0.5))) for f in forms]
        samples = [[] for _ in forms]
        for _ in range(args.rounds):
            for i, f in enumerate(forms):
                samples[i].append(timed(f, reps[i]))
        sync()
        for j in range(1, len(forms)):   # exact on integer-valued data
            for x, y in zip(dsets[0], dsets[j]):
                assert torch.equal(x.parent, y.parent), "%s: form %s differs from the unsplit group" % (name, names[j])
        med = [statistics.median(v) for v in samples]
        spread = max(samples[0]) - min(samples[0])
        rd = descs[3]
        split = "split=" in rd
        note = "rule splits" if split else "rule leaves alone"
        if split and med[3] > med[0] + spread:
            note += ": SLOWER than u beyond its spread"
            losers.append(name)
        lines.append("%-38s %-24s %-26s " % (name, "%.2f (%.2f..%.2f)" % (med[0], min(samples[0]), max(samples[0])),
                                            "t%s g%s k%s (u: t%s g%s)" % (field(rd, "tile"), field(rd, "grid"), field(rd, "kparts"), field(descs[0], "tile"), field(descs[0], "grid"))) +
                     " ".join("%9.2f" % m for m in med[1:]) + "  %6.2f  %s" % (med[0] / med[3], note))
        print(lines[-1], flush=True)
        print("#   rule: " + rd + " | singles: " + "+".join(fams) + " | rec: " + rec.info().split(" last_replay")[0], flush=True)
        lines.append("#   rule: " + rd + " | singles: " + "+".join(fams))
        lines.append("#   kparts of the forced forms: " + " ".join("%s=%s" % (n, field(d, "kparts", "unsplit")) for n, d in zip(names[4:12], descs[4:])))
        del forms, plans, plans_q, seq, rec, g_rec
    lines.append("")
    lines.append("# rows the rule splits and loses on (beyond the spread of u): " + (", ".join(losers) or "none"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
