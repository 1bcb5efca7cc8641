#!/usr/bin/env python3
"""Outer-product reductions, FAM_CONTRACT (contract = 2) against REDUCE_PART (contract = 0), on the same arrays in the same run.

Cases: mul_ at 256^3, 512^3 and 1024^3 for Float32, Float64, ComplexF64 and Int64; the skewed shapes (m, n, k) = (4096, 64, 64),
(64, 64, 4096) and (100, 90, 80); shapes large enough for the 64 x 64 tiles (2048^3, (4096, 2048, 256)); Float32 inputs into a Float64
destination (MIXED); a pairwise distance (f = abs2(a - b), op = +) and a min-plus product (f = a + b, op = min).
Every case is timed warm, two ways: plain HIP launches between two HIP events, and a recorded Sequence replayed by the library (host
clock around run + wait).  A timed window repeats the launch until it lasts about WINDOW seconds (the count is fixed per case from
a first estimate, the same for both plans).  The two plans alternate over ROUNDS rounds; the table prints the median per launch and the spread
(max - min over the rounds) of each, the ratio of the medians, and what the default gate (contract = 1) plans for the case.
The two plans' results are compared first (exactly for integers, to rounding otherwise).

The leading comment lines of an existing output file (the thresholds chosen from the table and what was tried and dropped: written by
hand) are kept; the table below them is replaced.

Usage: python tools/contract_cases.py [out.txt]      (default: profiles/contract_cases.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import strided_jl_amd as S  # noqa: E402
from bench import colmajor_view, event_time_ms  # noqa: E402

fn = S.fn
ROUNDS = 5
WINDOW = 0.2  # seconds per timed window
MARK = "# tools/contract_cases.py on "  # the first line this tool writes
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contract_cases.txt")
lines = []


def say(s=""):
    print(s)
    sys.stdout.flush()
    lines.append(s)


def cur():
    return int(torch.cuda.current_stream().cuda_stream)


def rand(shape, dt):
    n = int(np.prod(shape))
    if dt == torch.int64:
        t = torch.randint(-1000, 1000, (n,), dtype=dt, device="cuda")
    else:
        t = torch.randn(n, dtype=dt, device="cuda")
    return colmajor_view(S, t, shape)


def box(C, A, B):
    """The __mul! box of linalg.py: C2 = (m, n, 1), A2 = (m, 1, k), B2 = (1, n, k) for C (m, n), A (m, k), B (k, n)."""
    m, n = C.size
    k = A.size[1]
    A2 = S.StridedView(A.parent, (m, 1, k), (A.strides[0], 0, A.strides[1]), A.offset, A.op)
    B2 = S.StridedView(B.parent, (1, n, k), (0, B.strides[1], B.strides[0]), B.offset, B.op)
    C2 = S.StridedView(C.parent, (m, n, 1), (C.strides[0], C.strides[1], 0), C.offset, C.op)
    return (m, n, k), (C2, A2, B2)


def plans(f, op, dims, ops):
    out = {}
    old = S.get_option("contract")
    try:
        for c in (0, 2, 1):
            S.set_option("contract", c)
            out[c] = S.make_plan(f, op, "zero", dims, S.promoteshape(dims, *ops))
    finally:
        S.set_option("contract", old)
    return out


def time_hip(plan, reps):
    return event_time_ms(torch, lambda: plan.execute(cur()), reps) * 1e3


def time_seq(seq, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seq.run(reps, cur())
    seq.wait()
    return (time.perf_counter() - t0) / reps * 1e6


def run(name, f, op, dt, m, n, k, flop_per=2, dt_in=None):
    C, A, B = rand((m, n), dt), rand((m, k), dt_in or dt), rand((k, n), dt_in or dt)
    dims, ops = box(C, A, B)
    P = plans(f, op, dims, ops)
    res = {}
    for c in (0, 2):
        C.parent.zero_()
        P[c].execute(cur())
        torch.cuda.synchronize()
        res[c] = C.parent.clone()
    if dt == torch.int64:
        same = bool(torch.equal(res[0], res[2]))
    else:
        same = bool(torch.allclose(res[0], res[2], rtol=1e-4 if dt in (torch.float32,) else 1e-10, atol=1e-3 if dt == torch.float32 else 1e-9))
    work = 1.0 * m * n * k
    seqs = {c: S.Sequence().add(P[c]) for c in (0, 2)}
    for c in (0, 2):  # warm: code objects loaded, sequences resolved
        time_hip(P[c], 2)
        time_seq(seqs[c], 2)
    est = max(time_hip(P[c], 5) for c in (0, 2))  # us per launch of the slower plan
    reps = int(max(5, min(20000, WINDOW * 1e6 / est)))
    hip = {0: [], 2: []}
    sq = {0: [], 2: []}
    for _ in range(ROUNDS):
        for c in (0, 2):
            hip[c].append(time_hip(P[c], reps))
            sq[c].append(time_seq(seqs[c], reps))
    med = lambda v: statistics.median(v)  # noqa: E731
    spr = lambda v: max(v) - min(v)  # noqa: E731
    d1 = P[1].describe()
    fam1 = d1.split()[0].split("=")[1]
    d2 = P[2].describe()
    say("%-22s %-16s hip: c0 %8.1f +-%5.1f  c2 %8.1f +-%5.1f us  x%5.2f | seq: c0 %8.1f +-%5.1f  c2 %8.1f +-%5.1f us  x%5.2f | %6.2f Tops/s | reps=%d | same=%s | default=%s | %s" % (
        name, "(%d,%d,%d)" % (m, n, k), med(hip[0]), spr(hip[0]), med(hip[2]), spr(hip[2]), med(hip[0]) / med(hip[2]),
        med(sq[0]), spr(sq[0]), med(sq[2]), spr(sq[2]), med(sq[0]) / med(sq[2]), flop_per * work / med(hip[2]) / 1e6, reps, same, fam1,
        d2[d2.find("tile="):d2.find(" algbytes")]))
    seqs.clear()
    for p in P.values():
        p.close()


def main():
    say(MARK + "%s: contract = 0 (REDUCE_PART, c0) against contract = 2 (CONTRACT, c2); us per launch, median of %d rounds +- (max - min)" % (
        torch.cuda.get_device_name(0), ROUNDS))
    say("# x = c0 / c2; Tops/s = 2 m n k / c2's time through HIP; default = the family contract = 1 plans")
    mul = lambda a, b: a * b  # noqa: E731
    for dt, tn in ((torch.float32, "f32"), (torch.float64, "f64"), (torch.complex128, "c64"), (torch.int64, "i64")):
        for e in (256, 512, 1024):
            run("mul %s" % tn, mul, "+", dt, e, e, e)
    for dt, tn in ((torch.float32, "f32"), (torch.float64, "f64")):
        for m, n, k in ((4096, 64, 64), (64, 64, 4096), (100, 90, 80), (128, 128, 64), (192, 192, 256), (2048, 32, 256), (1000, 1000, 32), (1000, 1000, 16)):
            run("mul %s" % tn, mul, "+", dt, m, n, k)
    for dt, tn in ((torch.float32, "f32"), (torch.float64, "f64")):  # 64 x 64 tiles: 512 of them and more
        for m, n, k in ((2048, 2048, 2048), (4096, 2048, 256), (2048, 1024, 64)):
            run("mul %s" % tn, mul, "+", dt, m, n, k)
    for e in (256, 512, 1024):  # MIXED: operand types converted while staging, runtime-compiled
        run("mul f32->f64", mul, "+", torch.float64, e, e, e, dt_in=torch.float32)
    for e in (256, 512, 1024):
        run("pairwise f32", lambda a, b: fn.abs2(a - b), "+", torch.float32, e, e, e, 3)
        run("minplus f32", lambda a, b: a + b, "min", torch.float32, e, e, e)
    head = []
    if os.path.exists(OUT):
        with open(OUT) as fh:
            for ln in fh:
                if not ln.startswith("#") or ln.startswith(MARK):
                    break
                head.append(ln.rstrip("\n"))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(head + lines) + "\n")


if __name__ == "__main__":
    main()
