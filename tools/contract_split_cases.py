#!/usr/bin/env python3
"""The split form of FAM_CONTRACT (option "contract_split") against the library's default choice, on the same arrays in the same run.

Rows (m, n, k[, k2]), each for Float32, Float64 and ComplexF64: few outputs and a long reduced range -- (64,64,4096), (64,64,65536),
(32,32,1048576), (128,128,16384), (256,256,4096), (16,512,32768), two reduced dims (64,64,512,64) -- and two rows that must stay
unsplit, (100,90,80) and 1024^3.  Forms of a row:
  a   the default choice: contract = 1, contract_split = 0 (REDUCE_PART for the rows the rule splits)
  b   contract = 2, unsplit: one workgroup per output tile over the whole reduced range
  c   the rule: contract = 1, contract_split = 1
  d   contract = 2 with forced slices S in {2, 4, 8, 16, 32, 64} x forced tile in {16, 32, 64} (forms whose slices clamp to another
      form's plan are listed once); not for the two unsplit rows
The data is integer-valued (every accumulation order is exact): the forms' results are compared first, bit for bit with form a.
Every form is timed warm with plain HIP launches between two HIP events; a window repeats the launch until it lasts about WINDOW
seconds (the count is fixed per form from a first estimate); all forms of a row alternate over ROUNDS rounds; the table prints the
median per launch, the spread (max - min over the rounds) and the ratio to form a.  Under each row: the best forced form, and whether
the rule is faster than form a by more than the larger of the two spreads.

The shares of the two launches of a split plan come from a run of their own under the profiler:
  rocprofv3 --kernel-trace --stats -d DIR -o cs -- python tools/contract_split_cases.py --profile-run
  python tools/contract_split_cases.py --shares DIR/.../cs_results.db [out.txt]      (no GPU: reads the database, appends the shares)
--profile-run executes form c of every row PROFILE_REPS times, in the order of the table; --shares pairs the dispatches of
k_contract_split / k_contract_fold with the rows by that order.

The leading comment lines of an existing output file (the thresholds chosen from the table: written by hand) are kept; what this tool
wrote below them is replaced (the shares are appended to it).

Usage: python tools/contract_split_cases.py [out.txt]      (default: profiles/contract_split.txt)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import strided_jl_amd as S  # noqa: E402

ROUNDS = 5
WINDOW = 0.2  # seconds per timed window
PROFILE_REPS = 50
MARK = "# tools/contract_split_cases.py on "  # the first line this tool writes
SHARES = "# shares of the two launches of form c"
ROWS = [(64, 64, 4096), (64, 64, 65536), (32, 32, 1048576), (128, 128, 16384), (256, 256, 4096), (16, 512, 32768), (100, 90, 80),
        (1024, 1024, 1024), (64, 64, 512, 64)]
UNSPLIT = {(100, 90, 80), (1024, 1024, 1024)}
TYPES = ("f32", "f64", "c64")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
MODE = "profile" if "--profile-run" in sys.argv else ("shares" if "--shares" in sys.argv else "time")
lines = []


def say(s=""):
    print(s)
    sys.stdout.flush()
    lines.append(s)


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


def operands(dims, tn, device):
    """The product box over `dims` = (m, n, k[, k2]): C (m, n) and A (m, k[, k2]) column-major, B (n, k[, k2]) with k fastest; with
    two reduced dims the parents are padded along k, so that the two do not fuse.  Integer values of [-3, 3]."""
    m, n, red = dims[0], dims[1], dims[2:]
    pad = 1 if len(red) > 1 else 0
    kp = red[0] + pad
    q = int(np.prod(red[1:])) if len(red) > 1 else 1
    if device:
        import torch
        dt = {"f32": torch.float32, "f64": torch.float64, "c64": torch.complex128}[tn]
        mk = lambda cnt: torch.randint(-3, 4, (cnt,), device="cuda").to(dt)  # noqa: E731
    else:
        dt = {"f32": np.float32, "f64": np.float64, "c64": np.complex128}[tn]
        mk = lambda cnt: np.zeros(cnt, dtype=dt)  # noqa: E731
    tC, tA, tB = mk(m * n), mk(m * kp * q), mk(n * kp * q)
    N = len(dims)
    sa, sb = [1, 0, m] + [m * kp] * (N - 3), [0, kp * q, 1] + [kp] * (N - 3)
    C = S.StridedView(tC, (m, n) + (1,) * (N - 2), (1, m) + (0,) * (N - 2), 0)
    A = S.StridedView(tA, (m, 1) + tuple(red), tuple(sa), 0)
    B = S.StridedView(tB, (1, n) + tuple(red), tuple(sb), 0)
    return tC, (C, A, B)


def forms(dims, ops):
    """[(name, plan)]: a, b, c, then the forced forms whose plan differs from every form before."""
    def plan():
        return S.make_plan(lambda a, b: a * b, "+", "zero", dims, S.promoteshape(dims, *ops))
    out, seen = [], set()
    for name, kw in (("a default", dict(contract=1, contract_split=0)), ("b unsplit", dict(contract=2, contract_split=0)),
                     ("c rule", dict(contract=1, contract_split=1))):
        with options(**kw):
            out.append((name, plan()))
        seen.add(out[-1][1].describe())
    if MODE != "time" or tuple(dims) in UNSPLIT:
        return out
    for tile in (16, 32, 64):
        for s in (2, 4, 8, 16, 32, 64):
            with options(contract=2, contract_split=s, contract_tile=tile):
                p = plan()
            if p.describe() in seen or "kparts=" not in p.describe():
                p.close()
                continue
            seen.add(p.describe())
            out.append(("d t%d S%d" % (tile, s), p))
    return out


def short(desc):
    fam = desc.split()[0].split("=")[1]
    if fam == "contract":
        return "contract " + desc[desc.find("tile="):desc.find(" algbytes")]
    return fam + " " + desc[desc.find("form="):desc.find(" algbytes")]


def time_row(dims, tn):
    import torch
    from bench import event_time_ms
    cur = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    tC, ops = operands(dims, tn, True)
    F = forms(dims, ops)
    ref, same = None, True
    for name, p in F:  # results first: exact on this data
        tC.zero_()
        p.execute(cur())
        torch.cuda.synchronize()
        if ref is None:
            ref = tC.clone()
        elif not torch.equal(ref, tC):
            same = False
            say("  !! form %s differs from form a" % name)
    reps = {}
    for name, p in F:  # warm, and the launches per window
        event_time_ms(torch, lambda: p.execute(cur()), 3)
        est = event_time_ms(torch, lambda: p.execute(cur()), 5) * 1e3
        reps[name] = int(max(5, min(20000, WINDOW * 1e6 / est)))
    t = {name: [] for name, _ in F}
    for _ in range(ROUNDS):
        for name, p in F:
            t[name].append(event_time_ms(torch, lambda: p.execute(cur()), reps[name]) * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    spr = {k: max(v) - min(v) for k, v in t.items()}
    say("%s %s   (us per launch, median of %d rounds +- (max - min); x = a / form; results %s)" % (
        tn, "x".join(str(d) for d in dims), ROUNDS, "identical" if same else "DIFFER"))
    for name, p in F:
        say("  %-10s %9.1f +-%6.1f  x%6.2f  reps=%-5d | %s" % (name, med[name], spr[name], med["a default"] / med[name], reps[name], short(p.describe())))
    a, c = "a default", "c rule"
    forced = [n for n, _ in F if n.startswith("d ")]
    dc = dict(F)[c].describe()
    if dc == dict(F)[a].describe():
        say("  -> the rule leaves the plan of form a as it is: c %.1f against a %.1f us (spreads %.1f / %.1f)" % (med[c], med[a], spr[c], spr[a]))
    elif "kparts=" in dc:
        margin = max(spr[a], spr[c])
        say("  -> the rule splits: c %.1f against a %.1f us, %s (difference %.1f, larger spread %.1f)" % (
            med[c], med[a], "FASTER than a by more than the spread" if med[a] - med[c] > margin else "NOT faster than a by more than the spread",
            med[a] - med[c], margin))
    else:
        say("  -> the rule does not split: c %.1f against a %.1f us, %s (difference %.1f, larger spread %.1f)" % (
            med[c], med[a], "the same within the spread" if abs(med[a] - med[c]) <= max(spr[a], spr[c]) else "NOT the same within the spread",
            abs(med[a] - med[c]), max(spr[a], spr[c])))
    if forced:
        best = min(forced, key=lambda n: med[n])
        say("  -> best forced form: %s %.1f +-%.1f us; the rule is %s (c - best = %.1f, larger spread %.1f)" % (
            best, med[best], spr[best], "within its spread" if med[c] - med[best] <= max(spr[c], spr[best]) else "NOT within its spread",
            med[c] - med[best], max(spr[c], spr[best])))
    for _, p in F:
        p.close()
    del tC, ops
    torch.cuda.empty_cache()


def profile_run():
    import torch
    cur = lambda: int(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    for dims in ROWS:
        for tn in TYPES:
            tC, ops = operands(dims, tn, True)
            F = forms(dims, ops)
            p = dict(F)["c rule"]
            if "kparts=" in p.describe():
                for _ in range(PROFILE_REPS):
                    p.execute(cur())
                torch.cuda.synchronize()
            print("%s %s: %s" % (tn, "x".join(str(d) for d in dims), short(p.describe())))
            for _, q in F:
                q.close()
            del tC, ops
            torch.cuda.empty_cache()


def shares(db):
    """Pairs the dispatches of the two kernels, in start order, with the rows form c splits, PROFILE_REPS executions each."""
    import sqlite3
    cur = sqlite3.connect(db).cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    rows = list(cur.execute(f"select s.kernel_name, d.end - d.start from {kd} d join {ks} s on d.kernel_id = s.id order by d.start"))
    main = [ns for name, ns in rows if "k_contract_split" in name]
    fold = [ns for name, ns in rows if "k_contract_fold" in name]
    out = [SHARES + " (rocprofv3 --kernel-trace --stats, %d executions per row through HIP, a run of its own): median us per dispatch" % PROFILE_REPS]
    at = 0
    for dims in ROWS:
        for tn in TYPES:
            _, ops = operands(dims, tn, False)
            F = forms(dims, ops)
            d = dict(F)["c rule"].describe()
            for _, q in F:
                q.close()
            if "kparts=" not in d:
                continue
            m, f = main[at:at + PROFILE_REPS], fold[at:at + PROFILE_REPS]
            at += PROFILE_REPS
            if len(m) < PROFILE_REPS or len(f) < PROFILE_REPS:
                out.append("#   %s %s: dispatches missing from the trace" % (tn, "x".join(str(x) for x in dims)))
                continue
            mm, ff = statistics.median(m) / 1e3, statistics.median(f) / 1e3
            out.append("#   %-4s %-16s main %8.1f  fold %6.1f  (fold = %4.1f %% of the two) | %s" % (
                tn, "x".join(str(x) for x in dims), mm, ff, 100 * ff / (mm + ff), short(d)))
    if at != len(main) or at != len(fold):
        out.append("#   (%d main and %d fold dispatches in the trace, %d paired)" % (len(main), len(fold), at))
    return out


def main():
    out = args[-1] if args and args[-1].endswith(".txt") else os.path.join(ROOT, "profiles", "contract_split.txt")
    if MODE == "profile":
        return profile_run()
    old = []
    if os.path.exists(out):
        with open(out) as fh:
            old = [ln.rstrip("\n") for ln in fh]
    if MODE == "shares":
        keep = []
        for ln in old:
            if ln.startswith(SHARES):
                break
            keep.append(ln)
        body = keep + shares(args[0])
    else:
        import torch
        say(MARK + "%s: us per launch through HIP, median of %d rounds +- (max - min), windows of %.1f s" % (torch.cuda.get_device_name(0), ROUNDS, WINDOW))
        for dims in ROWS:
            for tn in TYPES:
                time_row(dims, tn)
        head = []
        for ln in old:
            if not ln.startswith("#") or ln.startswith(MARK):
                break
            head.append(ln)
        body = head + lines
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(body) + "\n")


if __name__ == "__main__":
    main()
