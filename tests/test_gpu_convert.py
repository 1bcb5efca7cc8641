"""GPU: the converting calls of tests/convert_cases.py in every kernel family, the WHOLE destination parent compared byte for byte with the
MODEL of Julia's conversions and per-operation typing (not with the oracle, which runs the same f-program as the device).

Every row runs through the one-shot entry point with the f-program interpreted (jit = 0); the rows of the compiled subset (every pure
conversion in STREAM, TILED and a reduction epilogue, and the listed mixed expressions: 40 compiled kernels at most,
tests/test_convert_host.py) run runtime-compiled too.  Reduction and TILED rows also run as a plan executed onto a fresh destination and
inside a recorded sequence.  After each run the destination's whole root allocation must hold the model's result inside the view and its
first contents outside, and every input root must be unchanged.  The device plan must be the cell the row names."""
import numpy as np
import pytest

import convert_cases as CC
import strided_jl_amd as S
import window_cases as W
from util import to_device

pytestmark = pytest.mark.gpu
NAMED = {"stream2c": "stream2", "tiled3": "tiled"}


class jit_mode:
    """with jit_mode(jit): the "jit" option set and restored.  Under jit = 1 a runtime-compiled kernel must have run (compiled or found in
    the cache) and no compilation may have failed -- the library would fall back to the interpreter without an error; under jit = 0 no
    runtime-compiled kernel may have run.  (Every converting call takes the f-program: none of the table's rows has a precompiled kernel.)"""

    def __init__(self, jit):
        self.jit = int(jit)

    def __enter__(self):
        self.old = S.get_option("jit")
        S.set_option("jit", self.jit)
        self.before = [S.get_option(k) for k in ("jit_compiles", "jit_hits", "jit_failures")]
        return self

    def __exit__(self, et, ev, tb):
        S.set_option("jit", self.old)
        if et is None:
            c, h, f = [S.get_option(k) for k in ("jit_compiles", "jit_hits", "jit_failures")]
            assert f == self.before[2], "runtime compilation failed"
            if self.jit:
                assert c + h > self.before[0] + self.before[1], "no runtime-compiled kernel ran"
            else:
                assert c + h == self.before[0] + self.before[1], "jit = 0 ran a runtime-compiled kernel"


def check(r, cache, what):
    dkey = r.arrays[0].parent.ctypes.data
    r.desc = what
    msg = r.mismatch(cache[dkey].cpu().numpy()) or r.inputs_changed({k: t.cpu().numpy() for k, t in cache.items() if k != dkey})
    assert msg is None, msg


def run_row(r, compiled):
    """The modes of one row; returns how many ran."""
    import torch
    stream = int(torch.cuda.current_stream().cuda_stream)
    planned = r.op is not None or r.cell.startswith("tiled")
    modes = ["one-shot"] + (["plan", "sequence"] if planned and not compiled else [])
    for mode in modes:
        with jit_mode(compiled):   # (around every run: each must take the kernel kind it is named after)
            cache = {}
            dev = tuple(to_device(a, cache) for a in r.arrays)
            torch.cuda.synchronize()
            desc = ""
            if mode == "one-shot":
                S._mapreduce_fuse_(r.f, r.op, r.initop, r.dims, dev)
                torch.cuda.synchronize()
            else:
                plan = q = None
                try:
                    plan = r.plan(dev)
                    desc = plan.describe()
                    assert CC.reached(desc, r.types) == NAMED.get(r.cell, r.cell) and "(mixed)" in desc, "%s: device plan [%s]" % (r.name, desc)
                    if mode == "plan":
                        plan.execute(stream)
                    else:
                        q = S.Sequence().add(plan)
                        q.run(1, stream)
                        q.wait()
                    torch.cuda.synchronize()
                finally:
                    if q is not None:
                        del q           # (the sequence goes before the plan it replays)
                    if plan is not None:
                        plan.close()
            check(r, cache, "%s jit=%d %s" % (mode, int(compiled), desc))
    return len(modes)


@pytest.mark.parametrize("cell", CC.cells())
def test_converting_calls_interpreted(cell):
    n = runs = 0
    for r in CC.rows(cell):
        runs += run_row(r, False)
        n += 1
    print("[convert] %s: %d rows, %d runs interpreted" % (cell, n, runs))
    assert n == sum(1 for s in CC.TABLE if s["cell"] == cell) > 0


@pytest.mark.parametrize("cell", sorted({s["cell"] for s in CC.TABLE if s.get("jit")}))
def test_converting_calls_runtime_compiled(cell):
    n = 0
    for s in CC.TABLE:
        if s["cell"] == cell and s.get("jit"):
            run_row(CC.build(s), True)
            n += 1
    print("[convert] %s: %d rows runtime-compiled" % (cell, n))
    assert n == sum(1 for s in CC.TABLE if s["cell"] == cell and s.get("jit")) > 0


@pytest.mark.parametrize("cell,form", [("group:linear", 0), ("group:tiled", 1)])
@pytest.mark.parametrize("jit", [0, 1])
def test_grouped_conversions(cell, form, jit):
    """Int16 -> Float32 members through the linear and the tiled body of the grouped kernel: one launch, then inside a recorded sequence"""
    import torch
    stream = int(torch.cuda.current_stream().cuda_stream)
    members = CC.group_rows(cell)
    for mode in ("group", "sequence"):
        with jit_mode(jit):
            caches = [{} for _ in members]
            dev = [tuple(to_device(a, c) for a in r.arrays) for r, c in zip(members, caches)]
            g = CC.build_group(members, dev)
            assert [m[0] for m in g.layout()] == [form] * len(members), g.layout()
            assert "f=prog" in g.describe() and "jit=%d" % jit in g.describe(), g.describe()
            torch.cuda.synchronize()
            if mode == "group":
                g.execute(stream)
            else:
                q = S.Sequence().add_group(g)
                q.run(1, stream)
                q.wait()
                del q
            torch.cuda.synchronize()
            for r, c in zip(members, caches):
                check(r, c, "%s %s jit=%d %s" % (cell, mode, jit, g.describe()))
            del g
