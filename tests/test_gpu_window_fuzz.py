"""GPU: the windowed problems of tests/window_cases.py through every map kernel family, the WHOLE destination parent compared byte for byte.

Each case runs on fresh device copies in five modes: direct execution under store policy 0 (plain), 1 (non-temporal) and 2 (write-through),
and as a recorded sequence uncut and cut in two block ranges (where a recorded launch picks the write-through policy by itself).  After
each mode the destination's whole root allocation must hold NumPy's result inside the view and its first contents outside, and every
input root must be unchanged.  The device plan must be the family and kernel variant the host plan of the same case is
(tests/test_window_cases_host.py), the paths reached are counted from the device plans' describe() against the same minimums, and the
sequences must have released launches by write-through for TILED vector cases and ORBIT cases."""
import collections

import numpy as np
import pytest

import strided_jl_amd as S
import window_cases as W
from util import to_device

pytestmark = pytest.mark.gpu
COUNTS = W.new_counter()
SELF_RELEASED = collections.Counter()
MODES = ("nt_store=0", "nt_store=1", "nt_store=2", "sequence", "sequence slices=2")


def field(info, key):
    for tok in info.split():
        if tok.startswith(key + "="):
            return tok.split("=", 1)[1]
    raise KeyError(key + " not in: " + info)


def run_case(case, counts, released):
    import torch
    stream = int(torch.cuda.current_stream().cuda_stream)
    host_plan = case.plan()
    host_desc = host_plan.describe()
    host_plan.close()
    dkey = case.arrays[0].parent.ctypes.data
    for mode in MODES:
        cache = {}
        dev = tuple(to_device(a, cache) for a in case.arrays)
        old = S.get_option("nt_store")
        info = ""
        plan = q = None
        try:
            if mode.startswith("nt_store="):
                S.set_option("nt_store", int(mode[-1]))
            plan = case.plan(dev)
            desc = plan.describe()
            assert W.variant_key(desc) == W.variant_key(host_desc), "%s: device plan [%s], host plan [%s]" % (case.name, desc, host_desc)
            torch.cuda.synchronize()
            if mode.startswith("nt_store="):
                plan.execute(stream)
            else:
                q = S.Sequence().add(plan)
                q.set("slices", 2 if mode.endswith("slices=2") else 1)
                q.run(1, stream)
                q.wait()
                info = q.info()
            torch.cuda.synchronize()
        finally:
            S.set_option("nt_store", old)
            if q is not None:
                del q           # (the sequence goes before the plan it replays)
            if plan is not None:
                plan.close()    # with its lane and order tables in device memory
        case.desc = "%s | %s %s" % (desc, mode, info.split(" last_replay")[0])
        msg = case.mismatch(cache[dkey].cpu().numpy()) or case.inputs_changed({k: t.cpu().numpy() for k, t in cache.items() if k != dkey})
        assert msg is None, msg
        if mode == "sequence":
            W.count(counts, desc)
            # (a sequence with a kernel that needs scratch memory replays through the HIP runtime, backend=hip: nothing is self-released there)
            if field(info, "backend") == "aql" and int(field(info, "self_released")) > 0:
                ps = W.paths(desc)
                released.update(p for p in ("tiled vec>1", "family=orbit") if p in ps)
        if mode == "sequence slices=2" and field(info, "backend") == "aql" and int(field(info, "sliced")) > 0:
            released["cut in two"] += 1


@pytest.mark.parametrize("recipe", sorted(W.RECIPES))
def test_windowed_problems_leave_the_parent_alone_under_every_store_policy(recipe):
    counts, released = W.new_counter(), collections.Counter()
    n = 0
    for case in W.cases(recipe):
        run_case(case, counts, released)
        n += 1
    COUNTS.update(counts)
    SELF_RELEASED.update(released)
    print("[window fuzz] %s: %d cases x %d modes: %s | self-released in a sequence: %s" % (
        recipe, n, len(MODES), ", ".join("%s x%d" % kv for kv in sorted(counts.items())), dict(released)))


def test_every_path_ran_on_the_device_often_enough():
    """runs after the recipes (file order), and fails when they did not run"""
    print("[window fuzz] total: " + ", ".join("%s x%d" % kv for kv in sorted(COUNTS.items())) + " | self-released in a sequence: %s" % dict(SELF_RELEASED))
    W.check_minimums(COUNTS)
    # the write-through store policy ran on ragged, windowed data: launches recorded for a sequence that released themselves
    assert SELF_RELEASED["tiled vec>1"] >= 8 and SELF_RELEASED["family=orbit"] >= 8, dict(SELF_RELEASED)
    # slices = 2 did cut launches in two block ranges: the scheduler cuts launches of 128 workgroups and more, which the 24 cases of
    # 32^4 elements in 4096-element tiles (256 workgroups) of the recipe tiled_orbits are
    assert SELF_RELEASED["cut in two"] >= 8, dict(SELF_RELEASED)
