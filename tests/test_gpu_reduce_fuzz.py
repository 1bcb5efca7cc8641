"""GPU: the windowed, order-independent reduction problems of tests/reduce_fuzz_cases.py, the WHOLE destination parent compared bit for bit.

Every case (checked on the CPU oracle by test_reduce_fuzz_host.py) runs on device copies of its parents:
  * one execution of its plan on the current stream;
  * a second execution of the same plan onto a re-uploaded destination -- the partials buffer is reused, and the arrival counters of an
    in-launch fold must have been left at zero by the workgroup that folded;
  * two more executions onto the same destination, without a re-upload: three applications, against expected_parent(times=3) -- initop =
    nothing accumulates, scale multiplies what the call before left;
  * a recorded Sequence of the plan replayed twice, on one queue and with the default number, against expected_parent(times=2).
After each, the destination's whole parent must hold the expected elements and the byte 0xA5 everywhere else.  The device plan must be the
plan the host made for the same case (family, form, lanes, cut, vector width, fold form: describe()), and the cells of the coverage table
are counted again from the device plans.  No case is skipped: the last test asserts that as many cases ran as the table has."""
import collections

import numpy as np
import pytest

import reduce_fuzz_cases as RF
import strided_jl_amd as S
from reduce_fuzz_cases import F, GROUPS, host_describe, with_options

pytestmark = pytest.mark.gpu

REACHED = collections.defaultdict(list)   # cell -> types of the cases that reached it on the device
EXACT_TX = set()
RAN = collections.Counter()


def cur():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def cuda(a):
    import torch
    if a.dtype == np.bool_:
        return torch.from_numpy(a.view(np.uint8).copy()).cuda().view(torch.bool)
    return torch.from_numpy(a.copy()).cuda()


def download(t):
    import torch
    if t.dtype == torch.bool:
        return t.view(torch.uint8).cpu().numpy().view(np.bool_)
    return t.cpu().numpy()


def run_case(case):
    import torch
    host_desc = host_describe(case)
    arrs = RF.views(case, S, cuda)
    dest = arrs[0].parent
    fresh = cuda(case.dest.parent)

    def go():
        plan = S.make_plan(F[case.f], case.op, case.initop, case.dims, arrs)
        desc = plan.describe()
        assert RF.plan_key(desc) == RF.plan_key(host_desc), "%s: device plan [%s], host plan [%s]" % (case.name, desc, host_desc)

        def check(what, times):
            torch.cuda.synchronize()
            err = case.mismatch(download(dest), times)
            assert err is None, "%s: %s [%s] %s" % (what, err, desc, case.note)

        plan.execute(cur())
        check("first execution", 1)
        dest.copy_(fresh)
        plan.execute(cur())
        check("second execution of the plan, destination uploaded again", 1)
        plan.execute(cur())
        plan.execute(cur())
        check("three executions onto one destination", 3)
        for queues in (1, None):
            dest.copy_(fresh)
            torch.cuda.synchronize()
            q = S.Sequence().add(plan)
            if queues is not None:
                q.set("queues", queues)
            q.run(2, cur())
            q.wait()
            check("recorded sequence replayed twice (queues: %s)" % (queues or "default"), 2)
            del q   # (the sequence goes before the plan it replays)
        plan.close()
        return desc

    desc = with_options(case, go)
    for c in RF.cells(desc, case):
        REACHED[c].append(case.type)
        if c == "col:exact":
            EXACT_TX.add(RF.token(desc, "tx").split("(")[0])


@pytest.mark.parametrize("recipe,t", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_reductions_are_exact_on_windowed_operands(recipe, t):
    n = 0
    for case in RF.cases(recipe, t):
        run_case(case)
        n += 1
    RAN[(recipe, t)] = n
    print("[reduce fuzz] %s %s: %d cases x 5 checks" % (recipe, t, n))


def test_every_cell_was_reached():
    """runs after the groups (file order), and fails when they did not all run: no case of the table may be left out"""
    print("[reduce fuzz] cells on the device: " + ", ".join("%s x%d" % (c, len(v)) for c, v in sorted(REACHED.items())))
    print("[reduce fuzz] exact lane maps, TX: " + " ".join(sorted(EXACT_TX, key=int)))
    assert sum(RAN.values()) == RF.table_size(), (sum(RAN.values()), RF.table_size())
    missing = sorted(set(RF.CELLS) - set(REACHED))
    assert not missing, missing
    if RF.SEED_OFFSET == 0:   # the counts test_reduce_fuzz_host.py asserts of the host plans, of the device plans
        RF.check_cells(REACHED, EXACT_TX)
