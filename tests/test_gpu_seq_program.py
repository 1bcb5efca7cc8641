"""GPU: whole programs through recorded sequences (csrc/smr_seq.cpp) -- the seeded programs of tests/seq_program_cases.py, 6-12 steps
of every kernel family, two-launch reductions, split contractions recorded twice with a rebound destination, map groups and
contraction groups, over windows of four padded parents.  Each program is replayed under queues 1 / 4 / 8, slices -1 / 1 / 3 and 1 / 3
replays; after each run the WHOLE of every parent is compared byte for byte with NumPy executing the list in order and with the same
plans executed one by one on a plain HIP stream.  The values are small integers and every sum is exact in any order
(seq_program_cases), so any order the replay scheduler may legally choose gives the same bits, and an order it may not choose does not.

tests/test_seq_program_host.py checks the same programs' schedules without a device; what only a device knows -- the partials of a
prepared plan are part of its footprint -- is asserted here."""
import functools

import numpy as np
import pytest

import seq_program_cases as P
from test_seq_schedule import ex, sched

pytestmark = pytest.mark.gpu

QUEUES = (1, 4, 8)
SLICES = (-1, 1, 3)
REPLAYS = (1, 3)


def stream():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def sync():
    import torch
    torch.cuda.synchronize()


def field(info, key):
    for tok in info.split():
        if tok.startswith(key + "="):
            return tok.split("=", 1)[1]
    raise KeyError(key + " not in: " + info)


class Device:
    """A program on the device: its parents, their first contents, the plans over them."""

    def __init__(self, prog):
        import torch
        self.prog = prog
        self.first = [torch.from_numpy(a).cuda() for a in prog.initial]
        self.parents = [t.clone() for t in self.first]
        self.rec = P.Recorded(prog, self.parents, lambda t: t.data_ptr(), stream())
        sync()

    def reset(self):
        for t, f in zip(self.parents, self.first):
            t.copy_(f)
        sync()

    def mismatch(self, want, note):
        """None when every parent holds exactly the bytes of `want`, else what differs first."""
        for i, (t, w) in enumerate(zip(self.parents, want)):
            g = t.cpu().numpy()
            ne = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
            if ne.size:
                e = int(ne[0])
                writers = [(k, s.kind) for k, s in enumerate(self.prog.steps) for m in s.leaves() if m.ops[0].par == i and P.extent(m.ops[0])[0] <= e <= P.extent(m.ops[0])[1]]
                return "%s parent %d: %d elements differ, first %d: got %r want %r, started as %r; steps writing around it %s | %s" % (
                    self.prog, i, ne.size, e, g[e], w[e], self.prog.initial[i][e], writers, note)
        return None


@functools.lru_cache(maxsize=None)
def expected(seed, reps):
    return P.run_numpy(P.pinned() if seed < 0 else P.program(seed), reps)


def replay(d, q, reps):
    d.reset()
    q.run(reps, stream())
    q.wait()
    sync()


# ---- the pinned chain ------------------------------------------------------------------------------------------------------------------
def test_the_pinned_chain_as_real_plans():
    """The five executions of tests/test_seq_schedule_fuzz.py: FIVE on one queue.  Before the barrier rule was closed, execution 0 of a
    replay went out free behind execution 3 of the previous one, which writes what it reads.  This test passes with the unsound bits
    too: inside one queue consecutive dispatches mostly run back to back on this hardware (profiles/r04_overlap.txt), so the overlap
    AQL allows is not observed; the device-free property test is the detector.  Here the closed bits are what the packets carry, and
    the results stay those of in-order execution."""
    prog = P.pinned()
    d = Device(prog)
    q = d.rec.sequence()
    q.set("queues", 1)
    for reps in (1, 2, 9):
        replay(d, q, reps)
        info = q.info()
        assert d.mismatch(expected(-1, reps), "%d replays | %s" % (reps, info)) is None
    assert field(info, "backend") == "aql", info
    execs = [ex(rd, wr) for rd, wr in P.footprints(prog, lambda i: d.parents[i].data_ptr())]
    bits = [p[5] for p in sched(execs, max_queues=1)["queues"][0]]
    assert bits == [1, 1, 0, 1, 0]
    assert field(info, "queues") == "1" and field(info, "packets") == "5", info
    assert (int(field(info, "ordered")), int(field(info, "unordered"))) == (sum(bits), len(bits) - sum(bits)), info
    d.reset()
    for _ in range(2):
        d.rec.execute(stream())
    sync()
    assert d.mismatch(expected(-1, 2), "one by one on a HIP stream") is None


# ---- programs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(P.PROGRAMS))
def test_program(seed):
    prog = P.program(seed)
    d = Device(prog)
    for reps in REPLAYS:                      # the same plans one by one on a plain HIP stream
        d.reset()
        for _ in range(reps):
            d.rec.execute(stream())
        sync()
        assert d.mismatch(expected(seed, reps), "one by one on a HIP stream, %d times" % reps) is None
    q = d.rec.sequence()
    aql = 0
    for queues in QUEUES:
        for slices in SLICES:
            q.set("queues", queues)
            q.set("slices", slices)
            for reps in REPLAYS:
                replay(d, q, reps)
                info = q.info()
                assert d.mismatch(expected(seed, reps), "queues %d slices %d replays %d | %s" % (queues, slices, reps, info)) is None
            if field(info, "backend") == "aql":
                aql += 1
                assert int(field(info, "queues")) <= queues, info
                if queues == 1:
                    assert field(info, "sliced") == "0", info
    assert aql == len(QUEUES) * len(SLICES) or "scratch" in info, info
    if "big" in prog.kinds():
        # slices = 3 for every component cuts nothing when the components that can be cut want more queues than there are; asked for
        # the transposing copy over 32^4 alone (grid 256 >= 64 * 3), the cut is certain: 3 queues for it, one for each other component
        big = q.components()[prog.kinds().index("big")]
        assert len(set(q.components())) + 2 <= 8
        q.set("queues", 8)
        q.set("slices", 1)
        q.set("slices:%d" % big, 3)
        for reps in REPLAYS:
            replay(d, q, reps)
            info = q.info()
            assert d.mismatch(expected(seed, reps), "the big step alone in 3 slices, replays %d | %s" % (reps, info)) is None
        if field(info, "backend") == "aql":
            assert field(info, "sliced") == "1" and int(field(info, "queues")) >= 3, info
    # what only a device knows: prepared, a split contraction's partials belong to its footprint, so the plan recorded twice with its
    # destination rebound is ONE component, although the two destinations are disjoint and the inputs are only read
    comp = q.components()
    for i, s in enumerate(prog.steps):
        if s.twin is not None:
            assert comp[i] == comp[s.twin], (prog, i, comp)
