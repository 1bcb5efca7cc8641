"""`with S.group():` as a property test on host views (no device): random programs of map calls whose operands are sub-views of a few
small parents, so that calls read and overwrite each other's outputs.  The launcher is stubbed (as in tests/test_group_host.py); the
recorded launches are replayed with the CPU oracle.
  (a) the members of one launch are order-independent: launches in order, the members of each launch in REVERSED order, give the parents
      the program gives call by call, bit for bit;
  (b) the library accepts every bucket the front forms (a refused bucket would silently run call by call);
  (c) with independent=True the front never defers a call whose destination view is a pending operand."""
import numpy as np

import group_cases as G
import strided_jl_amd as S
from strided_jl_amd import _lib as L
from strided_jl_amd.mapreduce import _view_id
from test_group_cases_host import byte_range, draw_view
from util import run_oracle

NPROG = 200
FS = [(G.ident, 1), (lambda a: a * 2, 1), (lambda a, b: a + b, 2)]


class Recorder(S.group):
    """`S.group` with the launcher stubbed out: records the deferred calls of every launch."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.launches = []

    def _launch(self, calls, stream):
        self.launches.append(list(calls))


def meets(a, b):
    return a[0] < b[1] and b[0] < a[1]


def program(seed):
    """(parents, their initial values, calls as (f, arrays)): 5-40 calls on random 1-d and 2-d sub-views of 3-4 parents of 48 elements.
    An input is the call's own destination (in place) or shares no byte range with it: a single call is well defined."""
    rng = np.random.default_rng([G.SEED_OFFSET, 91, seed])
    parents = [np.zeros(48) for _ in range(int(rng.integers(3, 5)))]
    init = [rng.integers(-8, 9, size=48).astype(np.float64) for _ in parents]
    calls, pool = [], []
    for _ in range(int(rng.integers(5, 41))):
        f, nin = FS[int(rng.integers(0, len(FS)))]
        shape = (int(rng.integers(1, 13)),) if rng.integers(0, 2) else (int(rng.integers(1, 5)), int(rng.integers(1, 5)))

        def view():
            same = [v for v in pool if v.size == shape]
            if same and rng.integers(0, 3) == 0:
                return same[int(rng.integers(0, len(same)))]   # an operand of an earlier call, exactly
            w = int(rng.integers(0, 48 - 24 + 1))                # else a view inside a window of 24 elements
            return draw_view(rng, parents[int(rng.integers(0, len(parents)))], w, w + 24, shape)

        dst = view()
        ins = []
        while len(ins) < nin:
            v = dst if rng.integers(0, 6) == 0 else view()
            if v is dst or not meets(byte_range(v), byte_range(dst)):
                ins.append(v)
        pool += [dst] + ins
        calls.append((f, (dst,) + tuple(ins)))
    return parents, init, calls


def reset(parents, init):
    for p, v in zip(parents, init):
        p[:] = v


def record(calls, independent):
    g = Recorder(independent=independent)
    for f, arrays in calls:
        assert g.defer(f, arrays[0].size, arrays)
    g.flush()
    assert sum(len(x) for x in g.launches) == len(calls)
    return g


def test_members_of_a_launch_are_order_independent_and_every_bucket_is_a_group():
    shared = buckets = 0
    for seed in range(NPROG):
        parents, init, calls = program(seed)
        g = record(calls, independent=False)
        reset(parents, init)
        for f, arrays in calls:
            run_oracle(f, None, None, arrays[0].size, arrays)
        want = [p.copy() for p in parents]
        reset(parents, init)
        for launch in g.launches:
            for c in reversed(launch):
                run_oracle(c.f, None, None, c.dims, c.arrays)
        for i, (p, w) in enumerate(zip(parents, want)):
            assert G.same_bits(p, w), "seed %d parent %d: %s" % (seed, i, [len(x) for x in g.launches])
        for launch in g.launches:  # (b): built, not executed
            built = [S.build_problem(c.f, None, None, c.dims, c.arrays, stream=0) for c in launch]
            try:
                L.Group([b[0] for b in built], False, keepalive=built)
            except L.UnsupportedOnDevice as e:
                raise AssertionError("seed %d: the library refuses a bucket of %d calls the front formed: %s" % (seed, len(launch), e))
            buckets += 1
            shared += len(launch) > 1
    assert shared >= NPROG and buckets > shared  # the programs do group: launches of several calls, and conflicts that flush


def test_independent_never_defers_a_write_to_a_pending_operand():
    deferred = 0
    for seed in range(NPROG):
        parents, init, calls = program(seed)
        g = Recorder(independent=True)
        for f, arrays in calls:
            assert g.defer(f, arrays[0].size, arrays)
            w = _view_id(arrays[0])
            for q in g.pending[:-1]:
                assert w not in [_view_id(a) for a in q.arrays], "seed %d: %s is written while a pending call uses it" % (seed, arrays[0])
            deferred += len(g.pending) > 1
        g.flush()
        assert sum(len(x) for x in g.launches) == len(calls)
    assert deferred >= NPROG
