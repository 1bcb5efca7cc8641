"""CPU: the programs of tests/seq_program_cases.py on NumPy parents -- what the corpus reaches (counted from describe()), and the replay
schedule of every program against the independent checker tests/sched_model.py: the components and acquire flags the library derives
from the plans (smr_seq_components, smr_seq_fences) must be those of the operands' byte ranges, and the schedule of those byte ranges
(smr_debug_seq_schedule) must pass every rule under the knobs the GPU test uses.  The partials of reductions and split contractions
exist only on a device; tests/test_gpu_seq_program.py asserts what they add."""
import collections

import pytest

import sched_model as M
import seq_program_cases as P
import window_cases as W
from test_seq_schedule import ex, sched

QUEUES = (1, 4, 8)
SLICES = (-1, 1, 3)


def host(prog):
    parents = [a.copy() for a in prog.initial]
    return parents, P.Recorded(prog, parents, lambda a: a.ctypes.data)


def executions(prog, parents, rec):
    """The steps as synthetic executions: byte ranges from the operands, grid from describe(), two launches where partials are folded."""
    out = []
    for s, (kind, x, _), (rd, wr) in zip(prog.steps, rec.items, P.footprints(prog, lambda i: parents[i].ctypes.data)):
        grid = int(W.token(x.describe(), "grid") or 64)
        out.append(ex(rd, wr, nlaunch=2 if s.kind == "part" else 1, grid=grid, sliceable=True, same_as=s.twin))
    return out


@pytest.fixture(scope="module")
def corpus():
    return [(P.program(seed),) + host(P.program(seed)) for seed in range(P.PROGRAMS)]


def test_the_corpus_reaches_every_kind_and_family(corpus):
    kinds = collections.Counter()
    assert len(corpus) >= 8
    for prog, parents, rec in corpus:
        assert 6 <= len([s for s in prog.steps if not s.shift and s.kind != "big"]) <= 12
        for s, (kind, x, _) in zip(prog.steps, rec.items):
            kinds[s.kind] += 1
            d = x.describe()
            if kind == "plan":
                assert W.family(d) == P.FAMILY[s.kind], (prog, s.kind, d)
            if s.kind == "part":
                assert "fold=second-launch" in d, d
            if s.kind == "split":
                assert "kparts=2" in d, d
            if s.kind == "generic":
                assert all(min(abs(t) for t in o.strides) > 1 for o in s.ops), s.ops   # stepped everywhere
            if kind == "group":
                assert len(x.layout()) == 3 and {r[0] for r in x.layout()} <= ({2} if s.kind == "mulgroup" else {0, 1}), x.layout()
    short = {k: kinds[k] for k in P.KINDS if kinds[k] < 3}
    assert not short, (short, dict(kinds))
    assert kinds["big"] >= 2, dict(kinds)


def test_numpy_keeps_every_value_small_and_every_pad_unchanged(corpus):
    for prog, _, _ in corpus[:4]:
        out = P.run_numpy(prog, 3)
        touched = [set() for _ in range(4)]
        for s in prog.steps:
            for m in s.leaves():
                touched[m.ops[0].par].update(P.index_of(m.ops[0]).ravel().tolist())
        for i, (a, b) in enumerate(zip(out, prog.initial)):
            assert abs(a).max() <= (4 if i < 3 else 8192 * 4), (prog, i, abs(a).max())
            same = a == b
            assert same.sum() >= a.size - len(touched[i]) and not same.all() or not touched[i], (prog, i)
            assert not (a == 0).all() and (a == a.round()).all()


def test_components_and_fences_follow_the_operands(corpus):
    several = 0
    for prog, parents, rec in corpus:
        execs = executions(prog, parents, rec)
        q = rec.sequence()
        m = M.conflict_matrix(execs)
        comp = q.components()
        assert comp == M._closure(len(execs), m), (prog, comp)
        acq, fp, resident = q.fences()
        assert acq == [int(any(M._any_hit(w["wr"], e["rd"]) for w in execs)) for e in execs], prog
        assert fp == M.union_bytes(execs) and resident, (prog, fp)
        several += len(set(comp)) >= 2
    assert several >= 3, several


def test_every_schedule_passes_the_checker(corpus):
    cut = 0
    for prog, parents, rec in corpus:
        execs = executions(prog, parents, rec)
        for queues in QUEUES:
            for slices in SLICES:
                knobs = dict(max_queues=queues, slices=slices)
                r = sched(execs, **knobs)
                assert M.check(execs, r, **knobs) == [], (prog, knobs)
                if (queues, slices) == (8, 3):
                    cut += r["nsliced"] >= 1
    assert cut >= 2, cut
