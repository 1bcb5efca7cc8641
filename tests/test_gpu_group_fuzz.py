"""GPU: the recipes of tests/group_cases.py through csrc/smr_k_group.hip -- both bodies, every natively compiled functor, the interpreted
and the runtime-compiled f, bit copies of every width, integer arithmetic, mixed types, member counts up to a few thousand.
Each group runs as ONE launch.  The WHOLE parent of every destination is read back: it must equal, bit for bit, the host parent after
the CPU oracle wrote the member into it (the result, and not one byte outside the member changed), and every member must equal the
same call issued alone.  Where the device's arithmetic may round differently from the host's (complex products, exp / sin / tanh) the
member is compared norm-wise within util.rtol, as tests/test_gpu_fuzz_families.py does, and the rest of the parent still bit for bit.
What each recipe reaches is asserted without a device in tests/test_group_cases_host.py."""
import numpy as np
import pytest

import group_cases as G
import strided_jl_amd as S
from util import host_flat, to_device

pytestmark = pytest.mark.gpu


def run_case(c):
    whole = []
    with G.options(c):
        g, want, got, alone = G.run_group(c.calls, ref=c.ref, whole=whole)
    d, lay = g.describe(), g.layout()
    assert "family=group" in d and "members=%d " % len(c.calls) in d and "f=%s " % c.fname in d and "jit=%d" % c.jit in d, (c, d)
    assert [(r[0], r[2], r[3]) for r in lay] == [(m["form"], m["wgs"], m["rank"]) for m in c.info], c
    for i in range(len(c.calls)):  # every member, not a sample
        G.judge(c, i, want[i], got[i], alone[i], whole[i])


def run_recipe(name, dt=None):
    cases = G.recipe(name, dt)
    assert cases
    for c in cases:
        run_case(c)


@pytest.mark.parametrize("dt", G.FLOATS)
def test_linear(dt):
    run_recipe("linear", dt)


@pytest.mark.parametrize("dt", G.FLOATS)
def test_transposing(dt):
    run_recipe("transposing", dt)


def test_tmin():
    run_recipe("tmin")


@pytest.mark.parametrize("dt", G.FLOATS)
def test_functors(dt):
    native = [c for c in G.recipe("functors", dt) if c.fname != "prog"]
    assert len(native) == (10 if G.is_complex(dt) else 11)
    for c in native:
        run_case(c)


@pytest.mark.parametrize("which", ["prog/float64/jit", "math/float64/jit", "prog/float64/interpreted"])
def test_functor_programs(which):
    (c,) = [c for c in G.recipe("functors", np.float64) if c.name == "functors/" + which]
    run_case(c)


def test_bitcopy():
    run_recipe("bitcopy")


@pytest.mark.parametrize("dt", [np.int32, np.int64, np.uint8])
def test_integer(dt):
    run_recipe("integer", dt)


@pytest.mark.parametrize("i", range(3))
def test_mixed(i):
    cases = G.recipe("mixed")
    assert len(cases) == 3
    run_case(cases[i])


@pytest.mark.parametrize("K", G.COUNTS)
def test_counts(K):
    for c in G.counts(which=(K,)):
        run_case(c)


def test_sliced_replays_equal_the_eager_group():
    """The carry-heavy linear members and the ragged transposing members with outer dims, recorded with Sequence.add_group and replayed
    as 2, 3 and 4 block ranges: cuts fall strictly inside members of both bodies, and every replay leaves what the eager group left."""
    from test_gpu_seq_group import assert_aql, field
    c, cuts = G.sliced()
    cache = {}
    devs = [tuple(to_device(a, cache) for a in arrays) for f, arrays in c.calls]
    parents = [host_flat(arrays[0])[0] for f, arrays in c.calls]          # host parents: the destinations' initial contents
    tensors = [cache[p.ctypes.data] for p in parents]
    built = [S.build_problem(f, None, None, arrays[0].size, dev, stream=G.cur_stream()) for (f, arrays), dev in zip(c.calls, devs)]
    g = G.L.Group([b[0] for b in built], keepalive=built)
    lay = g.layout()
    assert lay[-1][1] + lay[-1][2] == G.SEQ_GRID >= 256
    inside = {0: 0, 1: 0}
    for s in (2, 3, 4):
        hit = [r for x in cuts[s] for r in lay if r[1] < x < r[1] + r[2]]
        assert len(cuts[s]) == s - 1 and hit, (s, cuts[s])
        for r in hit:
            inside[r[0]] += 1
    assert inside[0] >= 1 and inside[1] >= 1, inside   # a cut strictly inside a linear member, one inside a transposing member
    G.sync()
    g.execute(G.cur_stream())
    G.sync()
    eager = [t.cpu().numpy() for t in tensors]
    for i, (f, arrays) in enumerate(c.calls):  # the eager group itself against the oracle, whole parents
        G.run_oracle(f, None, None, arrays[0].size, arrays)
        assert G.same_bits(eager[i], parents[i]), (i, c.info[i])
    q = S.Sequence().add_group(g)
    for s in (2, 3, 4):
        for t in tensors:
            t.fill_(-1.0)  # every destination parent overwritten: the replay has to write each member again
        G.sync()
        q.set("slices", s)
        q.run(1, G.cur_stream())
        q.wait()
        G.sync()
        info = q.info()
        assert_aql(info)
        if field(info, "backend") == "aql":
            assert field(info, "sliced") == "1" and field(info, "queues") == str(s) and field(info, "packets") == str(s), info
        for i, (t, (f, arrays)) in enumerate(zip(tensors, c.calls)):
            got = t.cpu().numpy()
            idx = G.element_index(arrays[0], host_flat(arrays[0])[1]).ravel()
            outside = np.ones(got.shape, dtype=bool)
            outside[idx] = False
            assert G.same_bits(got[idx], eager[i][idx]), "slices=%d member %d %s: %s" % (s, i, c.info[i], info)
            assert np.all(got[outside] == -1.0), "slices=%d member %d %s wrote outside its destination: %s" % (s, i, c.info[i], info)
