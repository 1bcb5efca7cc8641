"""GPU: groups recorded in sequences (smr_seq_add_group) -- K small maps as ONE kernel, replayed from ONE pre-built AQL packet, and
that one launch cut into block ranges over several hardware queues (csrc/smr_k_group.hip: GroupArgs::wg0).  Every result is compared
bit for bit with NumPy and with the same members run one by one through smr_mapreduce.

The scheduler cuts a launch only into ranges of at least 64 workgroups (csrc/smr_sched.cpp, unchanged), so the slicing case runs the
five members below together with small filler members that bring the grid to 4 x 64 workgroups and more."""
import functools
import gc
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import strided_jl_amd as S
from strided_jl_amd import _lib as L
from util import to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 256 * 4  # canonical indices per workgroup of the linear body (csrc/smr_group.h: GROUP_CHUNK)


def ident(x):
    return x


def sync():
    import torch
    torch.cuda.synchronize()


def cur_stream():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def field(info, key):
    for tok in info.split():
        if tok.startswith(key + "="):
            return tok.split("=", 1)[1]
    raise KeyError(key + " not in: " + info)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def hview(a):
    return S.StridedView(np.asfortranarray(a).copy(order="F"))


# (source shape, permutation, workgroups): the transposing body with ragged 32 x 32 tiles; with two tiles along one dim and an outer
# dim; the linear body on a tiny member; the linear body over two workgroups; four tiles
MEMBERS = [((17, 19), (1, 0), 1), ((33, 16, 2), (1, 0, 2), 4), ((3, 5, 4), (2, 0, 1), 1), ((CHUNK + 1,), (0,), 2), ((40, 40), (1, 0), 4)]
# fillers of the slicing case: 9 tiles / 10 chunks each, so that cuts at multiples of 8 fall inside members
FILL = [((96, 96), (1, 0), 9), ((9 * CHUNK + 5,), (0,), 10)]


def permute_calls(rng, specs):
    """(f, (destination, permuted source)) host calls and the NumPy results of permutedims! for `specs`."""
    calls, want = [], []
    for shp, perm, _ in specs:
        a = rng.standard_normal(shp)
        calls.append((ident, (hview(np.zeros(tuple(shp[i] for i in perm))), hview(a).permutedims(perm))))
        want.append(np.ascontiguousarray(np.transpose(a, perm)))
    return calls, want


class Case:
    """Members on the device as one group, with the results of the same calls issued one by one (smr_mapreduce) on private copies."""

    def __init__(self, calls, want):
        self.calls, self.want = calls, want
        self.cache = {}
        self.devs = [tuple(to_device(v, self.cache) for v in arrays) for _, arrays in calls]
        self.alone = []
        for f, arrays in calls:
            c2 = {}
            d2 = tuple(to_device(v, c2) for v in arrays)
            S._mapreduce_fuse_(f, None, None, arrays[0].size, d2)
            sync()
            self.alone.append(d2[0].toarray())
        self.built = [S.build_problem(f, None, None, arrays[0].size, dev, stream=cur_stream()) for (f, arrays), dev in zip(calls, self.devs)]
        self.group = L.Group([b[0] for b in self.built], keepalive=self.built)
        sync()

    def clear(self):
        for dev in self.devs:
            dev[0].parent.zero_()
        sync()

    def got(self):
        return [dev[0].toarray() for dev in self.devs]

    def check(self, note=""):
        for i, (x, w, y) in enumerate(zip(self.got(), self.want, self.alone)):
            assert same_bits(x, w), "member %d differs from NumPy %s" % (i, note)
            assert same_bits(x, y), "member %d differs from the call issued alone %s" % (i, note)

    def replay(self, seq, reps=1, stream=None):
        self.clear()
        seq.run(reps, cur_stream() if stream is None else stream)
        seq.wait()
        sync()


@functools.lru_cache(maxsize=None)
def five():
    calls, want = permute_calls(np.random.default_rng(31), MEMBERS)
    return Case(calls, want)


def sliced_specs():
    # the five members spread over the fillers: every cut of 2, 3 and 4 slices is inside some member (asserted from the layout)
    specs = []
    for i in range(14):
        specs += [FILL[0], FILL[1]]
        if i < len(MEMBERS):
            specs.append(MEMBERS[i])
    return specs


@functools.lru_cache(maxsize=None)
def filled():
    calls, want = permute_calls(np.random.default_rng(37), sliced_specs())
    return Case(calls, want)


@functools.lru_cache(maxsize=None)
def direct_available():
    """Does a sequence of one plain plan replay as AQL packets here?  (No: SMR_SEQ_DIRECT=0, a profiler, a failed direct path.)"""
    a = five().devs[0]
    X = S.StridedView(a[0].parent.clone(), a[0].size, a[0].strides, a[0].offset)
    q = S.Sequence().add(S.make_plan(ident, None, None, X.size, (X, a[0])))
    return field(q.info(), "backend") == "aql"


def assert_aql(info):
    """backend=aql, unless info() itself names scratch memory or the direct path is unavailable in this process."""
    if field(info, "backend") == "aql":
        return
    assert "scratch" in info or not direct_available(), "a group item replays through HIP for another reason: " + info


def test_layout_of_the_five_members():
    lay = five().group.layout()
    assert [r[2] for r in lay] == [m[2] for m in MEMBERS]
    assert [r[0] for r in lay] == [1, 1, 0, 0, 1]          # both bodies occur
    assert sum(r[2] for r in lay) >= 9


@pytest.mark.parametrize("queues", [1, 4])
@pytest.mark.parametrize("reps", [1, 3])
def test_replay_of_the_group_alone(reps, queues):
    c = five()
    q = S.Sequence().add_group(c.group)
    q.set("queues", queues)
    c.replay(q, reps)
    info = q.info()
    c.check(info)
    assert field(info, "items") == "1" and field(info, "groups") == "1", info
    assert_aql(info)
    if field(info, "backend") == "aql":
        assert field(info, "packets") == "1" and field(info, "queues") == "1", info   # one group = one packet


@pytest.mark.parametrize("slices", [2, 3, 4])
def test_one_group_cut_into_block_ranges(slices):
    c = filled()
    lay = c.group.layout()
    grid = lay[-1][1] + lay[-1][2]
    assert grid >= 64 * 4 and {r[0] for r in lay} == {0, 1}
    # the cuts (csrc/smr_sched.cpp: slice_range): ceil(grid / slices) rounded up to a multiple of 8
    per = ((grid + slices - 1) // slices + 7) & ~7
    cuts = [per * k for k in range(1, slices) if per * k < grid]
    firsts = {r[1] for r in lay}
    assert len(cuts) == slices - 1 and any(x not in firsts for x in cuts), (cuts, sorted(firsts))
    for x in cuts:  # ... and the cut member is in the table for the message
        assert any(r[1] <= x < r[1] + r[2] for r in lay)
    q = S.Sequence().add_group(c.group)
    q.set("slices", slices)
    c.replay(q, 2)
    info = q.info()
    c.check(info)
    assert_aql(info)
    if field(info, "backend") == "aql":
        assert field(info, "sliced") == "1" and field(info, "queues") == str(slices) and field(info, "packets") == str(slices), info
    # uncut, the same sequence gives the same arrays
    q.set("slices", 1)
    c.replay(q, 1)
    c.check("uncut")


def test_group_is_one_ordered_step_between_plans():
    """plan: member 2's input <- X';  the group;  plan: T <- member 2's destination.  Three replays, X changed in between."""
    import torch
    rng = np.random.default_rng(41)
    calls, want = permute_calls(rng, MEMBERS)
    c = Case(calls, want)
    dst2, src2 = c.devs[2]                      # src2 is the permuted view of member 2's input array of shape (3, 5, 4)
    inp = S.StridedView(src2.parent, (3, 5, 4), (1, 3, 15), 0)
    xs = [rng.standard_normal((4, 5, 3)) for _ in range(3)]
    X = to_device(hview(xs[0]))
    T = to_device(hview(np.zeros((4, 3, 5))))
    first = S.make_plan(ident, None, None, inp.size, (inp, X.permutedims((2, 1, 0))))
    last = S.make_plan(ident, None, None, T.size, (T, dst2))
    q = S.Sequence().add(first).add_group(c.group).add(last)
    assert q.components() == [0, 0, 0] and q.fences()[0] == [0, 1, 1]
    for r, x in enumerate(xs):
        X.parent.copy_(torch.from_numpy(np.asfortranarray(x).ravel(order="F").copy()))
        T.parent.zero_()
        c.clear()
        q.run(1, cur_stream())
        q.wait()
        sync()
        a2 = np.transpose(x, (2, 1, 0))         # what the first plan wrote into member 2's input
        assert same_bits(T.toarray(), np.ascontiguousarray(np.transpose(a2, (2, 0, 1)))), "replay %d: %s" % (r, q.info())
        for i, (g, w) in enumerate(zip(c.got(), c.want)):
            if i != 2:
                assert same_bits(g, w), (r, i)
    info = q.info()
    assert field(info, "items") == "3" and field(info, "groups") == "1", info
    assert_aql(info)


def test_complex_group_with_conj_and_constants():
    """ComplexF32, f = 2x + y with a conj (and transposed) x and a y that shares the destination's layout."""
    rng = np.random.default_rng(43)
    f = lambda x, y: 2 * x + y  # noqa: E731
    calls, want = [], []
    for shp in ((20, 18), (5, 7), (CHUNK + 6, 1), (33, 17)):
        x = (rng.standard_normal(shp[::-1]) + 1j * rng.standard_normal(shp[::-1])).astype(np.complex64)
        y = (rng.standard_normal(shp) + 1j * rng.standard_normal(shp)).astype(np.complex64)
        calls.append((f, (hview(np.zeros(shp, np.complex64)), hview(x).permutedims((1, 0)).conj(), hview(y))))
        want.append(np.complex64(2) * np.conj(x.T) + y)
    c = Case(calls, want)
    assert {r[0] for r in c.group.layout()} == {0, 1}
    q = S.Sequence().add_group(c.group)
    c.replay(q, 2)
    info = q.info()
    c.check(info + " | " + c.group.describe())
    assert_aql(info)


def test_runtime_compiled_f_replays_correctly():
    rng = np.random.default_rng(47)
    f = lambda x: x ** 2 + 1  # noqa: E731
    calls, want = [], []
    for shp, perm, _ in MEMBERS[:4]:
        a = rng.standard_normal(shp)
        calls.append((f, (hview(np.zeros(tuple(shp[i] for i in perm))), hview(a).permutedims(perm))))
        t = np.ascontiguousarray(np.transpose(a, perm))
        want.append(t * t + 1)
    c = Case(calls, want)
    q = S.Sequence().add_group(c.group)
    c.replay(q, 2)
    info = q.info()
    c.check(info + " | " + c.group.describe())
    assert field(info, "backend") in ("aql", "hip"), info


CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import test_gpu_seq_group as T
import strided_jl_amd as S
c = T.five()
q = S.Sequence().add_group(c.group)
c.replay(q, 2)
info = q.info()
c.check(info)
print("INFO", info)
print("DIGEST", T.digest(c.got()))
"""


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_hip_replay_in_a_child_process_without_the_direct_path():
    env = dict(os.environ, SMR_SEQ_DIRECT="0")
    r = subprocess.run([sys.executable, "-c", CHILD % (os.path.join(ROOT, "tests"), ROOT)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    info = [l for l in r.stdout.splitlines() if l.startswith("INFO")][0]
    assert "backend=hip" in info and "groups=1" in info and "SMR_SEQ_DIRECT=0" in info, info
    c = five()
    c.replay(S.Sequence().add_group(c.group), 2)
    c.check()
    assert [l for l in r.stdout.splitlines() if l.startswith("DIGEST")][0].split()[1] == digest(c.got()) == digest(c.want)


def test_sequence_keeps_its_group_alive_and_replays_on_a_library_owned_stream():
    """Eager direct launches on a stream of smr_stream_create write the group's inputs; the sequence (sole owner of the group by then)
    replays on that stream behind them."""
    rng = np.random.default_rng(53)
    calls, want0 = permute_calls(rng, MEMBERS)
    c = Case(calls, want0)
    q = S.Sequence().add_group(c.group)
    c.replay(q, 1)
    c.check("first replay, HIP stream")
    c.group = None                               # the sequence holds the only reference now
    gc.collect()
    fresh = [rng.standard_normal(shp) for shp, _, _ in MEMBERS]
    srcs = [to_device(hview(a)) for a in fresh]
    c.clear()
    st = S.Stream()
    try:
        before = S.get_option("eager_launches")
        with st:
            for (shp, perm, _), dev, s in zip(MEMBERS, c.devs, srcs):
                st_, n = [], 1
                for d in shp:
                    st_.append(n)
                    n *= d
                S.copy_(S.StridedView(dev[1].parent, shp, tuple(st_), 0), s)   # an eager launch writes the member's input array
            direct = S.get_option("eager_launches") - before
            q.run(2, st.handle)
            q.wait()
        sync()
        for i, ((shp, perm, _), a, dev) in enumerate(zip(MEMBERS, fresh, c.devs)):
            assert same_bits(dev[0].toarray(), np.ascontiguousarray(np.transpose(a, perm))), (i, direct, q.info())
        assert_aql(q.info())
    finally:
        st.close()
