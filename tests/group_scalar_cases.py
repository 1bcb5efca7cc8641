"""Runner and member recipes for grouped launches with per-member scalars (SMR_GROUP_MEMBER_SCALARS), shared by
tests/test_gpu_group_scalars.py.  Like group_cases.run_group, which cannot pass the flag: every member runs alone on private copies
taken beforehand, then the group runs as ONE launch, then the oracle evaluates each member's own f on the host arrays.  Member i's
scalars are a function of i (alpha(i) = 1 + i/8, beta(i) = 2 - i/16: exact in binary), so a wrong row of the constant table shows
in the result.  Nothing here imports torch at import time."""
import contextlib

import numpy as np

import strided_jl_amd as S
from strided_jl_amd import _lib as L
import group_cases as G
from util import host_flat, run_oracle, rtol, to_device

fn = S.fn
CHUNK = G.CHUNK


def real_of(dt):
    return np.float32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64


def alpha(i, dt=np.float64):
    return real_of(dt)(1 + i / 8)


def beta(i, dt=np.float64):
    return real_of(dt)(2 - i / 16)


# the lambda forms csrc/smr_canon.cpp recognises, as factories over the member's scalars: name -> (inputs, scalars, factory, NumPy stand-in)
FUNCTORS = {
    "scale": (1, 1, lambda a: lambda x: x * a, None),
    "sym": (2, 1, lambda a: lambda x, y: (x + y) / a, None),
    "axpy": (2, 1, lambda a: lambda x, y: a * x + y, None),
    "axpby": (2, 2, lambda a, b: lambda x, y: a * x + b * y, None),
    "expr5": (1, 1, lambda a: lambda x: x * fn.exp(a * x) + fn.sin(x * x), lambda a: lambda x: (x * np.exp(a * x) + np.sin(x * x)).astype(x.dtype)),
}

# (source shape, permutation): one element; a small plain box; the transposing body at GROUP_TMIN; just below it (linear body, transposed
# input); ragged tiles; two workgroups of the linear body; rank 5 reversed; two tiled dims with an outer dim
SPECS = [((1,), (0,)), ((5, 7), (0, 1)), ((16, 16), (1, 0)), ((15, 17), (1, 0)), ((33, 31), (1, 0)), ((CHUNK + 1,), (0,)), ((4,) * 5, (4, 3, 2, 1, 0)),
         ((40, 36, 3), (1, 0, 2))]
FORMS = [0, 0, 1, 0, 1, 0, 0, 1]
WGS = [1, 1, 1, 1, 2, 2, 1, 4 * 3]


def member(rng, shp, perm, dt, nin, ddt=None, inplace=False, conj=False):
    """(destination, input 0 = a permuted view of a fresh array, further inputs laid out like the destination).  The destination is a
    view into a padded parent filled with a pattern (group_cases.dest); inplace: it is its own last input."""
    x = G.hview(G.values(rng, shp, dt)).permutedims(perm)
    if conj:
        x = x.conj()
    dims = x.size
    d = G.dest(rng, dims, ddt or dt)
    if inplace:
        flat, _ = host_flat(d)
        flat[:] = G.values(rng, flat.shape, ddt or dt)  # data of the usual magnitude instead of the pattern: it is read
    ins = [x] + [d if inplace and k == nin - 1 else G.hview(G.values(rng, dims, dt)) for k in range(1, nin)]
    return (d,) + tuple(ins)


@contextlib.contextmanager
def option(name, value):
    old = S.get_option(name)
    S.set_option(name, value)
    try:
        yield
    finally:
        S.set_option(name, old)


class Run:
    """What one group left behind: per member the oracle's (or the stand-in's) result, the group's, the result of the call issued
    alone, and the destination's whole parent before and after with the indices of the member's elements in it."""

    def __init__(self, calls, member_scalars=True, independent=False, refs=None, execute=True):
        self.calls = calls
        self.cache, self.devs = {}, []
        for f, arrays in calls:
            self.devs.append(tuple(to_device(a, self.cache) for a in arrays))
        self.before = [host_flat(arrays[0])[0].copy() for f, arrays in calls]
        self.alone = []
        for f, arrays in calls:  # the same call alone, through the existing smr_mapreduce path, on private copies taken before anything ran
            c2 = {}
            d2 = tuple(to_device(a, c2) for a in arrays)
            S._mapreduce_fuse_(f, None, None, arrays[0].size, d2)
            G.sync()
            self.alone.append(d2[0].toarray())
        self.built = [S.build_problem(f, None, None, arrays[0].size, dev, stream=G.cur_stream()) for (f, arrays), dev in zip(calls, self.devs)]
        self.group = L.Group([b[0] for b in self.built], independent, keepalive=self.built, member_scalars=member_scalars)
        G.sync()
        self.compiles = 0
        if execute:
            before, c0 = S.get_option("launches"), S.get_option("jit_compiles")
            self.group.execute(G.cur_stream())
            assert S.get_option("launches") == before + 1
            G.sync()
            self.compiles = S.get_option("jit_compiles") - c0
        self.got = self.results()
        if refs is None:
            self.want = [run_oracle(f, None, None, arrays[0].size, arrays) for f, arrays in calls]
        else:
            self.want = [ref(*[a.toarray() for a in arrays[1:]]) for ref, (f, arrays) in zip(refs, calls)]
        self.idx = [G.element_index(arrays[0], host_flat(arrays[0])[1]) for f, arrays in calls]

    def results(self):
        return [dev[0].toarray() for dev in self.devs]

    def parent(self, i):
        """The whole device parent of member i's destination, as it is now."""
        flat, _ = host_flat(self.calls[i][1][0])
        return self.cache[flat.ctypes.data].cpu().numpy()

    def judge(self, exact=True, np_truth=None):
        """Every member three ways: bit for bit with the call issued alone; with the oracle (bit for bit when `exact`, else within
        util.rtol norm-wise); and its whole parent byte for byte -- the member as the call alone wrote it, every other element untouched."""
        for i, (f, arrays) in enumerate(self.calls):
            msg = "member %d of %s, destination %s" % (i, self.group.describe(), arrays[0].size)
            got, want, alone = self.got[i], np.asarray(self.want[i]), self.alone[i]
            assert got.dtype == want.dtype == np.dtype(arrays[0].dtype) and got.shape == want.shape, msg
            assert G.same_bits(got, alone), msg + ": differs from the call issued alone"
            if exact:
                assert G.same_bits(got, want), msg + ": differs from the oracle"
            else:
                x, y = got.astype(np.complex128).ravel(), want.astype(np.complex128).ravel()
                assert np.linalg.norm(x - y) <= rtol(arrays[0].dtype) * max(np.linalg.norm(x), np.linalg.norm(y), 1e-300), msg + ": not within rtol of the oracle"
            if np_truth is not None:
                assert G.same_bits(got, np_truth[i]), msg + ": differs from NumPy"
            expect = self.before[i].copy()
            expect[self.idx[i].ravel()] = alone.ravel()
            assert G.same_bits(self.parent(i), expect), msg + ": the destination's whole parent differs (padding or non-member elements changed?)"
