"""Randomised parity aimed at the FAST kernel families: the generic fuzz of
tests/test_gpu_fuzz.py draws small boxes and almost always lands in GENERIC / small STREAM.  Here every
recipe is built to select one family -- STREAM (flat and strided rows), TILED (1024- and 4096-element tiles,
ragged tiles, reversed dims = wide offsets, persistent form, orbit-major order), ORBIT, GENERIC, REDUCE_ALL,
REDUCE_PART (ROW / COL / general, split reductions) -- at sizes of 10^5..2*10^6 elements, four element types
(Float32, Float64, ComplexF32, ComplexF64), NaN-carrying min / max.  HIP path vs the CPU oracle on identical
inputs; + - * / maps of reals and copies / sums of complex numbers bit for bit, the rest within the reference's tolerance.  The families actually hit are
counted from smr_plan_describe and printed (>= 200 problems per family)."""
import collections
import os
import sys

import numpy as np
import pytest

import oraclelib
import strided_jl_amd as S
from test_gpu_fuzz import EXPRS, _random_view, bitwise, cx_exact, dview
from util import fview, rtol

pytestmark = pytest.mark.gpu
fn = S.fn
TYPES = [np.float32, np.float64, np.complex64, np.complex128]
COUNTS = collections.Counter()


def _data(rng, T):
    def data(shape):
        x = rng.random(shape) + 0.25
        if np.issubdtype(np.dtype(T), np.complexfloating):
            x = x + 1j * (rng.random(shape) - 0.5)
        return np.asfortranarray(x.astype(T))
    return data


def _perm_view(rng, mk, data, dims, reverse=False, keep0=False):
    """dense parent with a random dim permutation (unit stride lands on a random dim); optionally reversed dims;
    keep0: dim 0 stays in front (a short common unit axis with different continuation dims behind it)"""
    N = len(dims)
    perm = [int(q) for q in rng.permutation(N)]
    if keep0:
        perm = [0] + [1 + int(q) for q in rng.permutation(N - 1)]
    pshape = [0] * N
    for i in range(N):
        pshape[perm[i]] = dims[i]
    V = mk(data(tuple(pshape))).permutedims(tuple(perm))
    if reverse:
        idx = [slice(None, None, -1) if rng.integers(0, 2) else slice(None) for _ in range(N)]
        V = V.sview(*idx)
    assert V.size == tuple(dims)
    return V


def _flat_line_view(mk, data, dims, coin):
    """A view of size `dims` over a dense parent whose memory order starts with a box dim other than 0 (the line side of
    the FLAT family: unit-stride along a long dim), the remaining dims in one of three orders."""
    N = len(dims)
    qa = 1 + coin[2] % (N - 1)
    rest = [d for d in range(N) if d != qa]
    if coin[3] % 3 == 1:
        rest = rest[::-1]
    elif coin[3] % 3 == 2:
        rest = rest[1:] + rest[:1]
    order = [qa] + rest                       # order[i] = box dim at memory position i
    pshape = tuple(dims[d] for d in order)
    perm = [0] * N
    for i, d in enumerate(order):
        perm[d] = i                           # box dim d = parent dim perm[d]
    return mk(data(pshape)).permutedims(tuple(perm))


def recipe(name, seed, T):
    rng0 = np.random.default_rng(seed)
    f, nin, exact = EXPRS[int(rng0.integers(0, len(EXPRS)))]
    op = initop = None
    reduce_dims = ()
    opts = {}
    nan = False
    pick = lambda xs: xs[int(rng0.integers(0, len(xs)))]  # noqa: E731
    coin = [int(c) for c in rng0.integers(0, 6, size=8)]  # per-input decisions, drawn ONCE (run() is called for both backends)
    if name == "stream":
        dims = pick([(4096, 37), (100, 70, 9), (24, 50, 40), (250000,), (512, 16, 16)])
        mkview = lambda rng, mk, data, k: mk(data(dims)) if k != 1 or coin[k] % 3 else _random_view(rng, mk, data, list(dims))  # noqa: E731
    elif name == "stream_strided":
        dims = pick([(300, 41, 5), (64, 900), (1000, 33)])
        mkview = lambda rng, mk, data, k: _random_view(rng, mk, data, list(dims))  # noqa: E731
    elif name in ("tiled", "tiled_reversed", "tiled_persistent"):
        dims = pick([(512, 384), (1000, 700), (96, 40, 64), (33, 65, 130), (64, 16, 48, 20), (200, 200, 9)])
        rev = name == "tiled_reversed"
        if name == "tiled_persistent":
            opts = {"tiled_persist_min": 1}
        mkview = lambda rng, mk, data, k: _perm_view(rng, mk, data, dims, rev)  # noqa: E731
    elif name == "tiled_short0":
        dims = pick([(2, 40, 36), (3, 50, 70), (4, 16, 20, 12), (2, 128, 128), (3, 33, 65, 9), (4, 4, 4, 4, 4, 4), (2, 64, 2, 64)])
        mkview = lambda rng, mk, data, k: _perm_view(rng, mk, data, dims, keep0=True)  # noqa: E731
    elif name == "tiled_big":
        f, nin, exact = EXPRS[4] if rng0.integers(0, 2) else EXPRS[3]
        dims = pick([(32, 32, 32, 32), (64, 16, 32, 40), (48, 48, 24, 24)])
        mkview = None  # distinct arrays, cyclically permuted: three or more unit axes
    elif name == "flat":
        # round 3: unary transposing maps whose flat side has short leading dims with extents that are not powers of two
        # (destination or input flat, ragged tiles along p and q, outer dims, a sub-box offset, conj views, scalar / jit f)
        UN = [(cx_exact(lambda a: a), 1, True), (lambda a: a * 2.5, 1, True), (lambda a: fn.abs2(a) + 1, 1, True), (lambda a: a * a - a / 3, 1, True),
              (lambda a: fn.conj(a) * 3, 1, True), (cx_exact(lambda a, b: a + b), 2, True), (lambda a, b: 2 * a + 3 * b, 2, True), (lambda a, b, c: a * b - c, 3, True)]
        f, nin, exact = UN[int(rng0.integers(0, len(UN)))]
        dims = pick([(3, 480, 640), (3, 100, 70, 5), (5, 33, 200), (10, 3, 100, 3, 10), (6, 50, 41, 9), (3, 64, 1000), (7, 7, 300), (12, 40, 130)])
        mkview = None
    elif name == "flat2":
        # round 3: both sides' unit-stride dims are short and not powers of two (two-sided FLAT form); the input's leading dim is drawn
        # among the box dims, so one-sided FLAT, TILED and STREAM plans are mixed in
        UN = [(cx_exact(lambda a: a), 1, True), (lambda a: a * 2.5, 1, True), (lambda a: fn.abs2(a) + 1, 1, True), (lambda a: fn.conj(a) * 3, 1, True),
              (cx_exact(lambda a, b: a + b), 2, True), (lambda a, b: a * 2.5 + b, 2, True), (lambda a, b: 3 * a - b * 0.5, 2, True),
              (lambda a, b, c: a + b * c, 3, True)]   # n-ary: ONE input has the other layout, the rest the destination's
        f, nin, exact = UN[int(rng0.integers(0, len(UN)))]
        dims = pick([(5, 60, 50, 7), (17, 9, 33, 31), (3, 100, 90, 3), (7, 30, 40, 9), (6, 16, 16, 16, 5), (12, 10, 14, 9, 11), (10, 50, 60, 10), (31, 65, 33, 17)])
        coin[2] = len(dims) - 2 if coin[4] % 3 else coin[2]   # two times in three the LAST box dim leads the input
        mkview = None
    elif name == "flat_batched":
        # round 4: blocks that are contiguous on both sides, in different element orders, one behind the other (batched FLAT form); one time
        # in three the batch grid is permuted as well (the input side then moves block by block)
        f, nin, exact = pick([(cx_exact(lambda a: a), 1, True), (lambda a: a * 2.5, 1, True), (lambda a: fn.abs2(a) + 1, 1, True), (lambda a: fn.conj(a) * 3, 1, True)])
        dims = pick([(9, 11, 800), (5, 9, 1600), (3, 4, 5, 1200), (7, 6, 333, 9), (17, 23, 200), (3, 10, 13, 200), (9, 11, 40, 30), (6, 10, 50, 40)])
        mkview = None
    elif name == "flat2_long":
        # round 4: long unit-stride dims with odd extents (two-sided FLAT form with evenly cut leads; forced for these small boxes)
        UN = [(cx_exact(lambda a: a), 1, True), (lambda a: a * 2.5, 1, True), (cx_exact(lambda a, b: a + b), 2, True), (lambda a, b: 3 * a - b * 0.5, 2, True)]
        f, nin, exact = UN[int(rng0.integers(0, len(UN)))]
        dims = pick([(257, 129, 9), (301, 75, 11), (513, 65), (129, 257, 5), (131, 67, 3, 5)])
        opts = {"flat2_long": 100}
        mkview = None
    elif name == "tiled_blocks":
        # round 3: distinct arrays with three or four different unit axes, the tiles visited in compact blocks
        # (forced block edge / XCD runs / tile size; VERDICT r2 item 4: `add4 of 4 distinct arrays`, a 3-array map)
        f, nin, exact = EXPRS[4] if rng0.integers(0, 2) else EXPRS[3]
        dims = pick([(40, 40, 40, 40), (64, 16, 32, 40), (24, 20, 36, 28), (48, 48, 24, 24), (96, 33, 50)])
        opts = {"tile_block": int(pick([2, 3, 4, -1])), "tile_block_xcd": int(pick([0, 1])), "tile_log2": int(pick([10, 12, 0]))}
        mkview = None
    elif name in ("orbit", "aliased_classic", "orbit_pipe"):
        dims = pick([(256, 256), (1024, 1024), (96, 96, 24), (32, 32, 32, 32), (16, 16, 16, 16), (64, 8, 64, 8)])
        if name == "orbit_pipe":  # persistent pipelined form: needs more orbits than CUs
            dims = pick([(1024, 1024), (32, 32, 32, 32), (1536, 1536), (24, 24, 24, 24)])
            opts = {"orbit_pipe": 1}
        f, nin, exact = pick([EXPRS[1], EXPRS[2], EXPRS[4], EXPRS[7]])
        if len(dims) == 4 and len(set(dims)) == 1:
            f, nin, exact = EXPRS[4]  # all four cyclic views (two of them alone fuse into a plain 2-d transpose)
        if name == "aliased_classic":
            opts = {"orbit": 0}
        mkview = None
    elif name == "generic":
        dims = pick([(7, 9, 5, 3), (13, 3, 11), (5, 6, 7, 2), (3, 3, 3, 3, 3), (9, 11, 7), (2, 3, 2, 3, 2, 3)])
        mkview = lambda rng, mk, data, k: _random_view(rng, mk, data, list(dims))  # noqa: E731
    elif name == "reduce_all":
        dims = pick([(500, 300, 7), (1 << 20,), (128, 128, 64), (90, 41, 33, 4)])
        reduce_dims = tuple(range(len(dims)))
        mkview = lambda rng, mk, data, k: _perm_view(rng, mk, data, dims) if coin[k] % 2 else mk(data(dims))  # noqa: E731
    elif name == "reduce_short":   # short inner reduced dim (round 3: ROW form with 1-8 lanes per output instead of at least 16)
        dims = pick([(100, 600, 9), (3, 3000, 40), (7, 50000), (12, 50, 60, 10), (25, 2000, 3), (6, 1000, 2, 30)])
        reduce_dims = pick([(0,), (0,), (0, len(dims) - 1)] + ([(0, 2)] if len(dims) > 3 else []))
        mkview = lambda rng, mk, data, k: mk(data(dims))  # noqa: E731
    else:  # reduce_part
        dims = pick([(2048, 600), (600, 2048), (64, 300, 50), (40, 3, 5000), (300, 40, 40, 4)])
        k = int(rng0.integers(1, len(dims)))
        reduce_dims = tuple(sorted(rng0.choice(len(dims), size=k, replace=False).tolist()))
        mkview = lambda rng, mk, data, k: _perm_view(rng, mk, data, dims) if coin[k] % 3 == 0 else mk(data(dims))  # noqa: E731
    cplx = np.issubdtype(np.dtype(T), np.complexfloating)
    if reduce_dims:
        op = ["+", "+", "max", "min"][int(rng0.integers(0, 2 if cplx else 4))]
        initop = [None, "identity", "zero", ("scale", 0.5), ("const", 2.0)][int(rng0.integers(0, 5))]
        exact = False
        nan = op in ("max", "min") and rng0.integers(0, 4) == 0
    vseed = int(rng0.integers(0, 2 ** 31))
    N = len(dims)

    def run(mk, describe=None):
        rng = np.random.default_rng(vseed)
        data = _data(rng, T)
        if name == "flat2":
            kt = coin[5] % nin       # which input has the other layout; the rest are dense like the destination
            ins = [_flat_line_view(mk, data, dims, coin) if k == kt else mk(data(dims)) for k in range(nin)]
            if np.issubdtype(np.dtype(T), np.complexfloating) and coin[1] % 3 == 0:
                ins[coin[6] % nin] = ins[coin[6] % nin].conj()
        elif name == "flat":
            kt = coin[5] % nin
            if coin[0] % 2:          # the transposed input is the line side, destination and the other inputs dense in box order
                ins = [_flat_line_view(mk, data, dims, coin) if k == kt else mk(data(dims)) for k in range(nin)]
            else:                    # destination (and the inputs that share its layout) = the line side, the odd input dense
                ins = [mk(data(dims)) if k == kt else _flat_line_view(mk, data, dims, coin) for k in range(nin)]
            if np.issubdtype(np.dtype(T), np.complexfloating) and coin[1] % 3 == 0:
                ins[coin[6] % nin] = ins[coin[6] % nin].conj()
        elif name == "flat_batched":
            g = 2 if len(dims) == 3 or dims[2] > 16 else 3                       # dims of a block
            lead = [int(i) for i in np.random.default_rng(coin[0] * 8 + coin[1]).permutation(g)]
            if lead == list(range(g)):
                lead = lead[1:] + lead[:1]
            rest = list(range(g, N))
            if len(rest) == 2 and coin[2] % 3 == 0:
                rest = rest[::-1]
            perm = tuple(lead + rest)                                            # view dims = parent dims permuted
            inv = [0] * N
            for i, pp in enumerate(perm):
                inv[pp] = i
            ins = [mk(data(tuple(dims[inv[j]] for j in range(N)))).permutedims(perm)]
        elif name == "flat2_long":
            kt = coin[5] % nin
            perm = (1, 0) + tuple(range(2, N)) if coin[0] % 2 else tuple(range(1, N)) + (0,)
            inv = [0] * N
            for i, pp in enumerate(perm):
                inv[pp] = i
            ins = [mk(data(tuple(dims[inv[j]] for j in range(N)))).permutedims(perm) if k == kt else mk(data(dims)) for k in range(nin)]
        elif name in ("tiled_big", "tiled_blocks"):
            ins = [mk(data(dims)).permutedims(tuple((d + k) % N for d in range(N))) if len(set(dims)) == 1
                   else _perm_view(rng, mk, data, dims) for k in range(nin)]
        elif name in ("orbit", "aliased_classic", "orbit_pipe"):
            base = mk(data(dims))
            group = [tuple(range(N))]
            if N == 2:
                group.append((1, 0))
            elif N == 3:
                group.append((1, 0, 2))
            elif len(set(dims)) == 1:
                group += [tuple((d + k) % 4 for d in range(4)) for k in (1, 2, 3)]
            else:
                group += [(2, 1, 0, 3), (0, 3, 2, 1), (2, 3, 0, 1)]
            ins = [base.permutedims(group[k % len(group)]) for k in range(nin)]
        else:
            ins = [mkview(rng, mk, data, k) for k in range(nin)]
        if nan:
            x = ins[0].parent  # same linear position in the column-major host array and in the flat device tensor
            flat = x.reshape(-1, order="A") if isinstance(x, np.ndarray) else x.reshape(-1)
            flat[int(vseed % max(1, int(np.prod(dims)) // 2))] = np.nan
        odims = [1 if i in reduce_dims else dims[i] for i in range(N)]
        out = mk(data(tuple(odims))) if name != "stream_strided" else _random_view(rng, mk, data, odims)
        if name == "flat" and coin[0] % 2 == 0:
            out = _flat_line_view(mk, data, dims, coin)   # flat side = the input (dense in box order)
        mod = sys.modules["strided_jl_amd.mapreduce"]
        if describe is not None:
            arrs = S.promoteshape(tuple(dims), out, *ins)
            describe.append(S.make_plan(f, op, _initop_fn(initop), tuple(dims), arrs).describe())
        if op is None:
            mod._mapreduce_fuse_(f, None, None, tuple(dims), S.promoteshape(tuple(dims), out, *ins))
        else:
            S._mapreducedim_(f, op, initop, tuple(dims), (out, *ins))
        return out.toarray()

    return run, bitwise(f, exact, T), opts, dict(recipe=name, dims=dims, nin=nin, reduce=reduce_dims, op=op, initop=initop, nan=nan)


def _initop_fn(i):
    if isinstance(i, tuple):
        return (lambda x: x * i[1]) if i[0] == "scale" else (lambda x: i[1])
    return i


RECIPES = ["stream", "stream_strided", "tiled", "tiled_reversed", "tiled_persistent", "tiled_short0", "tiled_big", "orbit", "orbit_pipe", "aliased_classic", "generic",
           "reduce_all", "reduce_part", "tiled_blocks", "flat", "reduce_short", "flat2", "flat_batched", "flat2_long"]

SEED_OFFSET = int(os.environ.get("SMR_FUZZ_SEED_OFFSET", "0"))  # other seeds for longer campaigns on a GPU box


@pytest.mark.parametrize("name", RECIPES)
def test_family_targeted_random_problems_match_the_oracle(name, monkeypatch):
    import torch

    def funnel(f, op, initop, dims, arrays):
        p, keep = S.build_problem(f, op, initop, dims, arrays, stream=0)
        oraclelib.mapreduce(p, 4)
        return arrays[0]

    n = {"reduce_short": 24, "flat_batched": 24, "flat2_long": 20, "flat2": 44, "tiled_big": 40, "tiled_blocks": 30, "flat": 56, "generic": 200, "stream": 40, "tiled": 40, "tiled_reversed": 40, "tiled_persistent": 40, "aliased_classic": 40, "orbit_pipe": 30, "tiled_short0": 30}.get(name, 60)
    fam = collections.Counter()
    for i in range(n):
        for T in TYPES:
            seed = 7919 * RECIPES.index(name) + i + SEED_OFFSET
            run, exact, opts, info = recipe(name, seed, T)
            with monkeypatch.context() as m:
                m.setattr(sys.modules["strided_jl_amd.mapreduce"], "_mapreduce_fuse_", funnel)
                want = run(fview)
            for k, v in opts.items():
                S.set_option(k, v)
            try:
                desc = []
                got = run(dview, desc)
                torch.cuda.synchronize()
            finally:
                for k in opts:
                    S.set_option(k, {"tiled_persist_min": 32, "orbit": 1, "orbit_pipe": -1, "tile_block": -1, "tile_block_xcd": -1, "tile_log2": 0, "flat2_long": 80}[k])
            d = desc[0]
            key = d[d.find("family=") + 7:d.find(" ct=")]
            if key == "flat" and "two-sided" in d:
                key = "flat:two-sided"
            if key == "flat" and "batched" in d:
                key = "flat:batched"
            if key == "reduce_part":
                key += ":" + d[d.find("form=") + 5:].split()[0]
            if key == "tiled":
                key += ":4096" if "threads=1024" in d else ":1024"
                key += "+order" if "order=orbits" in d else ""
            fam[key] += 1
            msg = f"seed {seed} {np.dtype(T).name} {info} | {d}"
            assert got.shape == want.shape, msg
            if exact:   # (test_gpu_fuzz.bitwise: for complex types the copies and sums)
                assert np.array_equal(got, want), msg
            else:
                g, w = got.astype(np.complex128).ravel(), want.astype(np.complex128).ravel()
                assert np.array_equal(np.isnan(g), np.isnan(w)), msg
                g, w = np.nan_to_num(g), np.nan_to_num(w)
                nred = int(np.prod([info["dims"][j] for j in info["reduce"]])) if info["reduce"] else 1
                tol = rtol(T) + nred * float(np.finfo(np.dtype(T)).eps) / 8  # the oracle accumulates serially like the reference
                assert np.linalg.norm(g - w) <= tol * max(np.linalg.norm(g), np.linalg.norm(w), 1e-300), msg
    COUNTS.update(fam)
    print(f"[fuzz families] {name}: " + ", ".join(f"{k} x{v}" for k, v in sorted(fam.items())))


def test_every_family_was_hit_often_enough():
    """runs after the recipes (file order): >= 200 problems per kernel family"""
    print("[fuzz families] total: " + ", ".join(f"{k} x{v}" for k, v in sorted(COUNTS.items())))
    if not COUNTS:
        pytest.skip("recipes did not run in this session")
    by_family = collections.Counter()
    for k, v in COUNTS.items():
        by_family[k.split(":")[0]] += v
    for famname in ("stream", "tiled", "orbit", "generic", "reduce_all", "reduce_part"):
        assert by_family[famname] >= 200, (famname, dict(by_family))
    assert COUNTS["flat:two-sided"] >= 40, dict(COUNTS)    # round 3: two-sided FLAT form
    assert by_family["flat"] >= 60, dict(by_family)   # round 3: the FLAT family (short leading dims that are not powers of two)
