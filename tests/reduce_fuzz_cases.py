"""Deterministic table of windowed reduction problems whose result does not depend on the order of the reduction: one table for the CPU
oracle (test_reduce_fuzz_host.py) and the HIP kernels (test_gpu_reduce_fuzz.py).  Plain NumPy -- no GPU, no torch.

A case is a pure function of (recipe, seed, type); SMR_FUZZ_SEED_OFFSET selects other draws.  Every input is a window of a padded parent as
in window_cases.py (view dim i is parent dim perm[i], pads of 0..3 elements per dim or none at all, steps from {1, 1, 1, 2, 3, -1} as far as
the recipe's target form allows), NaN (Bool and the integers: the value that would change the result) fills the padding and the gaps, the
parents are 64-byte aligned and the view starts at an odd element of the unit-stride dim in a share of the cases.  One to three inputs,
functors ident / abs2 / mul / prog (2x - y + 1, compiled or interpreted) / amc (a * b - c); in a share of the cases one input is broadcast
along a random subset of dims, the same view is passed twice, a complex input is conjugated.  The destination is a window of a parent
filled with 0xA5: kept dims in random memory order, one of them stepped by 2 or 3 or reversed in a share of the cases, conjugated for complex
types in a share, Float64 for about a tenth of the Float32 cases (MIXED).

The data make every reduction order give the same bits (reduce_exact_cases.py has the argument):
  +          nonzero integers (a zero would hide a dropped or doubled element), drawn uniformly up to the largest magnitude that keeps
             3 x (sum over an output of the magnitudes of f and of its intermediate terms) + |initop(old)| below 2^24 (32-bit types) or
             2^53 (64-bit types) -- three applications onto the same destination are tested; `bound(case)` recomputes it from the data.
             The integer class takes full-range values and wraps in Int64, so any order gives the same bits there anyway.
  *          factors from {+-0.5, +-1, +-2}, at most 16 twos and 16 halves per output (integers: {+-1, +-2, +-3}, wrapping).  Not for the
             complex types: the sign of a zero component of a complex product depends on the order of the multiplications.
  min / max  integer data; in a share of the cases, at a random position of a random subset of the outputs, an extreme, a NaN, an Inf, or
             the whole row +-0.0 with the winning zero planted.  Expectations follow Julia (reduce_exact_cases._jl_minmax).
  & / |      Bool, flipped at a random position of a random subset of the outputs.
Expected values are computed from the integers (Python numbers per output), never by a floating-point reduction, for 1, 2 and 3
applications of the call onto the same destination: Case.expected_parent(times=k).

The `negzero` cases are deterministic: every input element is -0.0 and so is the destination.  With initop = nothing the sum is -0.0 --
Base Julia, the reference on one thread and the oracle on one thread agree -- and with initop = zero it is +0.0.  The threaded reference
seeds its per-task slots with zero(T) = +0.0 and so gives +0.0 in both: these cases are checked against the 1-thread oracle only.
"""
from __future__ import annotations

import math
import os

import numpy as np

import reduce_exact_cases as RC
from reduce_exact_cases import Case, Operand, SENTINEL, _index, _init, _jl_minmax, aligned_empty
import strided_jl_amd as S
from strided_jl_amd import _lib as L
from window_cases import layout

SEED_OFFSET = int(os.environ.get("SMR_FUZZ_SEED_OFFSET", "0"))
SEEDS = 14
TYPES = ("f32", "f64", "c32", "c64", "bool", "i64", "i32")     # i32: Int32 inputs into an Int64 destination
FLOATS = ("f32", "f64", "c32", "c64")
IN_DT = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128, "bool": np.bool_, "i64": np.int64, "i32": np.int32}
RECIPES = ("all", "all_box", "row", "row_short", "col", "general", "accumulate", "split", "final")
STEPS = (1, 1, 1, 2, 3, -1)
APPLICATIONS = 3
VMAX = {"f32": 4, "f64": 2, "c32": 2, "c64": 1, "bool": 4, "i64": 2, "i32": 2}   # elements per 16 bytes of the compute class (planning)
ES = {"f32": 4, "f64": 8, "c32": 8, "c64": 16, "bool": 4, "i64": 8, "i32": 8}    # bytes per element of the compute class
NIN = {"ident": 1, "abs2": 1, "mul": 2, "prog": 2, "amc": 3}


def is_cx(t):
    return t in ("c32", "c64")


def is_int(t):
    return t in ("i64", "i32")


def functions(S):
    """name -> f for the library (S = strided_jl_amd)"""
    return {"ident": lambda x: x, "abs2": S.fn.abs2, "mul": lambda x, y: x * y, "prog": lambda x, y: 2 * x - y + 1, "amc": lambda a, b, c: a * b - c}


# ---- exact per-element arithmetic --------------------------------------------------------------------------------------------------
def _wrap(v):
    """Python integer(s) -> two's-complement Int64"""
    return ((v + (1 << 63)) % (1 << 64)) - (1 << 63)


def apply_f(f, xs, t):
    """f over seen values.  xs: int64 / float64 arrays (complex types: (re, im) pairs of int64 arrays).  The integer class follows Julia's
    typing: Int32 * Int32 wraps in Int32, an Int64 literal (prog's 2 and 1) widens first."""
    if is_cx(t):
        (ar, ai) = xs[0]
        if f == "ident":
            return ar, ai
        if f == "abs2":
            return ar * ar + ai * ai, np.zeros_like(ar)
        (br, bi) = xs[1]
        if f == "mul":
            return ar * br - ai * bi, ar * bi + ai * br
        if f == "prog":
            return 2 * ar - br + 1, 2 * ai - bi
        (cr, ci) = xs[2]
        return ar * br - ai * bi - cr, ar * bi + ai * br - ci
    with np.errstate(over="ignore"):
        if t == "i32" and f in ("abs2", "mul", "amc"):
            xs = [x.astype(np.int32) for x in xs]
        if f == "ident":
            r = xs[0]
        elif f == "abs2":
            r = xs[0] * xs[0]
        elif f == "mul":
            r = xs[0] * xs[1]
        elif f == "prog":
            r = 2 * xs[0] - xs[1] + 1
        else:
            r = xs[0] * xs[1] - xs[2]
    return r.astype(np.int64) if is_int(t) else r


def envelope_f(f, xs, t):
    """per element: an upper bound of |f| and of every intermediate term of f (complex types: per component)"""
    if is_cx(t):
        a = [np.abs(r) + 0 for r, _ in xs], [np.abs(i) + 0 for _, i in xs]
        if f == "ident":
            return np.maximum(a[0][0], a[1][0])
        if f == "abs2":
            return a[0][0] ** 2 + a[1][0] ** 2
        m = [np.maximum(r, i) for r, i in zip(*a)]
        if f == "mul":
            return 2 * m[0] * m[1]
        if f == "prog":
            return 2 * m[0] + m[1] + 1
        return 2 * m[0] * m[1] + m[2]
    a = [np.abs(x) for x in xs]
    return {"ident": lambda: a[0], "abs2": lambda: a[0] * a[0], "mul": lambda: a[0] * a[1], "prog": lambda: 2 * a[0] + a[1] + 1,
            "amc": lambda: a[0] * a[1] + a[2]}[f]()


def _emax(f, m, cx):
    return {"ident": m, "abs2": (2 if cx else 1) * m * m, "mul": (2 if cx else 1) * m * m, "prog": 3 * m + 1, "amc": (2 if cx else 1) * m * m + m}[f]


def growth(initop):
    if isinstance(initop, tuple) and initop[0] == "scale":
        b = complex(initop[1])
        return int(abs(b.real) + abs(b.imag))
    return 1


def limit_of(t, mixed):
    return 2 ** 53 if (mixed or t in ("f64", "c64")) else 2 ** 24


def _bound(f_sum, oldmax, initop):
    """magnitude reached in APPLICATIONS applications: B_k = g * B_(k-1) + A, from B_0 = max(|old|, |beta|); at least 3 A + B_0"""
    g = growth(initop)
    b0 = oldmax
    if isinstance(initop, tuple):
        b = complex(initop[1])
        b0 = max(b0, int(abs(b.real) + abs(b.imag)))
    b = b0
    for _ in range(APPLICATIONS):
        b = g * b + f_sum
    return max(b, APPLICATIONS * f_sum + b0)


def largest_magnitude(f, nred, t, mixed, initop, oldmax):
    lim, cap = limit_of(t, mixed), (1 << 22 if mixed else 1 << 40)   # (MIXED: the inputs are Float32, every value must be one)
    lo, hi = 0, cap
    while lo < hi:
        m = (lo + hi + 1) // 2
        # (MIXED: f is evaluated in the inputs' Float32, the accumulation runs in Float64)
        if _bound(nred * _emax(f, m, is_cx(t)), oldmax, initop) < lim and not (mixed and _emax(f, m, False) >= 2 ** 24):
            lo = m
        else:
            hi = m - 1
    return lo


# ---- rows: (outputs, reduced elements) and back ------------------------------------------------------------------------------------
def to_rows(arr, rdims):
    kept = [d for d in range(arr.ndim) if d not in rdims]
    a = np.transpose(arr, kept + list(rdims))
    nout = int(np.prod([arr.shape[d] for d in kept])) if kept else 1
    return a.reshape(nout, -1)


def from_rows(rows, dims, rdims):
    kept = [d for d in range(len(dims)) if d not in rdims]
    order = kept + list(rdims)
    a = rows.reshape([dims[d] for d in order])
    return np.transpose(a, np.argsort(order))


def keepshape(dims, rdims):
    return tuple(1 if d in rdims else n for d, n in enumerate(dims))


def rows_to_keep(v, dims, rdims):
    """per-output values (in to_rows order) -> keepdims array"""
    kept = [d for d in range(len(dims)) if d not in rdims]
    a = np.asarray(v).reshape([dims[d] for d in kept] + [1] * len(rdims))
    return np.transpose(a, np.argsort(kept + list(rdims)))


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
def draw_layout(rng, e, perm, steps, mode, V):
    """(parent elements, strides, offset) of a view of extents e.  mode 0: no pads; 1: an odd start in the unit-stride dim; 2: pads of 0..3;
    3: pads that keep the unit-stride dim in whole aligned vectors of V elements; 4: pads of 0..3, none in the unit-stride dim."""
    N = len(e)
    lo = [int(v) for v in rng.integers(0, 4, size=N)]
    hi = [int(v) for v in rng.integers(0, 4, size=N)]
    if mode == 0:
        lo, hi = [0] * N, [0] * N
    for i in range(N):
        if perm[i] != 0:
            continue
        if mode == 1:
            lo[i] = 1 if lo[i] < 2 else 3
        elif mode == 3:
            lo[i] = V if (V <= 3 and lo[i] >= 2) else 0
            hi[i] = (-(lo[i] + (e[i] - 1) * abs(steps[i]) + 1)) % V
        elif mode == 4:
            lo[i] = hi[i] = 0
    if N == 0:   # one element (the destination of a complete reduction) between 0..3 elements of padding
        l0, h0 = (0, 0) if mode == 0 else (int(rng.integers(0, 4)), int(rng.integers(0, 4)))
        return 1 + l0 + h0, (), l0
    return layout(e, perm, lo, hi, list(steps))


def filler_for(t, op):
    if t == "bool":
        return op == "|"
    if is_int(t):
        info = np.iinfo(IN_DT[t])
        return {"+": info.max // 3 * 2 + 1, "*": 0, "min": info.min, "max": info.max}[op]
    return complex(math.nan, math.nan) if is_cx(t) else math.nan


def make_input(t, dims, lay, bdims, seen, fill, conj):
    """seen: the values the view shows (extents e = dims with 1 along the broadcast dims), already of the input's type"""
    plen, strides, off = lay
    e = tuple(1 if i in bdims else n for i, n in enumerate(dims))
    dt = IN_DT[t]
    parent = aligned_empty(plen, dt)
    parent[...] = fill
    parent[_index(off, e, strides)] = np.conj(seen) if conj else seen
    return Operand(dt, plen, off, tuple(0 if i in bdims else s for i, s in enumerate(strides)), conj=conj, parent=parent)


def make_dest(ddt, dims, rdims, lay, old, conj):
    plen, kstrides, off = lay
    kept = [d for d in range(len(dims)) if d not in rdims]
    strides = [0] * len(dims)
    for j, d in enumerate(kept):
        strides[d] = kstrides[j]
    parent = aligned_empty(plen, ddt)
    parent.view(np.uint8)[...] = SENTINEL
    osh = keepshape(dims, rdims)
    parent[_index(off, osh, strides)] = np.conj(old) if conj else old
    return Operand(ddt, plen, off, tuple(strides), conj=conj, parent=parent)


def to_dt(obj, dt):
    """object array of exact Python numbers -> dtype"""
    dt = np.dtype(dt)
    flat = obj.ravel()
    if dt.kind in "ib":
        out = np.array([int(v) for v in flat], dtype=np.int64).astype(dt) if dt.kind == "i" else np.array([bool(v) for v in flat], dtype=bool)
    elif dt.kind == "c":
        out = np.array([complex(v) for v in flat], dtype=dt)
    else:
        out = np.array([float(v.real) if isinstance(v, complex) else float(v) for v in flat], dtype=dt)
    return out.reshape(obj.shape)


def _objarr(values, shape):
    out = np.empty(int(np.prod(shape)), dtype=object)
    out[:] = list(values)
    return out.reshape(shape)


def combine(op, a, b, t):
    """op(a, b) per output on object arrays of exact Python numbers"""
    out = np.empty(a.shape, dtype=object)
    for i in np.ndindex(*a.shape):
        x, y = a[i], b[i]
        if op == "+":
            v = x + y
        elif op == "*":
            v = x * y
        elif op in ("min", "max"):
            v = (min(x, y) if op == "min" else max(x, y)) if is_int(t) else _jl_minmax([x, y], op)
        elif op == "&":
            v = bool(x) and bool(y)
        else:
            v = bool(x) or bool(y)
        out[i] = _wrap(v) if is_int(t) else v
    return out


def applications(op, initop, old, part, t):
    """{k: destination elements after k applications of dest = op(initop(dest), part)}"""
    cur, out = old, {}
    for k in range(1, APPLICATIONS + 1):
        start = _init(initop, cur)
        if is_int(t):
            start = _objarr([_wrap(int(v)) for v in start.ravel()], start.shape)
        cur = combine(op, start, part, t)
        out[k] = cur
    return out


# ---- recipes: shapes and layouts -----------------------------------------------------------------------------------------------------
class Spec:
    """dims, rdims, per-input layout rule inlay(k) -> (perm, steps, mode, dims that may be broadcast), destination rule, options"""

    def __init__(self, dims, rdims, inlay, destlay, options=None, ops=None):
        self.dims, self.rdims, self.inlay, self.destlay, self.options, self.ops = tuple(int(d) for d in dims), tuple(rdims), inlay, destlay, dict(options or {}), ops


def _steps(rng, n, pool=STEPS):
    return [int(pool[int(rng.integers(0, len(pool)))]) for _ in range(n)]


def _perm(rng, n, first=None):
    """random permutation of range(n): view dim i is parent dim perm[i]; first: the view dim that is parent dim 0"""
    p = [int(v) for v in rng.permutation(n)]
    if first is not None and n:
        j = p.index(0)
        p[j], p[first] = p[first], 0
    return tuple(p)


def _pick(rng, xs):
    return xs[int(rng.integers(0, len(xs)))]


def _factor(rng, target, k):
    """k extents >= 2 (fewer when the target is small) with a product near `target`, odd ones preferred"""
    out, left = [], max(1, int(target))
    for j in range(k):
        if left < 2:
            break
        hi = left if j == k - 1 else max(2, int(round(left ** (1.0 / (k - j)))) * 2)
        d = int(rng.integers(2, max(3, min(hi, left) + 1)))
        if d % 2 == 0 and d + 1 <= left and rng.integers(0, 3):
            d += 1
        out.append(d)
        left //= d
    return out


def _dest_rule(rng, nk, first=None, unit_first=False):
    def rule():
        perm = _perm(rng, nk, first)
        steps = [1] * nk
        if nk and rng.integers(0, 3) == 0:
            steps[int(rng.integers(0, nk))] = int(_pick(rng, (2, 3)))
        if nk and rng.integers(0, 4) == 0:
            j = int(rng.integers(0, nk))
            steps[j] = -steps[j]
        if unit_first and first is not None:
            steps[first] = 1
        return perm, steps, int(rng.integers(0, 3))
    return rule


def spec_all(rng, seed, t):
    sub, V = seed % 7, VMAX[t]
    b = _pick(rng, (1, 2, 16, 17))
    opts = {}
    if sub == 0:
        n, steps, modes = 4096, [1], (0, 3)
    elif sub == 1:
        n, steps, modes = int(rng.integers(1, 4096)), _steps(rng, 1), (0, 1, 2)
    elif sub == 2:
        n, steps, modes = 4096 * b + 4 * int(rng.integers(0 if b == 1 else -3, 4)), [1], (0, 3)   # (vectors start at 4096 elements)
    elif sub == 3:
        n, steps, modes = 4096 * b + int(rng.integers(-5, 6)), _steps(rng, 1, (1, 2, 3, -1)), (1,)
    elif sub == 4:
        n, steps, modes, opts = 4096 * int(rng.integers(2, 18)), [1], (0, 3), {"reduce_single": 0}
    elif sub == 5:
        n, steps, modes, opts = int(rng.integers(4097, 70001)), _steps(rng, 1), (1, 2), {"reduce_single": 0}
    elif seed % 2 == 0:
        n, steps, modes = 64 * 4096 + int(rng.integers(1, 9)), [1], (0, 1, 3)   # 65 workgroups: the second launch at default options
    else:
        n, steps, modes = int(rng.integers(1, 70001)), _steps(rng, 1), (0, 1, 2, 3)

    def inlay(k):
        st = list(steps) if k == 0 or sub in (0, 2, 4) or rng.integers(0, 2) else _steps(rng, 1)
        return (0,), st, int(_pick(rng, modes)), (0,)
    return Spec((n,), (0,), inlay, _dest_rule(rng, 0), opts)


def spec_all_box(rng, seed, t):
    N = 2 + seed % 2
    dims = [int(rng.integers(20, 151)), int(rng.integers(8, 61))] + ([int(rng.integers(2, 7))] if N == 3 else [])
    loose = seed % 4 >= 2   # no unit stride anywhere: REDUCE_ALL walks the box by index decomposition

    def inlay(k):
        perm = _perm(rng, N)
        steps = _steps(rng, N, (2, 3, -2, -3)) if loose else _steps(rng, N)
        if not loose:
            steps[perm.index(0)] = 1
        return perm, steps, int(rng.integers(0, 4)) if not (seed % 4 == 0 and k == 0) else 2, tuple(range(N))
    return Spec(dims, tuple(range(N)), inlay, _dest_rule(rng, 0))


ROW_L0 = (1, 2, 3, 7, 33, 100, 257, 1000, 2047, 4096, 5000, 64, 12, 516)


def spec_row(rng, seed, t):
    L0 = ROW_L0[seed % len(ROW_L0)] if seed < len(ROW_L0) else 2 * int(rng.integers(1, 2500)) + 1
    nr, nk = 1 + int(rng.integers(0, 3)), 1 + int(rng.integers(0, 3))
    red = [L0] + [int(_pick(rng, (2, 3, 5, 6, 7, 9))) for _ in range(nr - 1)]
    if L0 * int(np.prod(red[1:])) > 1 << 15:
        red = red[:2] if L0 <= 2500 else red[:1]
    kept = _factor(rng, min(300, (1 << 17) // int(np.prod(red))), nk) or [2]
    nk = len(kept)
    dims, N = kept + red, len(kept) + len(red)
    mode0 = seed % 4

    def inlay(k):
        perm, steps = _perm(rng, N, first=nk), _steps(rng, N)
        steps[nk] = 1
        return perm, steps, (mode0 + k) % 4 if mode0 else 0, tuple(range(N))
    return Spec(dims, tuple(range(nk, N)), inlay, _dest_rule(rng, nk))


def spec_row_short(rng, seed, t):
    L0 = 1 + (seed % max(1, 64 // ES[t])) if seed % 3 else max(1, 64 // ES[t])
    K0, K1, R1 = int(rng.integers(256, 331)), int(_pick(rng, (1, 1, 2, 3))), int(rng.integers(2, 13))
    kept = [K0] + ([K1] if K1 > 1 else [])
    dims, nk = kept + [L0, R1], len(kept)
    N = len(dims)

    def inlay(k):
        # the inner reduced dim first in memory, kept dim 0 right behind it, the rest in random order
        rest = [d for d in range(N) if d not in (nk, 0)]
        order = [nk, 0] + [rest[int(i)] for i in rng.permutation(len(rest))]
        perm = tuple(order.index(i) for i in range(N))
        steps = _steps(rng, N)
        steps[nk] = steps[0] = 1
        return perm, steps, 4 if seed % 2 else 0, tuple(d for d in range(N) if d not in (nk, 0))

    def destlay():
        perm, steps, mode = _dest_rule(rng, nk, first=0)()
        return perm, steps, mode
    return Spec(dims, (nk, nk + 1), inlay, destlay)


COL_TX = (17, 19, 21, 25, 27, 33, 37, 45, 51, 63, 75, 100, 127, 150, 200, 255)


def spec_col(rng, seed, t):
    V = VMAX[t]
    if seed % 14 < 8:      # a row of n0v vectors, no power of two: the exact lane map, in one to four segments
        tx = COL_TX[(seed + 5 * TYPES.index(t)) % len(COL_TX)]
        n0v = tx * int(_pick(rng, (1, 1, 1, 2, 3, 4)))
        K0 = n0v * V - (int(rng.integers(0, V)) if seed % 4 == 1 else 0)
        ty = max(1, 256 // tx)
    elif seed % 14 < 12:   # power-of-two rows at several widths
        K0, ty = V << int(_pick(rng, (2, 3, 4, 5, 6, 7, 8))), 8
    else:
        K0, ty = int(rng.integers(3, 700)), 8
    nk = 1 + seed % 3
    rest = [int(_pick(rng, (2, 3, 4))) for _ in range(nk - 1)]
    room = max(16, (1 << 17) // (K0 * int(np.prod(rest)) if rest else K0))
    want = min(room, int(_pick(rng, (8, 24, 33, 40, 64))) * ty + int(rng.integers(0, 9)))
    if seed % 2:           # two reduced dims, the inner one short
        L0 = int(_pick(rng, (2, 3, 5, 6, 7, 9)))
        red = [L0, max(2, want // L0)]
    else:
        red = [max(2, want)]
    dims = [K0] + rest + red
    N = len(dims)
    opts = {} if seed % 3 == 0 else ({"reduce_single": 1 << 20} if seed % 3 == 1 else {"reduce_single": 0})

    def inlay(k):
        perm, steps = _perm(rng, N, first=0), _steps(rng, N)
        steps[0] = 1
        return perm, steps, (seed + k) % 4 if seed % 4 else 0, tuple(range(N))
    return Spec(dims, tuple(range(nk, N)), inlay, _dest_rule(rng, nk, first=0, unit_first=True), opts)


def spec_general(rng, seed, t):
    nk, nr = 1 + int(rng.integers(0, 2)), 1 + int(rng.integers(0, 2))
    dims = [int(rng.integers(3, 41)) for _ in range(nk)] + [int(rng.integers(5, 61)) for _ in range(nr)]
    forced = seed % 3 == 0   # a layout that ROW or COL would take, on the general form by option
    if seed % 7 == 6:        # two outputs, 2^16 and more stepped elements each: cut 4 ways (folded in the launch) or 5 ways (second launch)
        nk, nr, forced = 1, 1, False
        dims = [2, int(rng.integers(1 << 16, 80000)) if seed < 7 else int(rng.integers(82000, 90000))]

    N = len(dims)

    def inlay(k):
        if forced:
            first = int(_pick(rng, (0, nk)))
            perm, steps = _perm(rng, N, first=first), _steps(rng, N)
            steps[first] = 1
            return perm, steps, int(rng.integers(0, 4)), tuple(range(N))
        if len(dims) == 2 and dims[1] >= 1 << 16:
            return (0, 1), [1, int(_pick(rng, (2, -2)))], int(rng.integers(0, 3)), (0,)
        return _perm(rng, N), _steps(rng, N, (2, 3, -2, -3, 2)), int(rng.integers(0, 3)), tuple(range(N))
    return Spec(dims, tuple(range(nk, N)), inlay, _dest_rule(rng, nk, first=0 if forced else None), {"reduce_part_kind": 0} if forced else {})


def spec_accumulate(rng, seed, t):
    N = 1 + seed % 3
    dims = _factor(rng, int(_pick(rng, (50, 700, 5000))), N) or [3]
    N = len(dims)

    def inlay(k):
        return _perm(rng, N), _steps(rng, N), int(rng.integers(0, 4)), tuple(range(N))
    return Spec(dims, (), inlay, _dest_rule(rng, N))


def spec_split(rng, seed, t):
    """few outputs, a long reduction: ROW cut along the inner dim, along the outer index, along both; COL; general; chunk counts that
    leave the trailing chunks empty"""
    sub, V = seed % 7, VMAX[t]
    u = V * 256   # elements one sweep of 256 lanes covers along the inner dim
    nout = int(_pick(rng, (2, 2, 3, 4)))
    single = (None, 1 << 20, 0)[(seed // 7 + sub) % 3]
    opts = {} if single is None else {"reduce_single": single}
    form = "row"
    if sub == 0:
        dims, nk = [nout, 8 * u * int(rng.integers(2, 5)) + int(rng.integers(-3, 4)) * V], 1
    elif sub == 1:
        dims, nk = [nout, int(rng.integers(16, 129)) * V, 2 * int(rng.integers(50, 200)) + 1], 1
    elif sub == 2:
        dims, nk = [min(nout, 2), 16 * u + V * int(rng.integers(0, 40)), int(_pick(rng, (2, 3)))], 1
    elif sub == 3:
        form = "col"
        dims, nk = [V * int(_pick(rng, (8, 16, 25, 32))), int(rng.integers(40, 400)), int(_pick(rng, (9, 18, 27, 7, 5)))], 1
    elif sub == 4:
        form = "general"
        dims, nk = [2, int(rng.integers(1 << 15, 49153)), 2], 1
    elif sub == 5:     # ROW: the inner dim cut 10 ways into chunks rounded up to whole sweeps: the last chunk is empty
        if seed < 7 or V == 4:   # whole aligned vectors: chunks of 8 u + 1 elements are rounded up to 9 u
            dims, nk = [2, 80 * u + V], 1
        else:                    # an odd length, scalar loads: the cut is planned for vectors, the chunks are rounded to 256 elements
            dims, nk = [2, (8 * V + 2) * (8 * V) * 256 + 1], 1
    else:              # COL, the outer index cut into more chunks than it fills
        form = "col"
        # (an exact lane map with a prime number of rows, all of them along the outer index: 13 chunks of 12 over 144, 15 of 14 over 196)
        dims, nk = ([V * 23, 10, 144] if seed < 7 else [V * 19, 12, 196]), 1
    N = len(dims)
    if form == "general":
        opts["reduce_part_kind"] = 0

    def inlay(k):
        first = 0 if form == "col" else nk
        perm, steps = _perm(rng, N, first=first), _steps(rng, N)
        steps[first] = 1
        if form == "row" and N > nk + 1:   # the long dim stays the first reduced one in memory order
            order = [nk] + [d for d in range(N) if d != nk]
            perm = tuple(order.index(i) for i in range(N))
        if sub == 6 or (sub == 5 and (seed < 7 or V == 4)):
            return perm, steps, 0, ()
        return perm, steps, (seed // 7 + k) % 4, tuple(range(N))
    return Spec(dims, tuple(range(nk, N)), inlay, _dest_rule(rng, nk, first=0 if nk else None, unit_first=form == "col"), opts)


FINAL_SHAPES = ((25, 20560), (19, 26728))   # lanes 25 x 10 and 19 x 13: 257 chunks of 8 x 10 (8 x 13) rows


def spec_final(rng, seed, t):
    """more than 256 chunks folded by a second launch: k_reduce_part_final then gives every output 64 lanes and walks the partials in
    batches of 8.  A row of 25 (19) elements taken one element per lane -- an odd row has no vector form -- gets an exact lane map of
    25 x 10 (19 x 13) lanes, and one workgroup along the kept dim is cut into as many chunks as hold 8 sweeps of its rows: 257 here.
    514000 and 507832 elements: the smallest shapes that reach the path, below the 2^19 allowed for second launches at default options."""
    dims = list(FINAL_SHAPES[seed % len(FINAL_SHAPES)])

    def inlay(k):
        return (0, 1), [1, 1], 0, (0,)
    return Spec(dims, (1,), inlay, _dest_rule(rng, 1, first=0, unit_first=True))


SPECS = {"final": spec_final, "all": spec_all, "all_box": spec_all_box, "row": spec_row, "row_short": spec_row_short, "col": spec_col, "general": spec_general,
         "accumulate": spec_accumulate, "split": spec_split}


# ---- a case ------------------------------------------------------------------------------------------------------------------------
def draw_op(rng, t):
    if t == "bool":
        return _pick(rng, ("&", "|"))
    if is_cx(t):
        return "+"
    return "+" if rng.random() < 0.6 else _pick(rng, ("*", "min", "max"))


def draw_initop(rng, t, op):
    if t == "bool":
        return None
    kind = _pick(rng, (None, "zero", "conj", "scale", "const"))
    if kind in ("scale", "const"):
        if op == "*":
            b = _pick(rng, (2, -2, -1, 1)) if kind == "scale" else _pick(rng, (1, -1, 2))
        else:
            b = _pick(rng, (2, -1, 3, -2))
        if is_cx(t):
            b = complex(b, _pick(rng, (1, -1, 0)))
            if kind == "scale" and abs(b.real) + abs(b.imag) > 3:
                b = complex(2, -1)
        return (kind, b)
    return kind


def build(recipe, seed, t):
    """The case (recipe, seed, type)."""
    if recipe == "negzero":
        return negzero_case(seed, t)
    rng = np.random.default_rng([SEED_OFFSET, RECIPES.index(recipe), seed, TYPES.index(t)])
    spec = SPECS[recipe](rng, seed, t)
    dims, rdims = spec.dims, spec.rdims
    N = len(dims)
    cx = is_cx(t)
    op = draw_op(rng, t)
    initop = draw_initop(rng, t, op)
    mixed = t == "f32" and seed % 10 == 3   # (2 seeds of 14: a seventh of the Float32 cases accumulate in Float64)
    # functor and inputs
    if t == "bool":
        f = "ident"
    elif op == "*":
        f = _pick(rng, ("ident", "ident", "mul")) if not is_int(t) else _pick(rng, ("ident", "mul", "prog"))
    else:
        f = _pick(rng, ("ident", "ident", "abs2", "mul", "prog", "amc"))
    plant = "none"
    if op in ("min", "max") and rng.integers(0, 3) > 0:
        f = "ident"
        plant = _pick(rng, ("extreme",)) if is_int(t) else _pick(rng, ("extreme", "nan", "inf", "zeros"))
    nin = NIN[f]
    options = dict(spec.options)
    if f in ("prog", "amc"):
        options["jit"] = 1 if rng.integers(0, 3) == 0 else 0
    dup = nin >= 2 and rng.integers(0, 5) == 0
    bk = int(rng.integers(1, nin)) if nin >= 2 and not dup and rng.integers(0, 3) == 0 else -1   # which input is broadcast
    lays = []
    for k in range(nin):
        perm, steps, mode, bok = spec.inlay(k)
        bd = tuple(d for d in bok if rng.integers(0, 2)) if k == bk else ()
        if k == bk and not bd and bok:
            bd = (bok[int(rng.integers(0, len(bok)))],)
        e = tuple(1 if i in bd else n for i, n in enumerate(dims))
        lays.append((draw_layout(rng, e, perm, steps, mode, VMAX[t]), bd, bool(cx and rng.integers(0, 3) == 0)))
    # destination: old values are small integers (products: +-1; Bool: the neutral value, or what the flips cannot change)
    osh = keepshape(dims, rdims)
    nout = int(np.prod(osh))
    nred = int(np.prod(dims)) // nout
    if t == "bool":
        old = _objarr([(op == "&") if rng.integers(0, 4) else (op == "|") for _ in range(nout)], osh)
    elif op == "*":
        old = _objarr([_pick(rng, (1, -1)) * (1 if is_int(t) else 1.0) for _ in range(nout)], osh)
    elif op in ("min", "max"):
        old = _objarr([(int(v) if is_int(t) else float(v)) for v in rng.integers(-1200, 1201, size=nout)], osh)
    elif cx:
        old = _objarr([complex(int(a), int(b)) for a, b in rng.integers(-4, 5, size=(nout, 2))], osh)
    else:
        old = _objarr([int(v) for v in rng.integers(-4, 5, size=nout)], osh)
    # data
    shapes = [tuple(1 if i in bd else n for i, n in enumerate(dims)) for _, bd, _ in lays]
    if dup:
        shapes[1] = shapes[0]
    seen = draw_data(rng, t, op, f, plant, dims, rdims, shapes, initop, mixed, nred)
    if seen is None and isinstance(initop, tuple) and initop[0] == "scale":   # too long a reduction for a growing destination
        initop = ("scale", complex(0, 1) if cx else -1)
        seen = draw_data(rng, t, op, f, plant, dims, rdims, shapes, initop, mixed, nred)
    assert seen is not None, (recipe, seed, t, dims)
    if dup:
        seen[1] = seen[0]
    # expected
    full = [tuple(np.broadcast_to(c, dims) for c in s) if cx else np.broadcast_to(s, dims) for s in seen]
    part = reduce_exact(op, f, full, dims, rdims, t)
    wants = applications(op, initop, old, part, t)
    ddt = np.float64 if mixed else (np.int64 if t == "i32" else IN_DT[t])
    fill = filler_for(t, op)
    ins = []
    for k, ((lay, bd, cj), s) in enumerate(zip(lays, seen)):
        if dup and k == 1:
            ins.append(ins[0])
            continue
        vals = (s[0] + 1j * s[1]).astype(IN_DT[t]) if cx else s.astype(IN_DT[t])
        ins.append(make_input(t, dims, lay, bd, vals, fill, cj))
    kept = [d for d in range(N) if d not in rdims]
    dperm, dsteps, dmode = spec.destlay()
    dconj = bool(cx and rng.integers(0, 3) == 0)
    dest = make_dest(ddt, dims, rdims, draw_layout(rng, [dims[d] for d in kept], dperm, dsteps, dmode, 1), to_dt(old, ddt), dconj)
    name = "%s/%d/%s" % (recipe, seed, t)
    c = Case(name, recipe, dims, rdims, op, initop, f, ins, dest, to_dt(wants[1], ddt), options, (),
             "plant=%s dup=%d bcast=%s mixed=%d" % (plant, dup, lays[bk][1] if bk >= 0 else (), mixed), {k: to_dt(w, ddt) for k, w in wants.items()})
    c.type, c.mixed, c.threads = t, bool(mixed), (1, 4)
    return c


def _nonzero(rng, shape, m):
    return rng.integers(1, m + 1, size=shape, dtype=np.int64) * (rng.integers(0, 2, size=shape, dtype=np.int64) * 2 - 1)


def draw_data(rng, t, op, f, plant, dims, rdims, shapes, initop, mixed, nred):
    """seen values per input (complex types: (re, im)); None when no magnitude keeps the sums exact"""
    cx = is_cx(t)
    if t == "bool":
        v = np.full(dims, op == "&")
        rows = to_rows(v, rdims).copy()
        for o in np.flatnonzero(rng.integers(0, 2, size=rows.shape[0])):
            rows[o, int(rng.integers(0, rows.shape[1]))] = op != "&"
        return [from_rows(rows, dims, rdims).copy()]
    if op == "+":
        if is_int(t):
            info = np.iinfo(IN_DT[t])
            out = [rng.integers(info.min, info.max, size=s, dtype=np.int64, endpoint=True) for s in shapes]
            return [np.where(v == 0, 1, v) for v in out]
        m = largest_magnitude(f, nred, t, mixed, initop, 8 if cx else 4)
        if m < 1:
            return None
        return [(_nonzero(rng, s, m), _nonzero(rng, s, m)) if cx else _nonzero(rng, s, m) for s in shapes]
    if op == "*":
        if is_int(t):
            return [_nonzero(rng, s, 3) for s in shapes]
        out = []
        for s in shapes:
            sign = (rng.integers(0, 2, size=s) * 2 - 1).astype(np.float64)
            if tuple(s) == tuple(dims):   # at most 8 twos and 8 halves per output and input (two inputs: 16)
                rows = to_rows(np.zeros(dims), rdims)
                rank = np.argsort(np.argsort(rng.random(rows.shape), axis=1), axis=1)
                n2, nh = int(rng.integers(0, 9)), int(rng.integers(0, 9))
                ex = np.where(rank < n2, 1, np.where(rank < n2 + nh, -1, 0))
                sign = sign * np.ldexp(1.0, from_rows(ex, dims, rdims))
            out.append(sign)
        return out
    # min / max
    vals = [rng.integers(-1000, 1001, size=s, dtype=np.int64) for s in shapes]
    if is_int(t):
        if plant == "extreme":
            info = np.iinfo(IN_DT[t])
            rows = to_rows(vals[0], rdims).copy()
            for o in np.flatnonzero(rng.integers(0, 2, size=rows.shape[0])):
                rows[o, int(rng.integers(0, rows.shape[1]))] = info.max if op == "max" else info.min
            vals[0] = from_rows(rows, dims, rdims).copy()
        return vals
    vals = [v.astype(np.float64) for v in vals]
    if plant != "none":
        sgn = 1.0 if op == "max" else -1.0
        rows = to_rows(vals[0], rdims).copy()
        for o in np.flatnonzero(rng.integers(0, 2, size=rows.shape[0])):
            j = int(rng.integers(0, rows.shape[1]))
            if plant == "zeros":
                rows[o, :] = -0.0 if op == "max" else 0.0
                rows[o, j] = 0.0 if op == "max" else -0.0
            else:
                rows[o, j] = {"extreme": sgn * (2000.0 + o % 7), "nan": math.nan, "inf": sgn * math.inf}[plant]
        vals[0] = from_rows(rows, dims, rdims).copy()
    return vals


def reduce_exact(op, f, full, dims, rdims, t):
    """op over the reduced dims of f(inputs), exactly -> object array of Python numbers, keepdims shape"""
    osh = keepshape(dims, rdims)
    ax = tuple(rdims)
    if t == "bool":
        r = full[0].all(axis=ax, keepdims=True) if op == "&" else full[0].any(axis=ax, keepdims=True)
        return _objarr([bool(v) for v in r.ravel()], osh)
    if is_cx(t):
        fr, fi = apply_f(f, full, t)
        return _objarr([complex(int(a), int(b)) for a, b in zip(fr.sum(axis=ax, keepdims=True).ravel(), fi.sum(axis=ax, keepdims=True).ravel())], osh)
    v = apply_f(f, full, t)
    if op == "+":
        return _objarr([int(x) for x in v.sum(axis=ax, keepdims=True, dtype=np.int64).ravel()], osh)
    if op == "*":
        if is_int(t):
            with np.errstate(over="ignore"):
                r = np.multiply.reduce(to_rows(v, rdims), axis=1)
            return rows_to_keep(_objarr([int(x) for x in r], (r.size,)), dims, rdims)
        r = np.multiply.reduce(to_rows(v, rdims), axis=1)   # powers of two, exponents within +-16: exact in any order
        return rows_to_keep(_objarr([float(x) for x in r], (r.size,)), dims, rdims)
    rows = to_rows(v, rdims)
    if is_int(t):
        r = rows.max(axis=1) if op == "max" else rows.min(axis=1)
        return rows_to_keep(_objarr([int(x) for x in r], (r.size,)), dims, rdims)
    return rows_to_keep(_objarr([_jl_minmax(rows[o], op) for o in range(rows.shape[0])], (rows.shape[0],)), dims, rdims)


# ---- reading a case back: what the host test asserts from the data ---------------------------------------------------------------------
def seen_values(case):
    """the values every input view shows, from its parent (complex types: (re, im) int64 pairs; else float64 / int64 arrays)"""
    out = []
    for o in case.ins:
        v = o.parent[_index(o.offset, case.dims, o.strides)]
        if o.conj:
            v = np.conj(v)
        if np.dtype(o.dtype).kind == "c":
            out.append((v.real.astype(np.int64), v.imag.astype(np.int64)))
            assert np.array_equal(out[-1][0], v.real) and np.array_equal(out[-1][1], v.imag)
        elif np.dtype(o.dtype).kind == "f":
            out.append(v.astype(np.float64))
        else:
            out.append(v.astype(np.int64))
    return out


def bound(case):
    """(what the data reach, the limit below which the type is exact) for a sum over a float type; None for the other cases"""
    t = case.type
    if case.op != "+" or is_int(t) or t == "bool" or case.cell == "negzero":
        return None
    xs = seen_values(case)
    if not is_cx(t):
        assert all(np.array_equal(x, np.rint(x)) for x in xs)
        xs = [x.astype(np.int64) for x in xs]
        assert all((x != 0).all() for x in xs), "a zero among the addends' factors"
    else:
        assert all((r != 0).all() and (i != 0).all() for r, i in xs)
    env = to_rows(envelope_f(case.f, xs, t), case.rdims).sum(axis=1).max()
    if case.mixed:
        assert envelope_f(case.f, xs, t).max() < 2 ** 24, "f is evaluated in Float32"
    d = case.dest
    old = d.parent[_index(d.offset, case.oshape, case._ostrides())]
    oldmax = int(max(np.abs(old.real).max(), np.abs(old.imag).max()))
    return _bound(int(env), oldmax, case.initop), limit_of(t, case.mixed)


# ---- sums of -0.0 ----------------------------------------------------------------------------------------------------------------------
def _negzero_forms(t):
    """(form, dims, reduced dims, which input dim is first in memory, all dims stepped, options)"""
    V = VMAX[t]
    u = V * 256
    return [
        ("all:epilogue", (1000,), (0,), 0, False, {}),
        ("all:in-launch", (3 * 4096,), (0,), 0, False, {}),
        ("all:second-launch", (3 * 4096,), (0,), 0, False, {"reduce_single": 0}),
        ("row", (6, 516), (1,), 1, False, {}),
        ("row:split", (2, 16 * u), (1,), 1, False, {}),
        ("row:split:empty", (2, 80 * u + V), (1,), 1, False, {}),
        ("col", (32 * V, 100), (1,), 0, False, {}),
        ("col:split", (16 * V, 5, 65 * 16), (1, 2), 0, False, {}),
        ("general", (12, 50), (1,), 0, True, {}),
        ("general:split", (2, 1 << 17), (1,), 1, False, {"reduce_part_kind": 0}),
        ("accumulate", (9, 7), (), 0, True, {}),
    ]


def negzero_count(t):
    return 2 * len(_negzero_forms(t))


def negzero_case(seed, t):
    form, dims, rdims, first, stepped, options = _negzero_forms(t)[seed // 2]
    initop = (None, "zero")[seed % 2]
    rng = np.random.default_rng([7, seed, TYPES.index(t)])
    N, cx = len(dims), is_cx(t)
    dt = IN_DT[t]
    perm = _perm(rng, N, first=first)
    steps = [2] * N if stepped else [1] * N
    lay = draw_layout(rng, dims, perm, steps, 0 if form.startswith(("all", "row:split", "col")) else 2, V=VMAX[t])
    nz = dt(complex(-0.0, -0.0)) if cx else dt(-0.0)
    ins = [make_input(t, dims, lay, (), np.full(dims, nz, dtype=dt), filler_for(t, "+"), False)]
    kept = [d for d in range(N) if d not in rdims]
    osh = keepshape(dims, rdims)
    dest = make_dest(dt, dims, rdims, draw_layout(rng, [dims[d] for d in kept], tuple(range(len(kept))), [1] * len(kept), 2, 1), np.full(osh, nz, dtype=dt), False)
    pz = dt(complex(0.0, 0.0)) if cx else dt(0.0)
    want = np.full(osh, nz if initop is None else pz, dtype=dt)
    c = Case("negzero/%d/%s" % (seed, t), "negzero", tuple(dims), tuple(rdims), "+", initop, "ident", ins, dest, want, dict(options), (),
             "%s: every addend and the destination are -0.0; 1-thread oracle only: the threaded reference seeds its per-task slots with "
             "zero(T) = +0.0 and gives +0.0 where Base Julia, the 1-thread reference and the device give -0.0" % form,
             {k: want for k in range(1, APPLICATIONS + 1)})
    c.type, c.mixed, c.threads = t, False, (1,)
    return c


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def groups():
    """the (recipe, type) pairs: one GPU test each"""
    return [(r, t) for r in RECIPES for t in TYPES] + [("negzero", t) for t in FLOATS]


def seeds(recipe, t):
    if recipe == "final":
        return range(len(FINAL_SHAPES))
    return range(negzero_count(t)) if recipe == "negzero" else range(SEEDS)


def cases(recipe, t):
    for seed in seeds(recipe, t):
        yield build(recipe, seed, t)


def table_size():
    return sum(len(seeds(r, t)) for r, t in groups())


def views(case, S, wrap=None):
    """(destination, inputs...) as StridedViews over copies of the case's parents.  wrap: parent array -> what the view is built over
    (default: a 64-byte aligned host copy, so that host plans see the alignment device allocations have); the same parent passed twice
    (deduplicated inputs) is wrapped once."""
    def aligned_copy(a):
        out = aligned_empty(a.size, a.dtype)
        out[...] = a
        return out
    wrap = wrap or aligned_copy
    done = {}

    def w(o):
        if id(o) not in done:
            done[id(o)] = wrap(o.parent)
        return done[id(o)]
    d = case.dest
    dest = S.StridedView(w(d), case.dims, case._ostrides(), d.offset, "conj" if d.conj else "identity")
    ins = tuple(S.StridedView(w(o), case.dims, o.strides, o.offset, "conj" if o.conj else "identity") for o in case.ins)
    return (dest,) + ins


# ---- what describe() says: the cells of the coverage table -----------------------------------------------------------------------------
def token(desc, key):
    for tok in desc.split():
        if tok.startswith(key + "="):
            return tok.split("=", 1)[1]
    return None


def plan_key(desc):
    """what host and device plans of a case must agree on"""
    return tuple(token(desc, k) for k in ("family", "ct", "f", "dims", "nout", "form", "lanes_per_out", "split", "lanes", "blocks", "vec", "fold", "xcut", "qcut", "tx"))


def _ceil_log2(n):
    k = 0
    while (1 << k) < n:
        k += 1
    return k


CT_VMAX = {"f32": 4, "f64": 2, "c32": 2, "c64": 1, "i64": 2}   # elements per 16 bytes of the compute class describe() names (ct=)


def empty_chunks(desc):
    """does the cut of a split partial reduction leave trailing chunks without elements?  This restates the chunk sizes of build_part_args
    (smr_k_reduce.hip) and g0log of plan_part_row (smr_plan_reduce.cpp) from describe()'s tokens; a note there points back here."""
    split = int(token(desc, "split") or 1)
    if token(desc, "family") != "reduce_part" or split == 1 or token(desc, "fold") == "epilogue":
        return False
    dims = [int(v) for v in token(desc, "dims").split("x")]
    nout, form, tr, vec = int(token(desc, "nout")), token(desc, "form"), int(token(desc, "lanes_per_out")), int(token(desc, "vec"))
    nk, p = 0, 1
    while p < nout:
        p *= dims[nk]
        nk += 1
    nred = int(np.prod(dims)) // nout
    if form == "general":
        chunk = -(-(-(-nred // split)) // tr) * tr
        return (split - 1) * chunk >= nred
    L0 = dims[nk]
    Q = nred // L0
    xs, qs = int(token(desc, "xcut")), int(token(desc, "qcut"))
    qchunk = -(-Q // qs)
    if form == "row":
        g0log = min(_ceil_log2(tr), _ceil_log2(-(-L0 // CT_VMAX[token(desc, "ct").split("(")[0]])))
        unit = vec << g0log
        xchunk = -(-(-(-L0 // xs)) // unit) * unit
    else:
        xchunk = -(-L0 // xs)
    return (xs - 1) * xchunk >= L0 or (qs - 1) * qchunk >= Q


def cells(desc, case):
    """the cells of the coverage table a plan belongs to"""
    fam, fold = token(desc, "family"), token(desc, "fold")
    vec = "vecV" if int(token(desc, "vec") or 1) > 1 else "vec1"
    out = []
    if fam == "reduce_all":
        out.append("all:%s:%s" % (vec, fold))
    elif fam == "reduce_part":
        form = token(desc, "form")
        if form == "general":
            out.append("accumulate" if not case.rdims else "general:%s" % fold)
        else:
            out.append("%s:%s:%s" % (form, vec, fold))
            xs, qs = int(token(desc, "xcut")), int(token(desc, "qcut"))
            if xs > 1 or qs > 1:
                out.append("xsplit>1 qsplit>1" if xs > 1 and qs > 1 else ("xsplit>1" if xs > 1 else "qsplit>1"))
        if form == "row":
            if token(desc, "nout") == "1":
                out.append("row:nout=1")
            if int(token(desc, "lanes_per_out")) <= 8:
                out.append("row:lanes<=8")
        if form == "col":
            if token(desc, "lanes") is not None and token(desc, "tx").split("(")[0] == token(desc, "lanes").split("x")[0]:
                out.append("col:exact")
            if "(narrowed)" in (token(desc, "tx") or ""):
                out.append("col:narrowed")
        if empty_chunks(desc):
            out.append("empty trailing chunks")
        if fold == "second-launch" and int(token(desc, "split")) > 256:
            out.append("final:batches-of-8")
    if "(mixed)" in desc and case.mixed:
        out.append("mixed")
    return out


CELLS = (["all:%s:%s" % (v, f) for v in ("vec1", "vecV") for f in ("epilogue", "in-launch", "second-launch")] +
         ["%s:%s:%s" % (k, v, f) for k in ("row", "col") for v in ("vec1", "vecV") for f in ("epilogue", "in-launch", "second-launch")] +
         ["row:nout=1", "row:lanes<=8", "col:exact"] + ["general:%s" % f for f in ("epilogue", "in-launch", "second-launch")] +
         ["accumulate", "mixed", "xsplit>1", "qsplit>1", "xsplit>1 qsplit>1", "empty trailing chunks", "final:batches-of-8"])
# Not in the list, because no shape within the table's limit of 2^18 input elements reaches it:
#   "col:narrowed" -- plan_part_col narrows the row segment (fewer lanes along kept dim 0) only when that puts at least 256 workgroups
#   along the kept dims while every lane row keeps 8 rows of the reduced space: 256 * 2^t * V * 8 * 2^(8-t) = 2^19 * V elements.  The
#   smallest shape that launches a narrowed segment is ComplexF64, kept dims (16, 128) with a gap between them (so that they do not
#   fuse), 256 reduced elements: 2^19 elements, `tx=8(narrowed)`.  (Kept dims (17, 128) with 128 reduced elements, 278528 elements, make
#   the planner narrow too -- 17 elements over segments of 16 lanes double the workgroups -- but the launch then takes the exact lane
#   map 17 x 15 instead, and describe() says (narrowed) only of a segment that is launched.)
# "mixed" exists for one pair of types only (Float32 into Float64).
MIN_CASES, MIN_TYPES, MIN_EXACT_TX = 8, 2, 12
ONE_TYPE = ("mixed",)


def check_cells(reached, exact_tx):
    """reached: cell -> list of types of the cases that reached it"""
    short = {c: (len(reached.get(c, ())), len(set(reached.get(c, ())))) for c in CELLS
             if len(reached.get(c, ())) < MIN_CASES or len(set(reached.get(c, ()))) < (1 if c in ONE_TYPE else MIN_TYPES)}
    assert not short, "cells reached too rarely (cases, types): %s" % short
    assert len(exact_tx) >= MIN_EXACT_TX, "exact lane maps with %d distinct TX: %s" % (len(exact_tx), sorted(exact_tx))


# ---- planning a case on the host, under its options -------------------------------------------------------------------------------------
F = functions(S)
GROUPS = groups()


def with_options(case, fn):
    """fn() with the library options of the case set, and put back after"""
    lib = L.load()
    saved = {k: lib.smr_get_option(k.encode()) for k in case.options}
    try:
        for k, v in case.options.items():
            L.check(lib.smr_set_option(k.encode(), v))
        return fn()
    finally:
        for k, v in saved.items():
            L.check(lib.smr_set_option(k.encode(), v))


def host_describe(case):
    """describe() of the plan made over 64-byte aligned host copies of the case's parents"""
    def go():
        plan = S.make_plan(F[case.f], case.op, case.initop, case.dims, views(case, S))
        d = plan.describe()
        plan.close()
        return d
    return with_options(case, go)
