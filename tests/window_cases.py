"""Deterministic table of windowed map problems for the map kernel families (TILED, STREAM, FLAT, ORBIT, GENERIC).

A case is a pure function of (recipe, seed, dtype), built on the host.  Every operand is a window of a larger parent: view dim i is
parent dim perm[i], the parent has (lo, hi) extra elements per dim, each 0..3 (lo odd in the unit-stride dim: the view starts inside a
vector; all pads 0: the view touches the parent's first and last element).  The destination's parent holds random finite bit patterns,
which must come out unchanged; the inputs' parents hold NaN outside the view (integers: the type's minimum), so a read that strays and
reaches the output shows.  Only functors whose result is bit-defined are used; the expected result is NumPy's on the host views, written
into a copy of the destination's parent, and `Case.mismatch` compares the WHOLE flat root allocation byte for byte.

tests/test_window_cases_host.py checks the table without a device (the checker itself, the CPU oracle against NumPy, which kernel
variants the table reaches, counted from describe()); tests/test_gpu_window_fuzz.py runs it under the three store policies and in
recorded sequences.  Host roots are 64-byte aligned like device allocations, so host and device plans choose the same variant.
Nothing here imports torch."""
import collections
import ctypes
import os

import numpy as np

import strided_jl_amd as S

fn = S.fn
SEED_OFFSET = int(os.environ.get("SMR_FUZZ_SEED_OFFSET", "0"))  # other seeds for longer campaigns on a GPU box
FLOATS = [np.float32, np.float64, np.complex64, np.complex128]
INTS = [np.int32, np.int64]
SEEDS = 12
MORE_SEEDS = {"generic": 24}  # (half of the GENERIC draws have a dim 0 long enough for another family)


def is_complex(dt):
    return np.issubdtype(np.dtype(dt), np.complexfloating)


def is_int(dt):
    return np.issubdtype(np.dtype(dt), np.integer)


# ---- functors whose result is bit-defined: (name, f for the library, the same in NumPy, inputs, which types) -----------------------
FUNCTORS = [
    ("ident", lambda a: a, lambda a: a, 1, "all"),
    ("conj", lambda a: fn.conj(a), lambda a: np.conj(a), 1, "float"),
    ("add2", lambda a, b: a + b, lambda a, b: a + b, 2, "all"),
    ("sub2", lambda a, b: a - b, lambda a, b: a - b, 2, "all"),
    ("add4", lambda a, b, c, d: a + b + c + d, lambda a, b, c, d: a + b + c + d, 4, "all"),
    ("mulsub", lambda a, b: a * b - a, lambda a, b: a * b - a, 2, "real"),                         # EXPRS[2] of tests/test_gpu_fuzz.py
    ("expr3", lambda a, b, c: (a + b) * c - b / 3, lambda a, b, c: (a + b) * c - b / 3, 3, "realfloat"),  # EXPRS[3]
]


def functors_for(dt, nin=None):
    out = []
    for name, f, npf, n, kinds in FUNCTORS:
        if kinds == "float" and is_int(dt):
            continue
        if kinds == "real" and is_complex(dt):
            continue
        if kinds == "realfloat" and (is_complex(dt) or is_int(dt)):
            continue
        if nin is None or n in nin:
            out.append((name, f, npf, n))
    return out


# ---- memory ---------------------------------------------------------------------------------------------------------------------------
def aligned_root(n, dt):
    """A flat array of n elements whose first byte is 64-byte aligned and that is the root of its allocation (util.host_flat)."""
    dt = np.dtype(dt)
    nbytes = max(1, n) * dt.itemsize
    buf = (ctypes.c_char * (nbytes + 64))()
    shift = (-ctypes.addressof(buf)) % 64
    raw = (ctypes.c_char * nbytes).from_buffer(buf, shift)
    a = np.frombuffer(raw, dtype=dt)
    assert a.ctypes.data % 64 == 0 and not isinstance(a.base, np.ndarray) and a.flags.writeable
    return a


def values(rng, n, dt):
    dt = np.dtype(dt)
    if is_int(dt):
        info = np.iinfo(dt)
        return rng.integers(info.min // 2, info.max // 2, size=n, dtype=dt, endpoint=True)
    if is_complex(dt):
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dt)
    return rng.standard_normal(n).astype(dt)


def finite_bits(rng, n, dt):
    """n elements of random bit patterns, every one finite."""
    dt = np.dtype(dt)
    a = np.frombuffer(rng.bytes(n * dt.itemsize), dtype=dt).copy()
    if not is_int(dt):
        r = a.view(np.float32 if dt.itemsize // (2 if is_complex(dt) else 1) == 4 else np.float64)
        r[~np.isfinite(r)] = 1.5
    return a


def poison(dt):
    dt = np.dtype(dt)
    if is_int(dt):
        return np.iinfo(dt).min
    return dt.type(complex(np.nan, np.nan)) if is_complex(dt) else dt.type(np.nan)


def element_index(view):
    """Index of every element of `view` in its flat root allocation, shaped like the view."""
    idx = np.full(view.size, view.offset, dtype=np.int64)
    for d, (n, s) in enumerate(zip(view.size, view.strides)):
        shp = [1] * len(view.size)
        shp[d] = n
        idx = idx + (np.arange(n, dtype=np.int64) * s).reshape(shp)
    return idx


def draw_pads(rng, N, mode, perm, pad_dims=None):
    """(lo, hi) per VIEW dim.  mode 0: no pads at all (the view is the whole parent); 1: lo odd in the parent's unit-stride dim; else 0..3
    everywhere.  pad_dims: the PARENT dims that may be padded (None: all)."""
    lo = [int(v) for v in rng.integers(0, 4, size=N)]
    hi = [int(v) for v in rng.integers(0, 4, size=N)]
    if mode % 4 == 0:
        lo, hi = [0] * N, [0] * N
    for i in range(N):
        if mode % 4 == 1 and perm[i] == 0:
            lo[i] = 1 if lo[i] < 2 else 3
        if pad_dims is not None and perm[i] not in pad_dims:
            lo[i] = hi[i] = 0
    return lo, hi


def layout(dims, perm, lo, hi, steps=None):
    """(parent elements, view strides, view offset) of a view of size `dims` whose dim i is dim perm[i] of a column-major parent with lo[i] /
    hi[i] extra elements in front of / behind it; steps[i]: the view's step along dim i in parent elements (negative: reversed)."""
    N = len(dims)
    steps = steps or [1] * N
    pshape = [0] * N
    for i in range(N):
        pshape[perm[i]] = lo[i] + (dims[i] - 1) * abs(steps[i]) + 1 + hi[i]
    pstr, s = [], 1
    for d in pshape:
        pstr.append(s)
        s *= d
    strides, off = [], 0
    for i in range(N):
        st = pstr[perm[i]]
        start = lo[i] if steps[i] > 0 else lo[i] + (dims[i] - 1) * abs(steps[i])
        off += start * st
        strides.append(st * steps[i])
    return s, tuple(strides), off


class Case:
    """arrays[0] is the destination.  `before`: the destination's parent as allocated; `expected`: the same with NumPy's result in the
    view; `inside`: which elements of that parent belong to the view; `inputs_before`: a copy of every input root (keyed by address)."""

    def __init__(self, name, fname, f, npf, dims, arrays, roots):
        self.name, self.fname, self.f, self.npf, self.dims, self.arrays, self.roots = name, fname, f, npf, tuple(dims), tuple(arrays), roots
        self.desc = ""
        dest = arrays[0]
        self.before = dest.parent.copy()
        idx = element_index(dest).ravel()
        assert len(np.unique(idx)) == idx.size
        self.inside = np.zeros(dest.parent.size, dtype=bool)
        self.inside[idx] = True
        with np.errstate(all="ignore"):
            r = np.asarray(npf(*[a.toarray() for a in arrays[1:]]))
        assert r.dtype == dest.dtype and r.shape == self.dims, (name, r.dtype, dest.dtype)
        if dest.op == "conj":
            r = np.conj(r)
        self.expected = self.before.copy()
        self.expected[idx] = r.ravel()
        self.inputs_before = {a.parent.ctypes.data: a.parent.copy() for a in arrays[1:]}

    def __repr__(self):
        return self.name

    def reset(self):
        self.arrays[0].parent[:] = self.before

    def plan(self, arrays=None):
        return S.make_plan(self.f, None, None, self.dims, arrays or self.arrays)

    def mismatch(self, got_parent_bytes, desc=None):
        """None when the destination's whole root allocation holds exactly the expected bytes, else what differs first."""
        g = np.ascontiguousarray(got_parent_bytes).reshape(-1).view(np.uint8)
        w = self.expected.view(np.uint8)
        tail = " | %s | %s" % (self.name, self.desc if desc is None else desc)
        if g.size != w.size:
            return "parent of %d bytes, expected %d" % (g.size, w.size) + tail
        ne = np.flatnonzero(g != w)
        if ne.size == 0:
            return None
        isz = self.expected.dtype.itemsize
        e = int(ne[0]) // isz
        got = g[e * isz:(e + 1) * isz].view(self.expected.dtype)[0]
        nbad = len(np.unique(ne // isz))
        return "element %d of the destination's parent (%s the view) is %r, expected %r, was %r; %d of %d elements differ" % (
            e, "inside" if self.inside[e] else "outside", got, self.expected[e], self.before[e], nbad, self.expected.size) + tail

    def inputs_changed(self, roots_now):
        """roots_now: address of a host input root -> its present contents (host or downloaded).  None, or which input changed."""
        for k, a in enumerate(self.arrays[1:]):
            key = a.parent.ctypes.data
            now = np.ascontiguousarray(roots_now[key]).reshape(-1).view(np.uint8)
            if not np.array_equal(now, self.inputs_before[key].view(np.uint8)):
                return "input %d changed | %s | %s" % (k + 1, self.name, self.desc)
        return None


def dest_view(rng, dims, perm, lo, hi, dt, steps=None, conj=False):
    n, strides, off = layout(dims, perm, lo, hi, steps)
    root = aligned_root(n, dt)
    root[:] = finite_bits(rng, n, dt)
    return S.StridedView(root, tuple(dims), strides, off, "conj" if conj else "identity")


def input_view(rng, dims, perm, lo, hi, dt, steps=None, conj=False, root=None):
    """root: another input's root of the same layout family (aliasing inputs of the orbit recipes); its values stay."""
    n, strides, off = layout(dims, perm, lo, hi, steps)
    if root is None:
        root = aligned_root(n, dt)
        root[:] = poison(dt)
        v = S.StridedView(root, tuple(dims), strides, off)
        idx = element_index(v).ravel()
        root[idx] = values(rng, idx.size, dt)
    assert root.size == n
    return S.StridedView(root, tuple(dims), strides, off, "conj" if conj else "identity")


def ident_perm(N):
    return tuple(range(N))


# ---- the table: recipe -> (shapes, types) ---------------------------------------------------------------------------------------------
# The shapes are the smallest at which each path is taken (tests/test_window_cases_host.py asserts what they reach).
TILED = [((100, 90), (1, 0)), ((257, 129), (1, 0)), ((33, 65, 30), (2, 1, 0)), ((96, 40, 16), (1, 2, 0)), ((64, 64), (1, 0))]
TILED_NARY = [((100, 90, 8), [(1, 0, 2), (2, 1, 0), (0, 1, 2)]), ((32, 32, 32), [(1, 2, 0), (2, 0, 1)])]
CUBES = [(16, 16, 16, 16), (32, 32, 32, 32)]
STREAM = [((131, 40, 3), (0, 2, 1)), ((1001, 9), (0, 1)), ((64, 33), (0, 1)), ((4096,), (0,))]
FLAT_TWO = [((5, 60, 50, 7), (3, 1, 2, 0)), ((17, 9, 33, 31), (3, 2, 1, 0)), ((3, 480, 64), (2, 1, 0))]
ORBIT = [((16, 16, 16, 16), None), ((96, 96, 8), [(0, 1, 2), (1, 0, 2)])]
GENERIC = [(7, 9, 5, 3), (13, 3, 11), (3, 3, 3, 3, 3)]
CYCLIC = [tuple((d + k) % 4 for d in range(4)) for k in range(4)]

RECIPES = {"tiled": FLOATS + INTS, "tiled_nary": FLOATS + INTS, "tiled_orbits": FLOATS + INTS, "tiled_reversed": FLOATS + INTS, "stream": FLOATS + INTS,
           "flat_one": FLOATS, "flat_batched": FLOATS, "flat_two": FLOATS, "orbit": FLOATS, "generic": FLOATS}


def _pick(rng, xs):
    return xs[int(rng.integers(0, len(xs)))]


def build(recipe, seed, dt):
    """The case (recipe, seed, dt)."""
    dt = np.dtype(dt)
    types = FLOATS + INTS
    rng = np.random.default_rng([SEED_OFFSET, sorted(RECIPES).index(recipe), seed, [np.dtype(t) for t in types].index(dt)])
    cx = is_complex(dt)
    flag = lambda: bool(cx and rng.integers(0, 3) == 0)  # noqa: E731  (a conj flag, one complex operand in three)
    name = "%s/%d/%s" % (recipe, seed, dt.name)
    steps_d = None
    pad_in = pad_out = None       # parent dims that may be padded (None: all)
    shared = None                 # orbit recipes: (lo, hi) of the one input buffer
    nshapes = {"tiled": len(TILED), "tiled_reversed": len(TILED), "tiled_nary": len(TILED_NARY), "tiled_orbits": len(CUBES), "orbit": len(ORBIT), "stream": len(STREAM),
               "flat_two": len(FLAT_TWO), "generic": len(GENERIC)}.get(recipe, 1)
    mode = (seed // nshapes) % 4  # how the pads are drawn (draw_pads): every shape of a recipe meets every mode
    if recipe in ("tiled", "tiled_reversed"):
        dims, perm = TILED[seed % len(TILED)]
        fname, f, npf, nin = _pick(rng, functors_for(dt))
        perms = [perm if k % 2 == 0 else ident_perm(len(dims)) for k in range(nin)]   # every other input is laid out like the destination
        if recipe == "tiled_reversed":
            steps_d = [-1 if (seed >> i) & 1 or i == (seed // 2) % len(dims) else 1 for i in range(len(dims))]
    elif recipe == "tiled_nary":
        dims, ps = TILED_NARY[seed % len(TILED_NARY)]
        fs = functors_for(dt, (3,)) if len(ps) == 3 and seed % 4 < 2 else []
        fname, f, npf, nin = _pick(rng, fs or functors_for(dt, (2,) if len(ps) == 2 else (4,)))
        perms = [ps[k % len(ps)] for k in range(nin)]
    elif recipe in ("tiled_orbits", "orbit") and (recipe == "tiled_orbits" or ORBIT[seed % len(ORBIT)][1] is None):
        dims = CUBES[seed % len(CUBES)] if recipe == "tiled_orbits" else ORBIT[seed % len(ORBIT)][0]
        fname, f, npf, nin = functors_for(dt, (4,))[0]
        perms = CYCLIC
        # tiled_orbits: one buffer padded in every dim (its strides are then no permutations of each other's: not the ORBIT family)
        shared = draw_pads(rng, 4, 2, ident_perm(4)) if recipe == "tiled_orbits" else ([0] * 4, [0] * 4)
        if recipe == "orbit":
            pad_out = (3,)
    elif recipe == "orbit":
        dims, perms = ORBIT[seed % len(ORBIT)]
        fname, f, npf, nin = _pick(rng, functors_for(dt, (2,)))
        shared = ([0] * len(dims), [0] * len(dims))
        pad_out = (len(dims) - 1,)
    elif recipe == "stream":
        dims, perm = STREAM[seed % len(STREAM)]
        fname, f, npf, nin = _pick(rng, functors_for(dt))
        perms = [perm] * nin
    elif recipe == "flat_one":
        dims, perm = (3, 480, 64), (2, 1, 0)
        fname, f, npf, nin = _pick(rng, functors_for(dt, (1,)))
        perms = [perm]
        pad_in = pad_out = (2,)   # the last memory dim only: that shifts the offset and keeps the strides
    elif recipe == "flat_batched":
        dims, perm = (9, 11, 800), (1, 0, 2)
        fname, f, npf, nin = _pick(rng, functors_for(dt, (1,)))
        perms = [perm]
        pad_in = pad_out = (2,)
    elif recipe == "flat_two":
        dims, perm = FLAT_TWO[seed % len(FLAT_TWO)]
        fname, f, npf, nin = _pick(rng, functors_for(dt, (1, 2)))
        perms = [perm] + [ident_perm(len(dims))] * (nin - 1)   # ONE input has the other layout, the rest the destination's
    elif recipe == "generic":
        dims = GENERIC[seed % len(GENERIC)]
        fname, f, npf, nin = _pick(rng, functors_for(dt))
        perms = [tuple(int(p) for p in rng.permutation(len(dims))) for _ in range(nin)]
    else:
        raise KeyError(recipe)
    N = len(dims)
    ins = []
    if shared is not None:
        lo, hi = shared
        first = input_view(rng, dims, ident_perm(N), lo, hi, dt)
        for k in range(nin):
            p = perms[k % len(perms)]
            # dim i of this view is dim p[i] of the identity view: the same root, lo / hi permuted along
            v = input_view(rng, tuple(dims[p[i]] for i in range(N)), p, [lo[p[i]] for i in range(N)], [hi[p[i]] for i in range(N)], dt, conj=flag(), root=first.parent)
            assert v.size == tuple(dims)
            ins.append(v)
        roots = [first.parent]
    else:
        for k in range(nin):
            steps = [int(rng.choice([1, 1, 1, 2, -1, 3])) for _ in range(N)] if recipe == "generic" else None
            lo, hi = draw_pads(rng, N, mode if mode == 0 else mode + k, perms[k], pad_in)
            ins.append(input_view(rng, dims, perms[k], lo, hi, dt, steps, conj=flag()))
        roots = [a.parent for a in ins]
    dperm = ident_perm(N)
    if recipe == "generic":
        dperm = tuple(int(p) for p in rng.permutation(N))
        steps_d = [int(rng.choice([1, 1, 1, 2, -1, 3])) for _ in range(N)]
    lo, hi = draw_pads(rng, N, mode, dperm, pad_out)
    if recipe == "orbit" and mode == 0:
        hi[N - 1] = 1 + seed % 3   # (the ORBIT destinations are always padded: behind the view when the draw has no pads)
    out = dest_view(rng, dims, dperm, lo, hi, dt, steps_d, conj=flag())
    return Case(name, fname, f, npf, dims, [out] + ins, [out.parent] + roots)


def cases(recipe):
    for seed in range(MORE_SEEDS.get(recipe, SEEDS)):
        for dt in RECIPES[recipe]:
            yield build(recipe, seed, dt)


# ---- what describe() says about a plan ------------------------------------------------------------------------------------------------
def family(desc):
    return desc[desc.find("family=") + 7:desc.find(" ct=")]


def token(desc, key):
    for tok in desc.split():
        if tok.startswith(key + "="):
            return tok.split("=", 1)[1]
    return None


def variant_key(desc):
    """Family and kernel variant of a plan: equal for the host plan and the device plan of a case."""
    fam = family(desc)
    if fam == "tiled":
        return (fam, token(desc, "tile"), token(desc, "staged"), token(desc, "threads"), token(desc, "vec"), token(desc, "mode"), " wide" in desc, " pipe" in desc,
                token(desc, "order"))
    if fam == "stream":
        return (fam, token(desc, "vec"))
    if fam == "flat":
        return (fam, "batched" if " batched " in desc else ("two-sided" if " two-sided " in desc else "one-sided"), token(desc, "flat_side"), token(desc, "run"))
    if fam == "orbit":
        return (fam, token(desc, "tile"), token(desc, "pair_grid") is not None)
    return (fam,)


def paths(desc):
    """The counted paths a plan takes."""
    fam = family(desc)
    out = ["family=" + fam]
    vec = token(desc, "vec") or "1"
    if fam == "tiled":
        if not vec.startswith("1"):
            out.append("tiled vec>1")
        if "(element-aligned)" in vec:
            out.append("tiled element-aligned")
        out.append("tiled mode=" + token(desc, "mode"))
        if " wide" in desc:
            out.append("tiled wide")
        if token(desc, "threads") == "1024":
            out.append("tiled threads=1024")
        if token(desc, "order") is not None:
            out.append("tiled order=orbits")
        if " pipe" in desc:
            out.append("tiled pipe")
    elif fam == "stream":
        out.append("stream element-aligned+tail" if "element-aligned+tail" in vec else ("stream vec=1" if vec == "1" else "stream aligned vec>1"))
    elif fam == "flat":
        out.append("flat " + variant_key(desc)[1])
    elif fam == "orbit":
        out.append("orbit pair_grid" if token(desc, "pair_grid") is not None else "orbit no pair_grid")
    return out


# every family of the table 24 times, every special path 8 times
MINIMUMS = dict([("family=" + f, 24) for f in ("tiled", "stream", "flat", "orbit", "generic")] +
                [("tiled " + p, 8) for p in ("vec>1", "element-aligned", "mode=9", "mode=1", "mode=7", "mode=2", "mode=0", "wide", "threads=1024")] +
                [("stream " + p, 8) for p in ("vec=1", "aligned vec>1", "element-aligned+tail")] +
                [("flat " + p, 8) for p in ("one-sided", "two-sided", "batched")] +
                [("orbit " + p, 8) for p in ("pair_grid", "no pair_grid")])
# Not reachable by a small windowed shape, so not in the minimums:
#   "tiled pipe" -- the persistent form starts at 32 rounds of 4 workgroups per CU: 32768 tiles, 32 Mi elements.


def check_minimums(counts):
    short = {k: (counts.get(k, 0), v) for k, v in MINIMUMS.items() if counts.get(k, 0) < v}
    assert not short, "paths reached too rarely (reached, minimum): %s | all: %s" % (short, dict(sorted(counts.items())))


def count(counter, desc):
    counter.update(paths(desc))
    return counter


def new_counter():
    return collections.Counter()
