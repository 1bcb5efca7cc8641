"""Deterministic recipes of grouped launches (smr_group_* / csrc/smr_k_group.hip) and the helpers that run one group on the device.
A recipe returns Case objects: the (f, host arrays) calls of ONE group in the convention of run_group below, and per member what the
recipe intends to hit (body, canonical rank, workgroups, the canonical position of the tiled dim q).  tests/test_group_cases_host.py
checks those intentions against smr_group_layout / smr_group_describe without a device; tests/test_gpu_group_fuzz.py runs the groups.

Every destination is a view into a fresh parent of its own that is larger than the view on every side and filled with a pattern, so
no group is ever refused for overlap and a write outside a member shows in the parent.  Nothing here imports torch at import time."""
import contextlib
import os

import numpy as np

import strided_jl_amd as S
from strided_jl_amd import _lib as L
from test_gpu_fuzz import _random_view
from test_gpu_fuzz_families import _perm_view
from util import host_flat, run_oracle, rtol, to_device

fn = S.fn
CHUNK = 256 * 4   # canonical indices per workgroup of the linear body (csrc/smr_group.h: GROUP_CHUNK)
TILE = 32         # tile edge of the transposing body (GROUP_TILE)
TMIN = 16         # the transposing body needs both tiled dims at least this long (GROUP_TMIN)
SEED_OFFSET = int(os.environ.get("SMR_FUZZ_SEED_OFFSET", "0"))  # other seeds for longer campaigns on a GPU box
FLOATS = [np.float32, np.float64, np.complex64, np.complex128]
EDGES = (16, 17, 31, 32, 33, 63, 64, 65)  # plane extents around the tile edge and its multiples


def ident(x):
    return x


def sync():
    import torch
    torch.cuda.synchronize()


def cur_stream():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def rand(rng, shape, dt):
    dt = np.dtype(dt)
    if np.issubdtype(dt, np.integer):
        a = rng.integers(-100000, 100000, size=shape).astype(dt)
    elif np.issubdtype(dt, np.complexfloating):
        a = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt)
    else:
        a = rng.standard_normal(shape).astype(dt)
    return S.StridedView(np.asfortranarray(a).copy(order="F"))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def element_index(view, shift=0):
    """Index of every element of `view` in the flat root allocation (shift: host_flat's second result), shaped like the view."""
    idx = np.full(view.size, view.offset + shift, dtype=np.int64)
    for d, (n, s) in enumerate(zip(view.size, view.strides)):
        shp = [1] * len(view.size)
        shp[d] = n
        idx = idx + (np.arange(n, dtype=np.int64) * s).reshape(shp)
    return idx


def run_group(calls, independent=False, ref=None, whole=None):
    """calls: (f, host arrays).  Returns (group, per call: oracle result, group result, result of the call issued alone).
    `ref`: a NumPy function of the input arrays that stands in for the oracle, whose f-program evaluator has no math opcodes.
    `whole`: a list that receives per call (the destination's whole parent before the run, the device's whole parent after the group ran,
    the host's whole parent -- which the oracle writes --, the indices of the destination's elements in it)."""
    cache, devs = {}, []
    for f, arrays in calls:
        devs.append(tuple(to_device(a, cache) for a in arrays))
    before_parents = [host_flat(arrays[0])[0].copy() for f, arrays in calls] if whole is not None else []
    alone = []
    for (f, arrays), dev in zip(calls, devs):  # the same call alone, on private copies taken before anything ran
        c2 = {}
        d2 = tuple(to_device(a, c2) for a in arrays)
        S._mapreduce_fuse_(f, None, None, arrays[0].size, d2)
        sync()
        alone.append(d2[0].toarray())
    built = [S.build_problem(f, None, None, arrays[0].size, dev, stream=cur_stream()) for (f, arrays), dev in zip(calls, devs)]
    g = L.Group([b[0] for b in built], independent, keepalive=built)
    sync()
    before = S.get_option("launches")
    g.execute(cur_stream())
    assert S.get_option("launches") == before + 1
    sync()
    got = [dev[0].toarray() for dev in devs]
    if ref is None:
        want = [run_oracle(f, None, None, arrays[0].size, arrays) for f, arrays in calls]
    else:
        want = [ref(*[a.toarray() for a in arrays[1:]]) for f, arrays in calls]
    if whole is not None:
        for (f, arrays), b in zip(calls, before_parents):
            flat, shift = host_flat(arrays[0])
            whole.append((b, cache[flat.ctypes.data].cpu().numpy(), flat, element_index(arrays[0], shift)))
    return g, want, got, alone


# ---- building blocks ------------------------------------------------------------------------------------------------------------------
def hview(a):
    return S.StridedView(np.asfortranarray(a).copy(order="F"))


def values(rng, shape, dt):
    dt = np.dtype(dt)
    if np.issubdtype(dt, np.integer):
        info = np.iinfo(dt)
        return np.asfortranarray(rng.integers(info.min // 2, info.max // 2, size=shape, dtype=dt, endpoint=True))
    if np.issubdtype(dt, np.complexfloating):
        return np.asfortranarray((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt))
    return np.asfortranarray(rng.standard_normal(shape).astype(dt))


def dest(rng, dims, dt, step0=1):
    """A destination of size `dims`: a view (step `step0` along dim 0) into a fresh column-major parent that has one or two more
    elements than the view needs at both ends of every dim.  The parent holds a pattern no result of the recipes equals."""
    lo = [int(rng.integers(1, 3)) for _ in dims]
    hi = [int(rng.integers(1, 3)) for _ in dims]
    steps = [step0] + [1] * (len(dims) - 1)
    pshape = tuple(lo[i] + (dims[i] - 1) * steps[i] + 1 + hi[i] for i in range(len(dims)))
    n = int(np.prod(pshape))
    parent = (7 + np.arange(n) % 113).astype(dt).reshape(pshape, order="F")
    return hview(parent).sview(*[slice(lo[i], lo[i] + (dims[i] - 1) * steps[i] + 1, steps[i]) for i in range(len(dims))])


def rank_of(dims):
    return max(1, sum(1 for d in dims if d > 1))  # the padded destination never fuses two dims; size-1 dims are dropped


def linear_member(rng, dims, dt, nin, bcast=None, ddt=None):
    """Inputs: stepped (1, 2, 3, -1), offset, permuted views (dense permuted, some dims reversed, for boxes of seven and more dims);
    bcast = (input, dim): that input is broadcast along that dim.  Returns (arrays, info)."""
    dims = tuple(dims)
    ins = []
    for k in range(nin):
        d_k = list(dims)
        if bcast is not None and bcast[0] == k:
            d_k[bcast[1]] = 1
        if len(dims) >= 7:
            ins.append(_perm_view(rng, hview, lambda shape: values(rng, shape, dt), d_k, reverse=True))
        else:
            ins.append(_random_view(rng, hview, lambda shape: values(rng, shape, dt), d_k))
    arrays = S.promoteshape(dims, dest(rng, dims, ddt or dt), *ins)
    total = int(np.prod(dims))
    return arrays, dict(form=0, rank=rank_of(dims), wgs=(total + CHUNK - 1) // CHUNK, total=total, dims=dims, bcast=bcast is not None)


def plane_member(rng, dt, p, q, before=(), after=(), nin=1, kt=0, rev="", step2=False, other="dst", conj=False, ddt=None):
    """A member whose input `kt` (0-based among `nin`) is unit-stride along the dim of extent q, behind dim 0 (extent p) and the outer
    dims `before`; `after` follow it.  rev: "q" reverses that input along its unit dim, "p" along dim 0.  step2: the destination has
    step 2 along dim 0.  The other inputs are laid out like the destination ("dst"), broadcast along dim 0 ("b0") or along q ("bq").
    The transposing body takes it when p and q reach TMIN, else the linear body."""
    dims = (p,) + tuple(before) + (q,) + tuple(after)
    N, qpos = len(dims), 1 + len(before)
    order = [qpos, 0] + [d for d in range(N) if d not in (0, qpos)]   # order[i] = box dim at memory position i of the staged input
    perm = [0] * N
    for i, d in enumerate(order):
        perm[d] = i
    st = hview(values(rng, tuple(dims[d] for d in order), dt)).permutedims(tuple(perm))
    if rev:
        st = st.sview(*[slice(None, None, -1) if d == (qpos if rev == "q" else 0) else slice(None) for d in range(N)])
    if conj:
        st = st.conj()
    ins = []
    for k in range(nin):
        if k == kt:
            ins.append(st)
            continue
        d_k = list(dims)
        if other == "b0":
            d_k[0] = 1
        elif other == "bq":
            d_k[qpos] = 1
        ins.append(hview(values(rng, tuple(d_k), dt)))
    arrays = S.promoteshape(dims, dest(rng, dims, ddt or dt, 2 if step2 else 1), *ins)
    outer = int(np.prod([d for i, d in enumerate(dims) if i not in (0, qpos)]))
    form = 1 if min(p, q) >= TMIN else 0
    total = int(np.prod(dims))
    wgs = ((p + TILE - 1) // TILE) * ((q + TILE - 1) // TILE) * outer if form else (total + CHUNK - 1) // CHUNK
    info = dict(form=form, rank=rank_of(dims), wgs=wgs, total=total, dims=dims, p=p, q=q, cq=1 + sum(1 for d in before if d > 1), outer=outer,
                both_sides=any(d > 1 for d in before) and any(d > 1 for d in after), nin=nin, kt=kt, rev=rev, step2=step2,
                other=other if nin > 1 else "", conj=conj)
    return arrays, info


class Case:
    """One group: `calls` in run_group's convention, `info` per member, and how its results are judged.
    exact: the device's whole destination parents equal the oracle's bit for bit (else: nothing outside the member changed, and the
    member agrees norm-wise within util.rtol).  alone_exact: every member equals the same call issued alone bit for bit.
    ref: NumPy stand-in for the oracle (math opcodes).  np_ref: NumPy truth compared in addition to the oracle (integers).
    fname / jit: what describe() reports as f= and jit= ; opts: library options the group is planned and run under."""

    def __init__(self, name, f, fname, jit=0, exact=True, alone_exact=True, ref=None, np_ref=None, opts=None):
        self.name, self.f, self.fname, self.jit, self.exact, self.alone_exact, self.ref, self.np_ref = name, f, fname, jit, exact, alone_exact, ref, np_ref
        self.opts = dict(opts or {})
        self.calls, self.info = [], []

    def add(self, member):
        arrays, info = member
        self.calls.append((self.f, arrays))
        self.info.append(info)
        return self

    def __repr__(self):
        return self.name


@contextlib.contextmanager
def options(case):
    """The library options of `case` for the duration of the block."""
    old = {k: S.get_option(k) for k in case.opts}
    try:
        for k, v in case.opts.items():
            S.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            S.set_option(k, v)


def build_group(case):
    """The case's group planned on its host views (no device needed)."""
    with options(case):
        built = [S.build_problem(f, None, None, arrays[0].size, arrays, stream=0) for f, arrays in case.calls]
        return L.Group([b[0] for b in built], keepalive=built)


def is_complex(dt):
    return np.issubdtype(np.dtype(dt), np.complexfloating)


def _rng(recipe_id, dt=None, extra=0):
    return np.random.default_rng([SEED_OFFSET, recipe_id, FLOATS.index(dt) if dt in FLOATS else 9, extra])


# ---- recipe `linear` ------------------------------------------------------------------------------------------------------------------
LINEAR_BOXES = [(1,), (255,), (256,), (257,), (1023,), (1024,), (1025,), (2049,), (255, 5), (256, 5), (257, 5), (300, 7), (3,) * 7, (2, 3, 2, 3, 2, 3, 2, 3),
                (3, 5, 7, 11), (5, 1, 7, 1, 9)]


def linear(dt):
    """The mixed-radix step of the linear body: totals around one and two chunks, dims[0] around 256, radices in which 256 has several
    non-zero digits (ranks 4, 7 and 8), inputs that are stepped, reversed, offset, permuted or broadcast views."""
    rng = _rng(1, dt)
    out, n = [], 0
    for fname, f, nin in (("ident", ident, 1), ("add2", lambda a, b: a + b, 2)):
        c = Case("linear/%s/%s" % (fname, np.dtype(dt).name), f, fname)
        for dims in LINEAR_BOXES:
            bcast = None
            for k in range(nin):
                n += 1
                if n % 6 == 0:  # one input in six
                    bcast = (k, int(rng.integers(0, len(dims))))
            c.add(linear_member(rng, dims, dt, nin, bcast))
        out.append(c)
    return out


# ---- recipe `transposing` -------------------------------------------------------------------------------------------------------------
OUTER = [((), ()), ((2,), ()), ((), (3,)), ((3,), (2,)), ((2, 3), ()), ((), (2, 2)), ((1,), (3,)), ((2,), (1,))]  # (before, after) the unit dim


def transposing(dt):
    """All 64 pairings of the plane extents, dealt to one group per (number of inputs, position of the staged input, conj): ranks 2-4,
    outer dims on either side of q, reversed staged inputs, stepped destinations, broadcast companions."""
    rng = _rng(2, dt)
    pairs = [(p, q) for p in EDGES for q in EDGES]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    kinds = [(nin, kt, cj) for nin in (1, 2, 3) for kt in range(nin) for cj in ((False, True) if is_complex(dt) else (False,))]
    fs = {1: ("scale", lambda a: a * 2.5), 2: ("add2", lambda a, b: a + b), 3: ("add3", lambda a, b, c: a + b + c)}
    if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)):
        k32 = np.float32(2.5)  # (a Float64 constant would widen the Float32 product)
        fs[1] = ("scale", lambda a: a * k32)
    out = []
    for g, (nin, kt, cj) in enumerate(kinds):
        fname, f = fs[nin]
        c = Case("transposing/%s/%s/in%d.%d%s" % (fname, np.dtype(dt).name, nin, kt, ".conj" if cj else ""), f, fname,
                 exact=not is_complex(dt) or nin > 1)  # a complex product with a constant: norm-wise against the oracle
        for n in range(g * len(pairs) // len(kinds), (g + 1) * len(pairs) // len(kinds)):
            p, q = pairs[n]
            before, after = OUTER[n % len(OUTER)]
            c.add(plane_member(rng, dt, p, q, before, after, nin, kt, rev=("", "q", "p")[n % 3], step2=(n // 2) % 3 == 0,
                               other=("dst", "b0", "bq")[(n // 3) % 3], conj=cj))
        out.append(c)
    return out


# ---- recipe `tmin` --------------------------------------------------------------------------------------------------------------------
TMIN_PLANES = [(15, 16), (16, 15), (16, 16), (15, 40), (40, 15)]


def tmin(dt=None):
    """Transposed planes on both sides of GROUP_TMIN: only (16, 16) takes the transposing body."""
    rng = _rng(3)
    c = Case("tmin/float64", ident, "ident")
    for p, q in TMIN_PLANES:
        c.add(plane_member(rng, np.float64, p, q))
    return [c]


# ---- recipe `functors` ----------------------------------------------------------------------------------------------------------------
def functor_table(dt):
    """(name, f, inputs, NumPy stand-in or None) in the lambda forms csrc/smr_canon.cpp recognises, constants in the real type of dt."""
    R = np.float32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64
    k, h = R(2.5), R(0.5)
    table = [("ident", lambda a: a, 1, None), ("add2", lambda a, b: a + b, 2, None), ("add3", lambda a, b, c: a + b + c, 3, None),
             ("add4", lambda a, b, c, d: a + b + c + d, 4, None), ("scale", lambda a: a * k, 1, None), ("sym", lambda a, b: (a + b) / 2, 2, None),
             ("axpy", lambda a, b: k * a + b, 2, None), ("axpby", lambda a, b: k * a + h * b, 2, None), ("abs2", lambda a: fn.abs2(a), 1, None),
             ("mul2", lambda a, b: a * b, 2, None)]
    if not is_complex(dt):
        table.append(("expr5", lambda a: a * fn.exp(h * a) + fn.sin(a * a), 1, lambda a: (a * np.exp(h * a) + np.sin(a * a)).astype(dt)))
    return table


def six_members(rng, c, dt, nin, ddt=None):
    """3 linear and 3 transposing members from the shapes of the two recipes above; the staged input takes every position in turn."""
    c.add(linear_member(rng, (257, 5), dt, nin, ddt=ddt))
    c.add(linear_member(rng, (3,) * 7, dt, nin, (nin - 1, 2), ddt=ddt))
    c.add(linear_member(rng, (1025,), dt, nin, ddt=ddt))
    c.add(plane_member(rng, dt, 17, 33, nin=nin, kt=0, other="b0", ddt=ddt))
    c.add(plane_member(rng, dt, 33, 65, (2,), (), nin, kt=1 % nin, rev="q", step2=True, other="dst", ddt=ddt))
    c.add(plane_member(rng, dt, 64, 31, (), (3,), nin, kt=nin - 1, rev="p", other="bq", ddt=ddt))
    return c


def MATH_F(p, q):
    return p ** 2 + fn.tanh(q)


def functors(dt):
    """One group per natively compiled functor, then f = prog (a * b - a) and a math-opcode f, runtime-compiled and interpreted."""
    rng = _rng(4, dt)
    cx = is_complex(dt)
    out = []
    for fname, f, nin, ref in functor_table(dt):
        bitwise = not cx or fname in ("ident", "add2", "add3", "add4")
        c = Case("functors/%s/%s" % (fname, np.dtype(dt).name), f, fname, exact=bitwise and ref is None, ref=ref,
                 alone_exact=not cx or bitwise or fname == "scale")
        out.append(six_members(rng, c, dt, nin))
    if np.dtype(dt) == np.dtype(np.float64):
        for jit in (1, 0):
            tag = "jit" if jit else "interpreted"
            out.append(six_members(rng, Case("functors/prog/float64/" + tag, lambda a, b: a * b - a, "prog", jit=jit, opts={"jit": jit}), dt, 2))
            if jit:  # (the interpreter has no math opcodes: with "jit" = 0 the library refuses this f, in a group as in a single call)
                out.append(six_members(rng, Case("functors/math/float64/" + tag, MATH_F, "prog", jit=jit, exact=False,
                                                 ref=lambda p, q: p * p + np.tanh(q), opts={"jit": jit}), dt, 2))
    return out


# ---- recipe `bitcopy` -----------------------------------------------------------------------------------------------------------------
def bitcopy(dt=None):
    """Copies and permutes of 1-, 2-, 4- and 8-byte integers (bit copies) and of ComplexF64 (16 bytes, f = ident)."""
    rng = _rng(5)
    out = []
    for t in (np.int8, np.int16, np.int32, np.int64, np.complex128):
        c = Case("bitcopy/%s" % np.dtype(t).name, ident, "ident" if t is np.complex128 else "bitcopy")
        c.add(linear_member(rng, (257, 5), t, 1))
        c.add(plane_member(rng, t, 33, 65, (2,), (3,), rev="q"))
        out.append(c)
    return out


# ---- recipe `integer` -----------------------------------------------------------------------------------------------------------------
def integer(dt):
    """Integer arithmetic (the 64-bit wrapping class, truncated on store) in groups.  Int32 and UInt8 operands are converted on load, which
    takes the f-program path: runtime-compiled once (Int32, a * b - a), interpreted otherwise."""
    rng = _rng(6, extra=np.dtype(dt).itemsize)
    wide = np.dtype(dt) == np.dtype(np.int64)
    out = []
    for tag, f, nin, native in (("scale3", lambda a: a * 3, 1, "scale"), ("add2", lambda a, b: a + b, 2, "add2"), ("prog", lambda a, b: a * b - a, 2, "prog")):
        jit = 1 if tag == "prog" and np.dtype(dt) != np.dtype(np.uint8) else 0
        c = Case("integer/%s/%s" % (tag, np.dtype(dt).name), f, native if wide else "prog", jit=jit, np_ref=f, opts={} if wide else {"jit": jit})
        c.add(linear_member(rng, (257, 5), dt, nin))
        c.add(linear_member(rng, (3, 5, 7, 11), dt, nin, (0, 1)))
        c.add(plane_member(rng, dt, 33, 17, (2,), (), nin, kt=nin - 1, rev="q", step2=True, other="b0"))
        c.add(plane_member(rng, dt, 31, 64, (), (3,), nin, kt=0, rev="p", other="bq"))
        out.append(c)
    return out


# ---- recipe `mixed` -------------------------------------------------------------------------------------------------------------------
def mixed(dt=None):
    """Destination / input type pairs of tests/test_mixed_precision.py; the transposing members stage another type than the destination's."""
    rng = _rng(7)
    f32, f64 = np.float32, np.float64
    out = []
    c = Case("mixed/f64=f32*f32-c", lambda a, b: a * b - 0.5, "prog", jit=1)        # Float32 product, widened, then a Float64 constant
    out.append(six_members(rng, c, f32, 2, ddt=f64))
    c = Case("mixed/f32=f32*0.1", lambda a: a * 0.1, "prog", jit=1)                 # a Float64 scalar: one rounding on store
    out.append(six_members(rng, c, f32, 1, ddt=f32))
    c = Case("mixed/f64=(f32+f32)*f64", lambda x, y, z: (x + y) * z, "prog", jit=1)  # the Float32 sum is rounded, the product is not
    for p, q, kt, rev in ((257, 5, 0, ""), (17, 33, 0, "p"), (33, 65, 1, "q"), (64, 31, 0, "")):
        # inputs 0 and 1 are Float32, input 2 Float64: built as a two-input Float32 member plus a Float64 array like the destination
        arrays, info = plane_member(rng, f32, p, q, nin=2, kt=kt, rev=rev, other="dst", ddt=f64)
        third = hview(values(rng, (p, q), f64))
        c.calls.append((c.f, arrays + (third,)))
        c.info.append(dict(info, nin=3))
    out.append(c)
    return out


# ---- recipe `counts` ------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 5, 256, 257, 2049)


def tiny_member(rng, dt=np.float64):
    """1-40 elements, one workgroup"""
    if rng.integers(0, 2):
        a, b = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        return plane_member(rng, dt, a, b)
    return linear_member(rng, (int(rng.integers(1, 41)),), dt, 1)


def counts(dt=None, which=COUNTS):
    """Member counts at powers of two +- 1 and a few thousand: every depth of the member search.  Tiny members, with a two-workgroup linear
    member and a four-tile transposing member at the first, middle and last positions (in both assignments up to 257 members)."""
    out = []
    for K in which:
        for variant in ((0, 1) if K <= 257 else (0,)):
            rng = _rng(8, extra=2 * K + variant)
            c = Case("counts/%d/%s" % (K, "lt"[variant]), ident, "ident")
            special = {pos: (i + variant) % 2 for i, pos in enumerate(sorted({0, K // 2, K - 1}))}
            for i in range(K):
                if i not in special:
                    c.add(tiny_member(rng))
                elif special[i] == 0:
                    c.add(linear_member(rng, (CHUNK + 1,), np.float64, 1))
                else:
                    c.add(plane_member(rng, np.float64, 40, 40))
            out.append(c)
    return out


RECIPES = {"linear": (linear, FLOATS), "transposing": (transposing, FLOATS), "tmin": (tmin, [None]), "functors": (functors, FLOATS), "bitcopy": (bitcopy, [None]),
           "integer": (integer, [np.int32, np.int64, np.uint8]), "mixed": (mixed, [None]), "counts": (counts, [None])}


def recipe(name, dt=None):
    return RECIPES[name][0](dt)


# ---- the group of the sequence test ---------------------------------------------------------------------------------------------------
SEQ_GRID = 264


def slice_cuts(grid, slices):
    """Where a launch of `grid` workgroups is cut (csrc/smr_sched.cpp: slice_range): ceil(grid / slices) rounded up to a multiple of 8."""
    per = ((grid + slices - 1) // slices + 7) & ~7
    return [per * k for k in range(1, slices) if per * k < grid]


def sliced():
    """Carry-heavy linear members and ragged transposing members with outer dims, laid out between one-workgroup fillers so that the cuts of
    2, 3 and 4 slices fall strictly inside them.  Returns (case, cuts by number of slices)."""
    rng = _rng(9)
    dt = np.float64
    c = Case("sliced/float64", ident, "ident")
    cuts = {s: slice_cuts(SEQ_GRID, s) for s in (2, 3, 4)}
    targets = sorted({x for v in cuts.values() for x in v})

    def tr(i):
        p, q, before, after = [(33, 65, (2,), ()), (65, 31, (2,), (2,)), (17, 33, (), (3,))][i % 3]
        return plane_member(rng, dt, p, q, before, after, rev=("q", "p", "")[i % 3], step2=i % 2 == 1)

    def lin(i):
        return linear_member(rng, [(3,) * 7, (300, 7), (2, 3, 2, 3, 2, 3, 2, 3), (3, 5, 7, 11)][i % 4], dt, 1)

    spare = [lin(i) if i % 2 else tr(i // 2) for i in range(10)]   # placed wherever they fit between the targets
    cur = 0

    def put(m):
        nonlocal cur
        c.add(m)
        cur += m[1]["wgs"]

    for j, x in enumerate(targets):
        m = lin(j // 2) if j % 2 else tr(j // 2)   # alternately a transposing and a linear member around the cut
        first = x - m[1]["wgs"] // 2
        assert m[1]["wgs"] >= 2 and first >= cur
        while cur < first:
            if spare and spare[0][1]["wgs"] <= first - cur:
                put(spare.pop(0))
            else:
                put(plane_member(rng, dt, 5, 7))
        put(m)
    while cur < SEQ_GRID:
        if spare and spare[0][1]["wgs"] <= SEQ_GRID - cur:
            put(spare.pop(0))
        else:
            put(plane_member(rng, dt, 5, 7))
    assert cur == SEQ_GRID
    return c, cuts


def judge(case, i, want, got, alone, whole=None):
    """The assertions on member i of a case that ran (tests/test_gpu_group_fuzz.py): see Case."""
    msg = "%s member %d %s" % (case.name, i, case.info[i])
    arrays = case.calls[i][1]
    want = np.asarray(want)
    assert got.dtype == want.dtype == np.dtype(arrays[0].dtype) and got.shape == want.shape, msg

    def close(x, y):
        x, y = x.astype(np.complex128).ravel(), y.astype(np.complex128).ravel()
        return np.linalg.norm(x - y) <= rtol(arrays[0].dtype) * max(np.linalg.norm(x), np.linalg.norm(y), 1e-300)

    if case.exact:
        assert same_bits(got, want), msg + ": differs from the oracle"
    else:
        assert close(got, want), msg + ": not within rtol of the oracle"
    if case.alone_exact:
        assert same_bits(got, alone), msg + ": differs from the call issued alone"
    else:
        assert close(got, alone), msg + ": not within rtol of the call issued alone"
    if case.np_ref is not None:
        with np.errstate(over="ignore"):
            truth = case.np_ref(*[a.toarray() for a in arrays[1:]])
        assert truth.dtype == got.dtype and np.array_equal(got, truth), msg + ": differs from NumPy"
    if whole is not None:
        before, dev_after, host_after, idx = whole
        outside = np.ones(before.shape, dtype=bool)
        outside[idx.ravel()] = False
        assert same_bits(dev_after[outside], before[outside]), msg + ": elements of the parent outside the member changed"
        if case.exact:
            expect = before.copy()
            expect[idx.ravel()] = want.ravel()
            assert same_bits(dev_after, expect), msg + ": whole parent differs from the oracle's result put into it"
            if case.ref is None:
                assert same_bits(dev_after, host_after), msg + ": whole parent differs from the host parent the oracle wrote"
