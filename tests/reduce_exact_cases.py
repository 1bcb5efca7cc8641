"""Bit-exact reduction cases: one table for the CPU oracle (test_reduce_exact_oracle.py) and the HIP kernels
(test_gpu_reduce_exact.py).  Plain NumPy -- no GPU, no torch.

Every case's data is integer-valued (or a product of factors from {+-0.5, +-1, +-2}, or a min / max with planted
extremes), bounded so that every partial result, in any order of the reduction, is exactly representable: the sum of
magnitudes per output stays below 2^24 for Float32 / ComplexF32 and below 2^53 for the 64-bit types.  Every correct
reduction order then gives the same bits, and the expected value is computed from the integers (or by the exact rule of
the operator), never by a floating-point reduction.

Every input view sits inside a larger parent whose margins and gaps hold NaN (Bool: the value that would change the
result), so a stray read poisons the result; every destination parent is filled with the byte 0xA5 around and between the
destination's elements, and all of it must come back unchanged.

`expect` lists substrings of the plan's describe() that pin the kernel path (family, form, vector width, fold form);
`cell` names the entry of the coverage table (test_gpu_reduce_exact.py::test_every_cell_was_reached).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

F32, F64, C32, C64, BOOL = np.float32, np.float64, np.complex64, np.complex128, np.bool_
SENTINEL = 0xA5  # every destination byte that is not a destination element
ALIGN = 64       # parents start at a 64-byte boundary: views at element offset 0 are 16-byte aligned


def aligned_empty(n, dtype):
    dtype = np.dtype(dtype)
    raw = np.empty(n * dtype.itemsize + ALIGN, dtype=np.uint8)
    skip = (-raw.ctypes.data) % ALIGN
    return raw[skip:skip + n * dtype.itemsize].view(dtype)


def pattern(n, a, b, p, c):
    """x[i] = ((i * a + b) mod p) - c as int64: position-dependent, so a misplaced element changes the sum."""
    return (np.arange(n, dtype=np.int64) * a + b) % p - c


def _real(dt):
    return np.dtype(dt).kind != "c"


def _margin(dt):
    return max(1, 64 // np.dtype(dt).itemsize)  # 64 bytes: keeps a view at the margin 16-byte aligned


def _index(off, dims, strides):
    """Parent index of every view element (array of the view's shape)."""
    idx = np.full(dims, off, dtype=np.int64)
    for d, (n, s) in enumerate(zip(dims, strides)):
        sh = [1] * len(dims)
        sh[d] = n
        idx = idx + (np.arange(n, dtype=np.int64) * s).reshape(sh)
    return idx


@dataclass
class Operand:
    dtype: type
    plen: int          # parent length (elements)
    offset: int
    strides: tuple     # element strides of the view (0 along reduced dims for the destination)
    conj: bool = False
    parent: np.ndarray = None  # filled parent (sentinels + data)


@dataclass
class Case:
    name: str
    cell: str
    dims: tuple
    rdims: tuple
    op: str
    initop: object
    f: str                                  # "ident", "abs2", "mul" (x*y) or "prog" (2x - y + 1, runtime-compiled)
    ins: list
    dest: Operand
    want: np.ndarray                        # destination elements after the call (keepdims shape), NaN = any NaN
    options: dict = field(default_factory=dict)
    expect: tuple = ()
    note: str = ""
    wants: dict = None                      # reduce_fuzz_cases.py: times -> destination elements after that many applications of the call

    @property
    def oshape(self):
        return tuple(1 if d in self.rdims else n for d, n in enumerate(self.dims))

    @property
    def nelem(self):
        return int(np.prod(self.dims))

    def expected_parent(self, times=1):
        """The destination parent as it must be after `times` applications of the call onto the same destination (more than one:
        cases that carry `wants`, computed like `want` in exact arithmetic)."""
        out = self.dest.parent.copy()
        w = self.want if times == 1 else self.wants[times]
        if self.dest.conj:
            w = np.conj(w)
        out[_index(self.dest.offset, self.oshape, self._ostrides())] = w
        return out

    def _ostrides(self):
        return tuple(0 if d in self.rdims else s for d, s in enumerate(self.dest.strides))

    def mismatch(self, got_parent, times=1):
        """None when `got_parent` (the destination's whole parent after `times` applications of the call) is right, else a message."""
        want = self.expected_parent(times)
        idx = _index(self.dest.offset, self.oshape, self._ostrides()).ravel()
        nanpos = idx[np.isnan(want[idx].astype(np.complex128))] if np.dtype(self.dest.dtype) != np.bool_ else idx[:0]
        gb = got_parent.copy()
        wb = want.copy()
        if len(nanpos):
            if not np.all(np.isnan(gb[nanpos].astype(np.complex128))):
                bad = nanpos[~np.isnan(gb[nanpos].astype(np.complex128))]
                return f"{self.name}: expected NaN at parent index {bad[:4].tolist()}, got {gb[bad[:4]].tolist()}"
            gb[nanpos] = 0
            wb[nanpos] = 0
        g8, w8 = gb.view(np.uint8), wb.view(np.uint8)
        if np.array_equal(g8, w8):
            return None
        es = np.dtype(self.dest.dtype).itemsize
        bad = np.unique(np.nonzero(g8 != w8)[0] // es)
        mine = set(idx.tolist())
        inside = [int(i) for i in bad if i in mine]
        outside = [int(i) for i in bad if i not in mine]
        msg = f"{self.name}:"
        if inside:
            msg += f" elements at parent index {inside[:4]}: got {gb[inside[:4]].tolist()} want {wb[inside[:4]].tolist()};"
        if outside:
            msg += f" {len(outside)} bytes-groups outside the destination written, first at {outside[:4]}"
        return msg


# ---- exact semantics ----------------------------------------------------------------------------------------------
def _init(initop, old):
    """initop applied to the destination's old values (object arrays of Python numbers)."""
    if initop is None:
        return old
    if initop == "zero":
        return np.zeros_like(old)
    if initop == "conj":
        return np.vectorize(lambda v: v.conjugate(), otypes=[object])(old)
    kind, beta = initop
    if kind == "scale":
        return old * beta
    return np.full_like(old, beta)


def _jl_minmax(vals, op):
    """Julia's min / max over a 1-d float array: NaN wins; max(-0.0, 0.0) = 0.0, min(-0.0, 0.0) = -0.0."""
    vals = np.asarray(vals, dtype=np.float64)
    if np.isnan(vals).any():
        return math.nan
    m = vals.max() if op == "max" else vals.min()
    if m == 0:
        zeros = vals[vals == 0]
        pos = (~np.signbit(zeros)).any()
        neg = np.signbit(zeros).any()
        return (0.0 if pos else -0.0) if op == "max" else (-0.0 if neg else 0.0)
    return float(m)


def _reduce_axes(arr, rdims, fn):
    """Apply fn to every output's reduced values (1-d) -> keepdims object array."""
    dims = arr.shape
    kept = [d for d in range(len(dims)) if d not in rdims]
    perm = kept + list(rdims)
    a = np.transpose(arr, perm)
    ko = tuple(dims[d] for d in kept)
    a = a.reshape(ko + (-1,))
    out = np.empty(ko, dtype=object)
    for i in np.ndindex(*ko):
        out[i] = fn(a[i])
    return out.reshape(tuple(1 if d in rdims else n for d, n in enumerate(dims)))


# ---- case construction --------------------------------------------------------------------------------------------
def _in_operand(dt, dims, vals, layout="dense", sentinel=None):
    """Input view of shape `dims` holding `vals` (array of the view's shape) inside a NaN-filled parent.
    layout: "dense" (column-major, aligned), "mis" (dense, one element past an aligned base), "step2" (stride 2 along
    dim 0), "rev" (1-d, stride -1), "box" (every dim stepped by 2: no unit stride, does not fuse), ("sub", pdims) (leading
    corner of a column-major array of shape pdims)."""
    m = _margin(dt)
    n = int(np.prod(dims))
    if layout in ("dense", "mis"):
        strides, s = [], 1
        for d in dims:
            strides.append(s)
            s *= d
        off = m + (1 if layout == "mis" else 0)
        plen = n + 2 * m + 1
    elif layout == "step2":
        strides, s = [2], 2 * dims[0]
        for d in dims[1:]:
            strides.append(s)
            s *= d
        off, plen = m, 2 * n + 2 * m
    elif layout == "rev":
        assert len(dims) == 1
        strides, off, plen = [-1], m + n - 1, n + 2 * m
    elif layout == "box":
        strides, s = [], 2
        for d in dims:
            strides.append(s)
            s *= 2 * d + 1
        off, plen = m, s + 2 * m
    elif isinstance(layout, tuple) and layout[0] == "sub":  # ("sub", parent dims): the leading corner of a larger array
        pdims = layout[1]
        strides, s = [], 1
        for d in pdims:
            strides.append(s)
            s *= d
        off, plen = m, s + 2 * m
    else:
        raise ValueError(layout)
    parent = aligned_empty(plen, dt)
    if sentinel is None:
        parent[...] = (np.nan + 1j * np.nan) if not _real(dt) else np.nan
    else:
        parent[...] = sentinel
    parent[_index(off, dims, strides)] = vals.astype(dt)
    return Operand(dt, plen, off, tuple(strides), parent=parent)


def _dest_operand(dt, dims, rdims, init_vals, dstep=1, conj=False, dstep_at=0):
    """Destination view (keepdims shape) with stride `dstep` along its kept dim number `dstep_at` (every other element
    of a column, or every other column), inside a 0xA5-filled parent."""
    oshape = tuple(1 if d in rdims else n for d, n in enumerate(dims))
    m = _margin(dt)
    # column-major over the kept dims, kept dim number dstep_at stepped by dstep
    strides, s, kept = [], 1, 0
    for d, n in enumerate(dims):
        if d in rdims:
            strides.append(0)
            continue
        if kept == dstep_at:
            s *= dstep
        strides.append(s)
        s *= n
        kept += 1
    nout = int(np.prod(oshape))
    span = _index(0, oshape, [0 if d in rdims else strides[d] for d in range(len(dims))]).max() + 1 if nout else 0
    plen = int(span) + 2 * m
    parent = aligned_empty(plen, dt)
    parent.view(np.uint8)[...] = SENTINEL
    v = np.asarray(init_vals).reshape(oshape)
    parent[_index(m, oshape, [0 if d in rdims else strides[d] for d in range(len(dims))])] = np.conj(v) if conj else v
    return Operand(dt, plen, m, tuple(strides), conj=conj, parent=parent)


def _obj(re, im=None):
    """Exact Python numbers (complex when `im` is given) as an object array."""
    out = np.empty(re.shape, dtype=object)
    flat = out.reshape(-1)
    r = re.reshape(-1).tolist()
    if im is None:
        flat[:] = r
    else:
        flat[:] = [complex(a, b) for a, b in zip(r, im.reshape(-1).tolist())]
    return out


def _to_dt(obj, dt):
    """Object array of exact Python numbers -> dtype (exact by construction)."""
    if np.dtype(dt) == np.bool_:
        return obj.astype(bool)
    if _real(dt):
        return np.array([float(v.real) if isinstance(v, complex) else float(v) for v in obj.ravel()], dtype=dt).reshape(obj.shape)
    return np.array([complex(v) for v in obj.ravel()], dtype=dt).reshape(obj.shape)


def sum_case(name, cell, dims, rdims, dt, *, f="ident", initop="zero", layout="dense", layout2=None, dest_dt=None, dstep=1,
             dstep_at=0, dconj=False, options=None, expect=(), seed=0, note="", scale=(7, 3)):
    """op = + over integer-valued data mapped by f (ident / abs2 / mul / prog): the sums are taken over the integers."""
    n = int(np.prod(dims))
    p, c = scale
    cx = not _real(dt)
    re = pattern(n, 37 + seed, 5 + seed, p, c).reshape(dims, order="F")
    im = pattern(n, 53 + seed, 11 + seed, p, c - 1).reshape(dims, order="F") if cx else np.zeros_like(re)
    ins = [_in_operand(dt, dims, re + 1j * im if cx else re, layout)]
    if f in ("mul", "prog"):
        if layout2 == "bcast":  # one element read through stride 0 along every dim
            re2 = np.full(dims, 3, dtype=np.int64)
            im2 = np.full(dims, -2 if cx else 0, dtype=np.int64)
            o = _in_operand(dt, (1,), np.array([3 - 2j]) if cx else np.array([3]))
            o.strides = (0,) * len(dims)
            ins.append(o)
        else:
            re2 = pattern(n, 29 + seed, 2 + seed, 5, 2).reshape(dims, order="F")
            im2 = pattern(n, 31 + seed, 7 + seed, 5, 2).reshape(dims, order="F") if cx else np.zeros_like(re)
            ins.append(_in_operand(dt, dims, re2 + 1j * im2 if cx else re2, layout2 or layout))
        if f == "mul":
            mre, mim = re * re2 - im * im2, re * im2 + im * re2
        else:
            mre, mim = 2 * re - re2 + 1, 2 * im - im2
    elif f == "abs2":
        mre, mim = re * re + im * im, np.zeros_like(re)
    else:
        mre, mim = re, im
    pre = mre.sum(axis=tuple(rdims), keepdims=True)
    pim = mim.sum(axis=tuple(rdims), keepdims=True)
    ddt = dest_dt or dt
    dcx = not _real(ddt)
    no = int(pre.size)
    old = _obj(pattern(no, 3, 1, 9, 4).reshape(pre.shape), pattern(no, 5, 2, 9, 4).reshape(pre.shape) if dcx else None)
    want = _init(initop, old) + (_obj(pre, pim) if dcx else _obj(pre))
    dest = _dest_operand(ddt, dims, rdims, _to_dt(old, ddt), dstep, dconj, dstep_at)
    return Case(name, cell, tuple(dims), tuple(rdims), "+", initop, f, ins, dest, _to_dt(want, ddt), dict(options or {}), tuple(expect), note)


def prod_case(name, cell, dims, rdims, dt, *, zero_at=None, initop=None, options=None, expect=(), note=""):
    """op = * over factors from {+-0.5, +-1, +-2} with at most 50 factors of two and 50 of one half, so every partial
    product, in any order, lies in [2^-50, 2^50]: exact.  zero_at: linear index of a single 0.0 -- the result is then a
    zero whose sign is the XOR of all the factors' signs."""
    n = int(np.prod(dims))
    step = max(1, n // 640)
    e = pattern(n, 7, 3, 13, 0)
    e = np.where(e == 1, 1, np.where(e == 2, -1, 0)) * (np.arange(n) % step == 0)
    for v in (1, -1):  # keep the first 50 of each kind
        pos = np.nonzero(e == v)[0]
        e[pos[50:]] = 0
    sgn = np.where(pattern(n, 11, 1, 5, 0) == 0, -1.0, 1.0)
    vals = sgn * np.ldexp(1.0, e)
    if zero_at is not None:
        vals[zero_at] = 0.0
    vals = vals.reshape(dims, order="F")
    ins = [_in_operand(dt, dims, vals)]

    def exact(v):
        neg = bool(int(np.signbit(v).sum()) % 2)
        if (v == 0).any():
            return -0.0 if neg else 0.0
        return math.copysign(math.ldexp(1.0, int(np.round(np.log2(np.abs(v))).sum())), -1.0 if neg else 1.0)

    part = _reduce_axes(vals, rdims, exact)
    old = np.array([[-1.0, 1.0][i % 2] for i in range(part.size)], dtype=object).reshape(part.shape)
    want = _init(initop, old) * part  # IEEE products of exact values: signed zeros included
    dest = _dest_operand(dt, dims, rdims, _to_dt(old, dt))
    return Case(name, cell, tuple(dims), tuple(rdims), "*", initop, "ident", ins, dest, _to_dt(want, dt), dict(options or {}), tuple(expect), note)


def minmax_case(name, cell, dims, rdims, dt, op, *, plant=(), nan_at=(), zeros=False, inf=False, layout="dense", options=None,
                expect=(), note=""):
    """op = min / max: integer data with a unique extreme planted at each linear index (column-major over the view) of
    `plant`, NaN at `nan_at`; zeros=True: all data +-0.0; inf=True: the planted extremes are +-Inf.  initop = nothing:
    the destination holds the opposite zero of the expected one (max: -0.0, min: +0.0) or a value that never wins."""
    n = int(np.prod(dims))
    sgn = 1.0 if op == "max" else -1.0
    if zeros:
        vals = np.where(pattern(n, 13, 2, 3, 0) == 0, 0.0, -0.0) * (1 if op == "min" else 1)
        if op == "min":
            vals = -vals  # mostly +0.0: the -0.0 must win
    else:
        vals = pattern(n, 41, 7, 101, 50).astype(np.float64)
    for k, i in enumerate(plant):
        vals[i] = sgn * (math.inf if inf else 1000.0 + k)
    for i in nan_at:
        vals[i] = math.nan
    vals = vals.reshape(dims, order="F")
    ins = [_in_operand(dt, dims, vals, layout)]
    part = _reduce_axes(vals, rdims, lambda v: _jl_minmax(v, op))
    oldv = (-0.0 if op == "max" else 0.0) if zeros else -sgn * 999.0
    want = np.empty(part.shape, dtype=object)
    for i in np.ndindex(*part.shape):
        want[i] = _jl_minmax([oldv, part[i]], op)
    dest = _dest_operand(dt, dims, rdims, np.full(part.shape, oldv, dtype=dt))
    return Case(name, cell, tuple(dims), tuple(rdims), op, None, "ident", ins, dest, _to_dt(want, dt), dict(options or {}), tuple(expect), note)


def inf_sum_case(name, cell, n, dt, *, pos_at, neg_at=None, expect=()):
    """+ with +Inf (and -Inf): +Inf, or NaN when both occur."""
    vals = pattern(n, 37, 5, 7, 3).astype(np.float64)
    vals[pos_at] = math.inf
    if neg_at is not None:
        vals[neg_at] = -math.inf
    ins = [_in_operand(dt, (n,), vals)]
    want = np.array([math.nan if neg_at is not None else math.inf], dtype=dt)
    dest = _dest_operand(dt, (n,), (0,), np.zeros(1, dtype=dt))
    return Case(name, cell, (n,), (0,), "+", "zero", "ident", ins, dest, want, {}, tuple(expect))


def bool_case(name, cell, dims, rdims, op, *, flip_at=(), init=True, options=None, expect=()):
    """& / | over Bool: all true (&) or all false (|) except at `flip_at`; the parent's margins hold the value that
    would flip the result."""
    n = int(np.prod(dims))
    base = op == "&"
    vals = np.full(n, base)
    for i in flip_at:
        vals[i] = not base
    vals = vals.reshape(dims, order="F")
    ins = [_in_operand(BOOL, dims, vals, sentinel=not base)]
    part = _reduce_axes(vals, rdims, lambda v: bool(v.all()) if op == "&" else bool(v.any()))
    want = np.empty(part.shape, dtype=bool)
    for i in np.ndindex(*part.shape):
        want[i] = (init and part[i]) if op == "&" else (init or part[i])
    dest = _dest_operand(BOOL, dims, rdims, np.full(part.shape, init))
    return Case(name, cell, tuple(dims), tuple(rdims), op, None, "ident", ins, dest, want, dict(options or {}), tuple(expect))


# ---- the table ----------------------------------------------------------------------------------------------------
RA, RP = "family=reduce_all", "family=reduce_part"
K = 4096  # elements per REDUCE_ALL workgroup (256 lanes x 16): blocks = ceil(n / 4096), capped at reduce_blocks = 2048


def _all(v, fold, blocks=None):
    return (RA, f"vec={v} fold={fold}") + ((f"blocks={blocks} ",) if blocks else ())


def _part(form, v, fold, split=None):
    return (RP, f"form={form}", f"vec={v} fold={fold}") + ((f"split={split} ",) if split else ())


# position classes of REDUCE_ALL for min / max plants: n, vector width, {class: linear index}
#   vector, Float32 (V = 4): 18440 = 5 workgroups; workgroup b reads [4096 b, 4096 b + 4096); the last row of 64 vectors holds 2
#   vector, Float64 (V = 2): workgroup b reads [2048 b, +2048) and [2048 b + 10240, +2048); the last row is partial
#   scalar, Float32 (n odd): 5 workgroups of 256 lanes, element i is read by workgroup (i mod 1280) / 256
_PLANTS = {
    ("vec", "f32"): (18440, 4, {"first": 0, "last": 18439, "tail": 18436, "lastwg": 17000, "innerwg": 5000}),
    ("vec", "f64"): (18440, 2, {"first": 0, "last": 18439, "tail": 18436, "lastwg": 9000, "innerwg": 3000}),
    ("scalar", "f32"): (18441, 1, {"first": 0, "last": 18440, "tail": 18400, "lastwg": 3660, "innerwg": 6700}),
}


def table():
    """name -> zero-argument builder of the Case (built on demand: some inputs are tens of MiB)."""
    T = {}

    def add(name, fn, *a, **kw):
        assert name not in T, name
        T[name] = lambda: fn(name, *a, **kw)

    # -- REDUCE_ALL: one workgroup, in-launch fold, second launch ------------------------------------------------------
    add("all_1000_f32", sum_case, "all:one:scalar", (1000,), (0,), F32, expect=_all(1, "epilogue", 1))
    add("all_4096_f32", sum_case, "all:one:vec", (K,), (0,), F32, expect=_all(4, "epilogue", 1))
    add("all_4097_f32", sum_case, "all:fold:scalar", (K + 1,), (0,), F32, expect=_all(1, "in-launch", 2))
    add("all_4100_f32", sum_case, "all:fold:vec", (K + 4,), (0,), F32, expect=_all(4, "in-launch", 2))
    add("all_64blk_f32", sum_case, "all:fold:64", (64 * K,), (0,), F32, expect=_all(4, "in-launch", 64))
    add("all_65blk_f32", sum_case, "all:second:65", (64 * K + 4,), (0,), F32, expect=_all(4, "second-launch", 65))
    add("all_capped_f32", sum_case, "all:second:capped", (2048 * K + 3 * K,), (0,), F32, scale=(5, 2),
        expect=_all(4, "second-launch", 2048))
    add("all_rs0_2blk_f32", sum_case, "all:second:rs0", (K + 4,), (0,), F32, options={"reduce_single": 0},
        expect=_all(4, "second-launch", 2))
    add("all_rs0_64blk_f64", sum_case, "all:second:rs0", (64 * K,), (0,), F64, options={"reduce_single": 0},
        expect=_all(2, "second-launch", 64))
    # -- REDUCE_ALL, scalar by layout -------------------------------------------------------------------------------
    add("all_misaligned_f32", sum_case, "all:scalar:misaligned", (3 * K,), (0,), F32, layout="mis", expect=_all(1, "in-launch", 3))
    add("all_stride2_f32", sum_case, "all:scalar:stride2", (3 * K,), (0,), F32, layout="step2", expect=_all(1, "in-launch", 3))
    add("all_reversed_f64", sum_case, "all:scalar:reversed", (3 * K,), (0,), F64, layout="rev", expect=(RA, "fold=in-launch"))
    add("all_box_f32", sum_case, "all:scalar:box", (60, 120), (0, 1), F32, layout="box", expect=("fold=in-launch", "vec=1"))
    add("all_bcast_mul_f32", sum_case, "all:vec:bcast", (3 * K,), (0,), F32, f="mul", layout2="bcast", expect=_all(4, "in-launch", 3))
    add("all_ntload0_f32", sum_case, "all:ntload0", (8 * K,), (0,), F32, options={"nt_load": 0}, expect=_all(4, "in-launch", 8))
    add("all_ntload1_f32", sum_case, "all:ntload1", (8 * K,), (0,), F32, options={"nt_load": 1}, expect=_all(4, "in-launch", 8))
    # -- REDUCE_ALL: every float type, initops, destinations ---------------------------------------------------------
    add("all_f64_none", sum_case, "all:f64", (3 * K + 2,), (0,), F64, initop=None, expect=_all(2, "in-launch", 4))
    add("all_c64_scale_cx", sum_case, "all:c32", (3 * K,), (0,), C32, initop=("scale", 2 - 1j), expect=_all(2, "in-launch", 3))
    add("all_c128_fold", sum_case, "all:c64:fold", (3 * K,), (0,), C64, initop="conj",
        note="16-byte partials published as two 8-byte write-through stores", expect=_all(1, "in-launch", 3))
    add("all_c128_second", sum_case, "all:c64", (70 * K,), (0,), C64, initop=("const", 3 + 4j), scale=(5, 2),
        expect=_all(1, "second-launch", 70))
    add("all_f32_scale3", sum_case, "all:f32:scale", (K + 4,), (0,), F32, initop=("scale", 3), expect=_all(4, "in-launch", 2))
    add("all_c64_conjdest", sum_case, "all:conjdest", (K + 4,), (0,), C32, initop=None, dconj=True, expect=_all(2, "in-launch", 2))
    add("all_mixed_f32_to_f64", sum_case, "all:mixed", (1 << 20,), (0,), F32, dest_dt=F64, scale=(61, 0), seed=2,
        note="Float32 accumulation would round: the exact sum is odd and above 2^24", expect=(RA, "(mixed)", "vec=1"))
    # -- REDUCE_ALL functor paths on the vector path -------------------------------------------------------------------
    add("all_abs2_f32", sum_case, "all:f:abs2", (3 * K,), (0,), F32, f="abs2", expect=_all(4, "in-launch", 3) + ("f=abs2",))
    add("all_mul_f64", sum_case, "all:f:mul", (3 * K,), (0,), F64, f="mul", expect=_all(2, "in-launch", 3) + ("f=mul2",))
    add("all_prog_f32", sum_case, "all:f:jit", (3 * K,), (0,), F32, f="prog", options={"jit": 1}, expect=_all(4, "in-launch", 3) + ("f=prog",))
    add("all_prog_interp_c64", sum_case, "all:f:interp", (3 * K,), (0,), C32, f="prog", options={"jit": 0},
        expect=_all(2, "in-launch", 3) + ("f=prog",))
    # -- REDUCE_ALL: *, min, max, +-Inf, &, | --------------------------------------------------------------------------
    add("all_prod_f32", prod_case, "all:prod", (3 * K,), (0,), F32, expect=_all(4, "in-launch", 3))
    add("all_prod_f64_65", prod_case, "all:prod", (65 * K,), (0,), F64, expect=_all(2, "second-launch", 65))
    add("all_prod_zero_f64", prod_case, "all:prod:zero", (3 * K,), (0,), F64, zero_at=5000, expect=_all(2, "in-launch", 3))
    for (path, tn), (n, v, pos) in _PLANTS.items():
        dt = F32 if tn == "f32" else F64
        for cls, i in pos.items():
            for op in ("max", "min"):
                add(f"all_{op}_{path}_{tn}_{cls}", minmax_case, f"all:{op}", (n,), (0,), dt, op, plant=(i,), expect=_all(v, "in-launch", 5))
            add(f"all_nan_{path}_{tn}_{cls}", minmax_case, "all:nan", (n,), (0,), dt, "max" if cls in ("first", "tail") else "min",
                nan_at=(i,), expect=_all(v, "in-launch", 5))
    add("all_max_zeros_f32", minmax_case, "all:zeros", (18440,), (0,), F32, "max", zeros=True, expect=_all(4, "in-launch", 5))
    add("all_min_zeros_f64", minmax_case, "all:zeros", (18440,), (0,), F64, "min", zeros=True, expect=_all(2, "in-launch", 5))
    add("all_max_inf_f64", minmax_case, "all:inf", (18440,), (0,), F64, "max", plant=(9000,), inf=True, expect=_all(2, "in-launch", 5))
    add("all_min_inf_f32", minmax_case, "all:inf", (18441,), (0,), F32, "min", plant=(18440,), inf=True, expect=_all(1, "in-launch", 5))
    add("all_sum_inf_f32", inf_sum_case, "all:suminf", 3 * K, F32, pos_at=7000, expect=_all(4, "in-launch", 3))
    add("all_sum_infnan_f64", inf_sum_case, "all:suminf", 3 * K, F64, pos_at=7000, neg_at=11, expect=_all(2, "in-launch", 3))
    add("all_and_bool", bool_case, "all:bool", (3 * K,), (0,), "&", flip_at=(12287,), expect=(RA, "fold=in-launch"))
    add("all_or_bool", bool_case, "all:bool", (3 * K,), (0,), "|", flip_at=(4096,), init=False, expect=(RA, "fold=in-launch"))
    add("all_or_bool_none", bool_case, "all:bool", (3 * K,), (0,), "|", init=False, expect=(RA, "fold=in-launch"))
    # -- REDUCE_PART, general form -------------------------------------------------------------------------------------
    add("gen_forced_f32", sum_case, "gen:forced", (512, 40), (0,), F32, options={"reduce_part_kind": 0}, expect=_part("general", 1, "epilogue"))
    add("gen_natural_f64", sum_case, "gen:natural", (512, 40), (0,), F64, layout="step2", dstep=2, expect=_part("general", 1, "epilogue"))
    add("gen_fold_f32", sum_case, "gen:fold", (65536, 2), (0,), F32, layout="step2", expect=_part("general", 1, "in-launch"))
    add("gen_second_c64", sum_case, "gen:second", (131072, 2), (0,), C32, layout="step2", initop=("scale", 2), expect=_part("general", 1, "second-launch"))
    add("gen_max_f64", minmax_case, "gen:max", (512, 40), (0,), F64, "max", layout="step2", plant=(511,), nan_at=(512 * 7 + 3,),
        expect=_part("general", 1, "epilogue"))
    add("gen_and_bool", bool_case, "gen:bool", (512, 40), (0,), "&", flip_at=(700,), options={"reduce_part_kind": 0}, expect=_part("general", 1, "epilogue"))
    # -- ROW ----------------------------------------------------------------------------------------------------------
    add("row_vec_f32", sum_case, "row:vec:1", (K, 8), (0,), F32, dstep=2, expect=_part("row", 4, "epilogue", 1))
    add("row_scalar_f32", sum_case, "row:scalar:1", (K - 1, 8), (0,), F32, expect=_part("row", 1, "epilogue", 1))
    add("row_fold_f32", sum_case, "row:vec:fold", (32768, 2), (0,), F32, expect=_part("row", 4, "in-launch"))
    add("row_fold_scalar_f64", sum_case, "row:scalar:fold", (16383, 2), (0,), F64, initop=None, expect=_part("row", 1, "in-launch"))
    add("row_second16_f32", sum_case, "row:second:16", (131072, 2), (0,), F32, expect=_part("row", 4, "second-launch", 16))
    add("row_second64_f32", sum_case, "row:second:64", (1 << 19, 2), (0,), F32, initop=("const", -7), expect=_part("row", 4, "second-launch", 64))
    add("row_subbox_f32", sum_case, "row:subbox", (500, 300), (0, 1), F32, layout=("sub", (512, 384)), expect=_part("row", 4, "second-launch", 17) + ("nout=1 ",))
    add("row_abs2_f64", sum_case, "row:f:abs2", (K, 8), (0,), F64, f="abs2", expect=_part("row", 2, "epilogue"))
    add("row_mul_c64", sum_case, "row:f:mul", (K, 8), (0,), C32, f="mul", dconj=True, initop=None, expect=_part("row", 2, "epilogue"))
    add("row_prog_f32", sum_case, "row:f:jit", (K, 8), (0,), F32, f="prog", options={"jit": 1}, expect=_part("row", 4, "epilogue"))
    add("row_prog_interp_f64", sum_case, "row:f:interp", (K, 8), (0,), F64, f="prog", options={"jit": 0}, expect=_part("row", 2, "epilogue"))
    add("row_prod_f32", prod_case, "row:prod", (32768, 2), (0,), F32, expect=_part("row", 4, "in-launch"))
    add("row_max_f32", minmax_case, "row:max", (K, 8), (0,), F32, "max", plant=(K * 5 + 4095,), nan_at=(3 * K,), expect=_part("row", 4, "epilogue"))
    add("row_min_zeros_f64", minmax_case, "row:zeros", (16384, 2), (0,), F64, "min", zeros=True, expect=_part("row", 2, "in-launch"))
    add("row_max_zeros_f32", minmax_case, "row:zeros", (131072, 2), (0,), F32, "max", zeros=True, expect=_part("row", 4, "second-launch"))
    add("row_or_bool", bool_case, "row:bool", (K, 8), (0,), "|", flip_at=(K * 7 + 1,), init=False, expect=(RP, "form=row"))
    # -- COL ----------------------------------------------------------------------------------------------------------
    add("col_pow2_f32", sum_case, "col:pow2", (128, 64, 4), (1,), F32, dstep=2, dstep_at=1, expect=_part("col", 4, "epilogue", 1) + ("lanes_per_out=8 ",))
    add("col_exact_f32", sum_case, "col:exact:f32", (100, 2000), (1,), F32, expect=_part("col", 4, "second-launch", 25) + ("lanes=25x10",))
    add("col_exact_f64", sum_case, "col:exact:f64", (100, 2000), (1,), F64, expect=_part("col", 2, "second-launch", 50) + ("lanes=50x5",))
    add("col_scalar_f32", sum_case, "col:scalar", (127, 64), (1,), F32, expect=_part("col", 1, "epilogue"))
    add("col_fold_f32", sum_case, "col:fold", (128, 256), (1,), F32, expect=_part("col", 4, "in-launch"))
    add("col_second_f32", sum_case, "col:second", (64, 65536), (1,), F32, initop=("scale", -2), expect=_part("col", 4, "second-launch"))
    add("col_rs0_f64", sum_case, "col:rs0", (128, 256), (1,), F64, options={"reduce_single": 0}, expect=_part("col", 2, "second-launch"))
    add("col_rsbig_f32", sum_case, "col:rsbig", (64, 65536), (1,), F32, options={"reduce_single": 1 << 20}, expect=_part("col", 4, "in-launch"))
    add("col_exact_split_f32", sum_case, "col:exact:split", (100, 90, 80, 7), (1, 2, 3), F32, scale=(5, 2),
        expect=_part("col", 4, "second-launch", 512) + ("lanes=25x10",))
    add("col_c128", sum_case, "col:c64", (128, 256), (1,), C64, initop="conj", expect=_part("col", 1, "in-launch"))
    add("col_abs2_f32", sum_case, "col:f:abs2", (128, 64), (1,), F32, f="abs2", expect=_part("col", 4, "epilogue"))
    add("col_mul_f64", sum_case, "col:f:mul", (128, 64), (1,), F64, f="mul", expect=_part("col", 2, "epilogue"))
    add("col_prog_c64", sum_case, "col:f:jit", (128, 64), (1,), C32, f="prog", options={"jit": 1}, expect=_part("col", 2, "epilogue"))
    add("col_prog_interp_f32", sum_case, "col:f:interp", (128, 64), (1,), F32, f="prog", options={"jit": 0}, expect=_part("col", 4, "epilogue"))
    add("col_prod_f64", prod_case, "col:prod", (128, 256), (1,), F64, expect=_part("col", 2, "in-launch"))
    add("col_min_f32", minmax_case, "col:min", (128, 256), (1,), F32, "min", plant=(128 * 255 + 127,), nan_at=(128 * 200 + 64,),
        expect=_part("col", 4, "in-launch"))
    add("col_max_zeros_f64", minmax_case, "col:zeros", (128, 64), (1,), F64, "max", zeros=True, expect=_part("col", 2, "epilogue"))
    add("col_and_bool", bool_case, "col:bool", (128, 64), (1,), "&", flip_at=(128 * 30 + 5,), expect=(RP, "form=col"))
    return T


CELLS = sorted({"all:one:scalar", "all:one:vec", "all:fold:scalar", "all:fold:vec", "all:fold:64", "all:second:65",
                "all:second:capped", "all:second:rs0", "all:scalar:misaligned", "all:scalar:stride2", "all:scalar:reversed",
                "all:scalar:box", "all:vec:bcast", "all:ntload0", "all:ntload1", "all:c64:fold", "gen:forced", "gen:natural",
                "row:vec:1", "row:scalar:1", "row:vec:fold", "row:scalar:fold", "row:second:16", "row:second:64", "row:subbox",
                "col:pow2", "col:exact:f32", "col:exact:f64", "col:scalar", "col:fold", "col:second", "col:rs0", "col:rsbig",
                "all:f:abs2", "all:f:mul", "all:f:jit", "all:f:interp", "row:f:abs2", "row:f:mul", "row:f:jit", "row:f:interp",
                "col:f:abs2", "col:f:mul", "col:f:jit", "col:f:interp"})
