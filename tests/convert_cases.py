"""Table of converting calls: every kernel family with operands whose element type is not the compute type, checked against a model of
Julia's conversions and per-operation typing that is written here from Julia's rules (no torch, nothing from strided_jl_amd/expr.py).

The model
  promote_type   any float beats any integer; among floats the widest wins; complex if any operand is; among integers the wider wins, at
                 equal width unsigned wins; Bool yields to everything.
  literals       a Python int is an Int64, a Python float a Float64, an np.float32 a Float32.
  + - * min max  convert both arguments to the promoted type (round to nearest even) and operate in it; + - * of integers convert by
                 wrapping (`a % T`); Bool + Bool and Bool - Bool are Int64, Bool * Bool is Bool, Bool * float is ifelse(b, x, copysign(0, x)).
  /              of two integers is Float64, else in the promoted type.
  real (.) complex   Julia's own methods: x + z = Complex(x + re, im), z * x = Complex(re * x, im * x), z / x = Complex(re / x, im / x).
  comparisons    mathematical (an Int32 against a Float32 is compared exactly), Bool.
  sqrt           of an integer is Float64.
  store          convert(eltype(dest), v): float to narrower float rounds once; float to integer / Bool is defined for integer-valued
                 values in range only, complex to real for a zero imaginary part only.  Julia throws for the rest; the table holds defined
                 conversions only and `convert` asserts that.
`evaluate` walks an expression tree operation by operation in NumPy scalar types with an explicit astype at every conversion and returns
an array of the Julia element type.  The same tree gives the function handed to the library (`library_function`).

Documented limit kept by the table: an integer-typed sub-expression inside a float-class call is computed in Float64 on the device (exact
below 2^53, no wrap to the Julia integer type), so such sub-expressions stay inside the range of their Julia type.

Rows: every operand is a window of a padded parent (window_cases.layout / aligned_root); NaN (integers: the type's minimum) surrounds the
inputs, random finite bits surround the destination, and `Row.mismatch` (window_cases.Case.mismatch) compares the destination's WHOLE
parent byte for byte with the model's result written into a copy.  Reductions with + and * use exact data only (Julia converts on every
step, so only data whose every partial result is representable in the destination type is bit-defined; the bound is recomputed from the data);
max / min take the full value sets (rounding is monotone).  Every row names the cell (family and form) it is meant to reach;
tests/test_convert_host.py asserts from describe() that it does."""
import numpy as np

import strided_jl_amd as S
import window_cases as W
from reduce_exact_cases import pattern

fn = S.fn
B, I8, I16, I32, I64, U8, U16, U32, U64, F32, F64, C32, C64 = [np.dtype(t) for t in (
    np.bool_, np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.complex64, np.complex128)]
INTS = (B, I8, I16, I32, I64, U8, U16, U32, U64)
FLOATS = (F32, F64, C32, C64)
NAMES = {B: "Bool", I8: "Int8", I16: "Int16", I32: "Int32", I64: "Int64", U8: "UInt8", U16: "UInt16", U32: "UInt32", U64: "UInt64",
         F32: "Float32", F64: "Float64", C32: "ComplexF32", C64: "ComplexF64"}


def is_cx(t):
    return np.dtype(t).kind == "c"


def is_float(t):
    return np.dtype(t).kind in "fc"


def is_int(t):
    return np.dtype(t).kind in "biu"


def real_of(t):
    t = np.dtype(t)
    return {C32: F32, C64: F64}.get(t, t)


def complex_of(t):
    return C32 if real_of(t) == F32 else C64


def int_range(t):
    t = np.dtype(t)
    return (0, 1) if t == B else (int(np.iinfo(t).min), int(np.iinfo(t).max))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def promote_type(*ts):
    ts = [np.dtype(t) for t in ts]
    r = ts[0]
    for t in ts[1:]:
        r = _promote2(r, t)
    return r


def _promote2(a, b):
    if a == b:
        return a
    cx = is_cx(a) or is_cx(b)
    ra, rb = real_of(a), real_of(b)
    if ra.kind == "f" or rb.kind == "f":
        fl = [t for t in (ra, rb) if t.kind == "f"]
        r = max(fl, key=lambda t: t.itemsize)
    elif ra == B or rb == B:
        r = rb if ra == B else ra
    elif ra.itemsize != rb.itemsize:
        r = ra if ra.itemsize > rb.itemsize else rb
    else:
        r = ra if ra.kind == "u" else rb
    return complex_of(r) if cx else r


def convert(x, T, wrap=False):
    """Julia's convert(T, x) elementwise; wrap: `x % T` between integer types (what + - * of mixed integers do)."""
    x, T = np.asarray(x), np.dtype(T)
    s = x.dtype
    if s == T:
        return x
    if is_cx(s) and not is_cx(T):
        assert np.all(x.imag == 0), "InexactError: %s(%s) of a non-zero imaginary part" % (NAMES[T], NAMES[s])
        return convert(np.ascontiguousarray(x.real), T)
    if is_cx(T):
        out = np.empty(x.shape, T)
        R = real_of(T)
        out.real = convert(np.ascontiguousarray(x.real), R)
        out.imag = convert(np.ascontiguousarray(x.imag), R) if is_cx(s) else R.type(0)
        return out
    if T.kind == "f":
        with np.errstate(over="ignore"):
            return x.astype(T)   # an integer or a wider float: one rounding to nearest even
    if s == B:
        return x.astype(T)
    lo, hi = int_range(T)
    if s.kind == "f":
        assert np.all(np.isfinite(x)) and np.all(x == np.floor(x)), "InexactError: %s of a non-integer %s" % (NAMES[T], NAMES[s])
        d = x.astype(np.float64)
        assert np.all(d >= float(lo)) and np.all(d < float(hi + 1)), "InexactError: out of the range of %s" % NAMES[T]   # (hi + 1: a power of two)
        if T == B:
            return d != 0
        if T == U64:   # through Python integers: exact on [2^63, 2^64) too
            return np.array([int(v) for v in d.ravel()], dtype=object).astype(np.uint64).reshape(d.shape)
        return d.astype(np.int64).astype(T)
    # integer to integer
    if not wrap:
        slo, shi = int_range(s)
        if slo < lo or shi > hi:
            ok = (x.astype(object) >= lo) & (x.astype(object) <= hi)
            assert np.all(ok), "InexactError: %s(%s)" % (NAMES[T], NAMES[s])
    if T == B:
        return x != 0
    return x.astype(T)


def _signbit_pick(a, b, want_negative):
    """of two equal zeros (or equal values) the one whose sign bit is `want_negative`, if either has it"""
    return np.where(np.signbit(a) == want_negative, a, b)


def jl_minmax(op, a, b):
    """Julia's min / max of two arrays of one real type: NaN if either is NaN; min(-0.0, 0.0) = -0.0, max(-0.0, 0.0) = 0.0."""
    if a.dtype.kind != "f":
        return np.minimum(a, b) if op == "min" else np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        r = np.where(a < b, a, b) if op == "min" else np.where(a > b, a, b)
        r = np.where(a == b, _signbit_pick(a, b, op == "min"), r)
    r = np.where(np.isnan(a) | np.isnan(b), a.dtype.type(np.nan), r)
    return r.astype(a.dtype)


def _cx(re, im):
    out = np.empty(np.broadcast(re, im).shape, complex_of(re.dtype))
    out.real, out.imag = re, im
    return out


def jl_binary(op, a, b):
    a, b = np.asarray(a), np.asarray(b)
    ta, tb = a.dtype, b.dtype
    if op in ("lt", "le", "gt", "ge"):
        assert not is_cx(ta) and not is_cx(tb)
        for t in (ta, tb):
            assert t.itemsize < 8 or t == F64, "the model compares through Float64, which holds every value of these types"
        x, y = a.astype(np.float64), b.astype(np.float64)
        with np.errstate(invalid="ignore"):
            return {"lt": x < y, "le": x <= y, "gt": x > y, "ge": x >= y}[op]
    if is_cx(ta) or is_cx(tb):
        re_a, im_a = (np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)) if is_cx(ta) else (a, None)
        re_b, im_b = (np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)) if is_cx(tb) else (b, None)
        R = real_of(promote_type(ta, tb))
        if op in ("add", "sub"):
            re = jl_binary(op, re_a, re_b)
            if im_a is not None and im_b is not None:
                im = jl_binary(op, im_a, im_b)
            elif im_a is not None:
                im = im_a
            else:
                im = im_b if op == "add" else -im_b
            return _cx(convert(re, R), convert(im, R))
        if op == "mul" and (im_a is None or im_b is None):
            if im_b is None:
                return _cx(convert(jl_binary("mul", re_a, b), R), convert(jl_binary("mul", im_a, b), R))
            return _cx(convert(jl_binary("mul", a, re_b), R), convert(jl_binary("mul", a, im_b), R))
        if op == "div" and im_b is None:
            return _cx(convert(jl_binary("div", re_a, b), R), convert(jl_binary("div", im_a, b), R))
        raise NotImplementedError("the model has no %s of %s and %s" % (op, NAMES[ta], NAMES[tb]))
    T = promote_type(ta, tb)
    with np.errstate(all="ignore"):
        if op == "div":
            if is_int(T):
                T = F64
            return (convert(a, T) / convert(b, T)).astype(T)
        if op in ("min", "max"):
            return jl_minmax(op, convert(a, T), convert(b, T))
        if ta == B and tb == B:
            if op == "mul":
                return a & b
            T = I64
        if op == "mul" and (ta == B) != (tb == B) and T.kind == "f":   # *(x::Bool, y::AbstractFloat) = ifelse(x, y, copysign(zero(y), y))
            m, y = (a, convert(b, T)) if ta == B else (b, convert(a, T))
            return np.where(m, y, np.copysign(T.type(0), y)).astype(T)
        x, y = convert(a, T, wrap=True), convert(b, T, wrap=True)
        r = {"add": np.add, "sub": np.subtract, "mul": np.multiply}[op](x, y)
        return np.asarray(r).astype(T)


def jl_unary(op, a):
    a = np.asarray(a)
    if op == "sqrt":
        x = a if a.dtype.kind in "fc" else convert(a, F64)
        assert not is_cx(x.dtype) and np.all(x >= 0)   # (a negative argument is a DomainError)
        return np.sqrt(x)
    raise NotImplementedError(op)


# ---- expression trees: ("arg", k) | ("lit", value) | (op, child, ...) -------------------------------------------------------------------
def A(k):
    return ("arg", k)


def L(v):
    return ("lit", v)


def evaluate(tree, arrays):
    """The value of the tree on the arrays, typed and rounded operation by operation as Julia does it."""
    if tree[0] == "arg":
        return np.asarray(arrays[tree[1]])
    if tree[0] == "lit":
        v = tree[1]
        if isinstance(v, np.generic):
            return np.asarray(v)
        if isinstance(v, bool):
            return np.asarray(v, dtype=B)
        return np.asarray(v, dtype=I64 if isinstance(v, int) else F64)
    args = [evaluate(t, arrays) for t in tree[1:]]
    return jl_unary(tree[0], *args) if len(args) == 1 else jl_binary(tree[0], *args)


def result_type(tree, types):
    """The Julia element type of the tree for operands of these types (evaluated on one harmless element each)."""
    return evaluate(tree, [np.ones(1, dtype=t) for t in types]).dtype


def library_function(tree):
    """The same tree as a function for the library."""
    def go(t, xs):
        if t[0] == "arg":
            return xs[t[1]]
        if t[0] == "lit":
            return t[1]
        a = [go(c, xs) for c in t[1:]]
        if t[0] == "add":
            return a[0] + a[1]
        if t[0] == "sub":
            return a[0] - a[1]
        if t[0] == "mul":
            return a[0] * a[1]
        if t[0] == "div":
            return a[0] / a[1]
        if t[0] == "lt":
            return a[0] < a[1]
        return getattr(fn, t[0])(*a)   # min max sqrt
    return lambda *xs: go(tree, xs)


def show(tree):
    if tree[0] == "arg":
        return "x%d" % tree[1]
    if tree[0] == "lit":
        return repr(tree[1])
    return "%s(%s)" % (tree[0], ", ".join(show(t) for t in tree[1:]))


IDENT = A(0)


# ---- value sets -------------------------------------------------------------------------------------------------------------------------
def int_values(t):
    """the type's minimum and maximum, -1, 0, 1, the neighbourhood of 2^24 (where Float32 stops holding every integer), and the 32-bit edges
    whose Float32 image is a halfway case or lies next to one -- as far as the type holds them"""
    lo, hi = int_range(t)
    c = [lo, hi, -1, 0, 1] + [s * (2 ** 24 + d) for s in (1, -1) for d in (-1, 0, 1, 3)] + [2 ** 31 - 1, 2 ** 31 - 64, 2 ** 32 - 1, 2 ** 32 - 128]
    return sorted({v for v in c if lo <= v <= hi})


def _f32_neighbours(f):
    f = np.float32(f)
    nxt = np.nextafter(f, np.float32(np.inf))
    mid = (np.float64(f) + np.float64(nxt)) / 2   # exact: one more bit
    return [mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf)]


def f64_to_f32_values():
    """Float64 values around the roundings of Float32: halfway cases (ties to an even and to an odd neighbour) and their neighbours; the
    overflow threshold (2 - 2^-24) * 2^127 with its neighbours; values that become subnormals and zero; +-0.0, +-Inf, NaN"""
    out = []
    for base in (1.0, 1.5, 16777216.0, 0.1, 3.0e38, 1.1754944e-38, 7.0e-40):
        b = np.float32(base)
        out += _f32_neighbours(b) + _f32_neighbours(np.nextafter(b, np.float32(np.inf)))
    thr = (2.0 - 2.0 ** -24) * 2.0 ** 127
    out += [np.nextafter(thr, 0.0), thr, np.nextafter(thr, np.inf), float(np.finfo(np.float32).max), 1.0e39]
    out += [2.0 ** -149, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 2.0 ** -151, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, 2.0 ** -127, 2.0 ** -126 * (1 - 2.0 ** -30), 1.0e-60]
    out = [float(v) for v in out]
    out += [-v for v in out]
    return out + [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -2.5, 1.0 / 3.0, 1.0e10]


def f32_values():
    """Float32 values of every kind (widening is exact: the bits say whether it was)"""
    t = np.finfo(np.float32)
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, t.max, -t.max, t.tiny, -t.tiny, 2.0 ** -149, -2.0 ** -149, 2.0 ** -130, 1.0, -1.0, 0.1, 16777216.0, 16777218.0, 1.0 / 3.0, -2.5e-7]
    return [float(np.float32(x)) for x in v]


def _holds(ft, v):
    """does the float type hold the integer v exactly?"""
    p = 24 if real_of(ft) == F32 else 53
    v = abs(int(v))
    return v == 0 or (v >> max(0, v.bit_length() - p)) << max(0, v.bit_length() - p) == v


def float_to_int_values(ft, it):
    """every integer-valued edge of the integer type that the float type holds exactly: the edges of int_values, the largest value of the
    float type below each power-of-two bound, and for the 64-bit types the values around 2^63 and below 2^64"""
    lo, hi = int_range(it)
    p = 24 if real_of(ft) == F32 else 53
    c = set(int_values(it)) | {lo + 1, hi - 1, 2, 100, -100}
    for bound in (hi + 1, -lo, 2 ** 63, 2 ** 31, 2 ** 32, 2 ** 24):   # the float type's neighbours of these powers of two
        if bound > 1:
            ulp_below = max(1, bound >> p)
            c |= {bound - ulp_below, -(bound - ulp_below), bound, -bound, bound + 2 * ulp_below}
    if it == U64:
        c |= {2 ** 63 - 1024, 2 ** 63, 2 ** 63 + 2048, 2 ** 64 - 2048}
    if it == I64:
        c |= {-2 ** 63, 2 ** 63 - 1024}
    return sorted(v for v in c if lo <= v <= hi and _holds(ft, v))


def _spread(rng, n, specials, ordinary):
    """n values: every special at least once (when n allows), ordinary ones in between, in a fixed random order"""
    specials = list(specials)
    if n <= len(specials):
        vals = specials[:n]
    else:
        vals = specials + list(ordinary(n - len(specials)))
    vals = np.array(vals, dtype=object)
    return vals[rng.permutation(n)]


def conversion_data(rng, n, s, d):
    """n values of type s whose conversion to d is defined, the value sets of the pair in front"""
    s, d = np.dtype(s), np.dtype(d)
    rs = real_of(s)
    if is_int(s):
        lo, hi = int_range(s)
        if is_int(d):
            lo, hi = max(lo, int_range(d)[0]), min(hi, int_range(d)[1])
        sp = [v for v in int_values(s) if lo <= v <= hi]
        re = _spread(rng, n, sp, lambda k: [int(v) for v in rng.integers(max(lo, -2 ** 62), min(hi, 2 ** 62), size=k, endpoint=True)])
        return np.array([int(v) for v in re], dtype=object).astype(s)
    if is_int(d):
        sp = float_to_int_values(s, d)
        lo, hi = sp[0], sp[-1]
        bits = 24 if rs == F32 else 53
        re = _spread(rng, n, sp, lambda k: [int(v) for v in rng.integers(max(lo, -2 ** (bits - 1)), min(hi, 2 ** (bits - 1)), size=k, endpoint=True)])
        re = np.array([float(v) for v in re]).astype(rs)
    else:
        sp = f64_to_f32_values() if rs == F64 else f32_values()
        with np.errstate(over="ignore"):
            re = np.array(list(_spread(rng, n, sp, lambda k: rng.standard_normal(k) * 10.0 ** rng.integers(-3, 4, size=k))), dtype=np.float64).astype(rs)
    if not is_cx(s):
        return re
    out = np.empty(n, s)
    out.real = re
    if is_cx(d):
        out.imag = np.roll(re, 7)
    else:
        out.imag = np.where(np.arange(n) % 2 == 0, rs.type(0.0), rs.type(-0.0))   # complex to real: +0.0 and -0.0 imaginary parts
    return out


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def make_view(root, dims, perm, lo, hi, steps=None, bcast=()):
    """view of size dims over root; the dims in `bcast` have stride 0 (the parent has extent 1 there)"""
    e = [1 if i in bcast else n for i, n in enumerate(dims)]
    n, strides, off = W.layout(e, perm, lo, hi, steps)
    strides = tuple(0 if i in bcast else s for i, s in enumerate(strides))
    if root is None:
        return n
    assert root.size == n
    return S.StridedView(root, tuple(dims), strides, off)


def new_input(dims, perm, lo, hi, dt, data, steps=None):
    n = make_view(None, dims, perm, lo, hi, steps)
    root = W.aligned_root(n, dt)
    root[:] = W.poison(dt) if np.dtype(dt) != B else True
    v = make_view(root, dims, perm, lo, hi, steps)
    root[W.element_index(v).ravel()] = np.asarray(data, dtype=dt).ravel()
    return v


def new_dest(rng, dims, perm, lo, hi, dt, steps=None, bcast=(), old=None):
    n = make_view(None, dims, perm, lo, hi, steps, bcast)
    root = W.aligned_root(n, dt)
    root[:] = W.finite_bits(rng, n, dt) if np.dtype(dt) != B else rng.integers(0, 2, size=n).astype(B)
    v = make_view(root, dims, perm, lo, hi, steps, bcast)
    if old is not None:
        kept = S.StridedView(root, tuple(1 if i in bcast else m for i, m in enumerate(dims)), v.strides, v.offset)
        root[W.element_index(kept).ravel()] = np.asarray(old, dtype=dt).ravel()
    return v


# ---- reductions -----------------------------------------------------------------------------------------------------------------------
def sum_limit(t):
    """largest magnitude every integer up to which the type holds"""
    t = np.dtype(t)
    if t == B:
        return 1
    if is_int(t):
        return int_range(t)[1]
    return 2 ** 24 if real_of(t) == F32 else 2 ** 53


def exact_sum_data(dims, rdims, s, d, room):
    """integers (of dims' shape) whose sum of magnitudes per output stays <= min(limit of d, limit of s, 2^53) - room: every partial sum in
    any order is then an integer that the destination type holds (non-negative data when either type is unsigned: no partial sum is negative)"""
    n = int(np.prod(dims))
    nred = int(np.prod([dims[i] for i in rdims])) if rdims else 1
    lim = min(sum_limit(d), 2 ** 53) - room
    assert lim >= 1
    m = int(max(1, min(lim // nred, sum_limit(s), 40)))
    nonneg = np.dtype(s).kind in "bu" or np.dtype(d).kind in "bu"
    v = pattern(n, 7, 3, m + 1, 0) if nonneg else pattern(n, 7, 3, 2 * m + 1, m)
    v = v.reshape(dims)
    kept = [i for i in range(len(dims)) if i not in rdims]
    rows = np.transpose(v, kept + list(rdims)).reshape(int(np.prod([dims[i] for i in kept])) if kept else 1, nred)
    rows = rows * (np.cumsum(np.abs(rows), axis=1) <= lim)   # past the bound: zeros
    assert np.abs(rows).sum(axis=1).max() <= lim
    back = rows.reshape([dims[i] for i in kept] + [dims[i] for i in rdims])
    return np.transpose(back, np.argsort(kept + list(rdims)))


def exact_prod_data(dims, rdims, s, d):
    """factors 1 and -1 (1 alone when either type is unsigned) and a few 2s per output: every partial product in any order is plus or
    minus a power of two that both types hold, with room for an old destination of magnitude 1 scaled by 2"""
    n = int(np.prod(dims))
    nred = int(np.prod([dims[i] for i in rdims])) if rdims else 1
    signed = np.dtype(s).kind not in "bu" and np.dtype(d).kind not in "bu"
    kmax = max(0, min(6, sum_limit(d).bit_length() - 3, sum_limit(s).bit_length() - 1))
    v = np.where(pattern(n, 7, 3, 3, 0) == 0, -1, 1) if signed else np.ones(n, np.int64)
    two = (pattern(n, 11, 5, 13, 0) == 0).reshape(dims)
    kept = [i for i in range(len(dims)) if i not in rdims]
    order = kept + list(rdims)
    rows = np.transpose(two, order).reshape(-1, nred)
    rows = rows & (np.cumsum(rows, axis=1) <= (np.arange(rows.shape[0]) % (kmax + 1) if rows.shape[0] > 1 else np.array([kmax]))[:, None])   # 0 .. kmax factors of 2
    two = np.transpose(rows.reshape([dims[i] for i in order]), np.argsort(order))
    return v.reshape(dims) * np.where(two, 2, 1)


def _jl_reduce_minmax(op, x, axes):
    """Julia's minimum / maximum of Float64 data along axes: NaN wins, then the order with -0.0 < 0.0"""
    f = np.min if op == "min" else np.max
    with np.errstate(invalid="ignore"):
        r = f(np.where(np.isnan(x), 0.0, x), axis=axes, keepdims=True)
        zero_pick = np.any((x == 0) & (np.signbit(x) == (op == "min")), axis=axes, keepdims=True)
        r = np.where(r == 0, np.where(zero_pick, -0.0 if op == "min" else 0.0, 0.0 if op == "min" else -0.0), r)
    return np.where(np.any(np.isnan(x), axis=axes, keepdims=True), np.nan, r)


def reduce_model(op, initop, vals, old, rdims, d):
    """dest = op(initop(old), reduce(op, vals over rdims)) in the destination type d.  vals: the mapped values in their Julia type; old: the
    destination's present elements (kept shape).  +: exact integer data (asserted); min / max: any data (rounding is monotone)."""
    d = np.dtype(d)
    axes = tuple(rdims)
    kshape = tuple(1 if i in rdims else n for i, n in enumerate(vals.shape))
    old = np.asarray(old).reshape(kshape)
    if initop == "zero":
        init = np.zeros(kshape, d)
    elif initop is None:
        init = old
    else:
        assert initop[0] == "scale" and float(initop[1]).is_integer()
        init = None
    if op == "+":
        def ints(a):
            a = np.asarray(a)
            assert np.all(np.isfinite(a)) and np.all(a == np.round(a))
            return a.astype(np.int64) if not (is_int(a.dtype) and a.dtype.itemsize == 8) else a.astype(np.int64)
        parts = []
        for part in ((lambda a: np.ascontiguousarray(a.real)), (lambda a: np.ascontiguousarray(a.imag))) if (is_cx(vals.dtype) or is_cx(d)) else ((lambda a: a),):
            v = ints(part(vals))
            o = ints(part(old)) * (int(initop[1]) if init is None else 1) if initop != "zero" else np.zeros(kshape, np.int64)
            bound = np.abs(v).sum(axis=axes, keepdims=True) + np.abs(o) if axes else np.abs(v) + np.abs(o)
            assert bound.max() <= min(sum_limit(d), 2 ** 53), "a partial sum may not be representable in %s" % NAMES[d]
            if d.kind in "bu":
                assert v.min() >= 0 and o.min() >= 0
            parts.append((v.sum(axis=axes, keepdims=True) if axes else v) + o)
        if is_cx(d):
            return _cx(parts[0].astype(real_of(d)), parts[1].astype(real_of(d)))
        if len(parts) == 2:
            assert np.all(parts[1] == 0)
        return np.array([int(x) for x in parts[0].ravel()], dtype=object).astype(d).reshape(kshape)
    if op == "*":
        assert not is_cx(vals.dtype) and not is_cx(d) and initop != "zero"
        v, o = np.asarray(vals), np.asarray(old)
        assert np.all(v == np.round(v)) and np.all(o == np.round(o))
        v, o = v.astype(np.int64), o.astype(np.int64) * (int(initop[1]) if init is None else 1)
        bound = (np.abs(v).prod(axis=axes, keepdims=True) if axes else np.abs(v)) * np.abs(o)
        assert bound.max() <= min(sum_limit(d), sum_limit(vals.dtype), 2 ** 53), "a partial product may not be representable"
        if d.kind in "bu" or vals.dtype.kind in "bu":
            assert v.min() >= 0 and o.min() >= 0
        r = (v.prod(axis=axes, keepdims=True) if axes else v) * o
        return np.array([int(x) for x in r.ravel()], dtype=object).astype(d).reshape(kshape)
    assert op in ("min", "max") and not is_cx(vals.dtype) and not is_cx(d) and init is not None
    x = convert(vals, F64) if vals.dtype != F64 else vals
    for t in (vals.dtype, d):
        assert t.itemsize < 8 or t == F64 or np.all(np.abs(old.astype(object)) < 2 ** 53)
    r = _jl_reduce_minmax(op, x, axes) if axes else x
    r = jl_minmax(op, np.asarray(convert(init, F64), dtype=np.float64), np.asarray(r, dtype=np.float64))
    return convert(r, d)


# ---- rows -------------------------------------------------------------------------------------------------------------------------------
class Row(W.Case):
    """One call.  arrays[0] is the destination; `expected` is the destination's parent with the model's result in the view."""

    def __init__(self, spec, arrays, result):
        self.spec = spec
        self.name, self.cell, self.tree, self.dims = spec["name"], spec["cell"], spec["tree"], tuple(spec["dims"])
        self.op, self.initop, self.rdims, self.jit = spec.get("op"), spec.get("initop"), tuple(spec.get("rdims", ())), bool(spec.get("jit"))
        self.fname = show(self.tree)
        self.f = library_function(self.tree)
        self.arrays = tuple(arrays)
        self.roots = [a.parent for a in arrays]
        self.desc = ""
        dest = arrays[0]
        self.before = dest.parent.copy()
        kept = S.StridedView(dest.parent, tuple(1 if i in self.rdims else n for i, n in enumerate(self.dims)), dest.strides, dest.offset)
        idx = W.element_index(kept).ravel()
        assert len(np.unique(idx)) == idx.size
        self.inside = np.zeros(dest.parent.size, dtype=bool)
        self.inside[idx] = True
        assert result.dtype == dest.dtype and result.size == idx.size, (self.name, result.dtype, dest.dtype, result.shape)
        self.expected = self.before.copy()
        self.expected[idx] = result.ravel()
        self.inputs_before = {a.parent.ctypes.data: a.parent.copy() for a in arrays[1:]}
        self.types = tuple(np.dtype(a.dtype) for a in arrays)

    def plan(self, arrays=None):
        return S.make_plan(self.f, self.op, self.initop, self.dims, arrays or self.arrays)


def _pads(N, k):
    """(lo, hi) per dim: never all zero, odd in dim 0 for every other operand (the view starts inside a vector)"""
    lo = [(1 + k) % 3 if i else 1 + 2 * (k % 2) for i in range(N)]
    hi = [(2 + k + i) % 3 for i in range(N)]
    hi[0] = max(hi[0], 1)
    return lo, hi


def build(spec):
    """The row of a spec (see `table`)."""
    rng = np.random.default_rng([W.SEED_OFFSET, spec["seed"]])
    dims, tree, types, d = tuple(spec["dims"]), spec["tree"], [np.dtype(t) for t in spec["types"]], np.dtype(spec["dest"])
    N = len(dims)
    rdims, op, initop = tuple(spec.get("rdims", ())), spec.get("op"), spec.get("initop")
    n = int(np.prod(dims))
    perms = spec.get("perms") or [tuple(range(N))] * len(types)
    steps = spec.get("steps") or [None] * len(types)
    # data
    if "data" in spec:
        datas = spec["data"](rng, n)
    elif op == "+":
        assert tree == IDENT
        room = 8 if initop != "zero" else 0
        re = exact_sum_data(dims, rdims, types[0], d, room)
        if is_cx(types[0]):
            im = np.roll(re, 5) if is_cx(d) else np.where(np.arange(n).reshape(dims) % 2 == 0, 0.0, -0.0)
            v = np.empty(dims, types[0])
            v.real, v.imag = re, im
        else:
            v = re.astype(types[0])
        datas = [v.ravel()]
    elif op == "*":
        assert tree == IDENT
        datas = [exact_prod_data(dims, rdims, types[0], d).astype(types[0]).ravel()]
    else:
        assert tree == IDENT
        datas = [conversion_data(rng, n, types[0], d)]
        if op in ("min", "max") and is_float(types[0]) and rdims and len(rdims) < N and not is_int(d):
            pass   # (NaN lands in some outputs only: the value set holds one NaN, spread over many outputs)
        elif op in ("min", "max") and is_float(types[0]) and not is_int(d):
            x = datas[0]
            x[np.isnan(x)] = types[0].type(-3.0)   # one output: a NaN would be all the result says
    ins = []
    for k, (t, dat) in enumerate(zip(types, datas)):
        lo, hi = _pads(N, k + 1)
        ins.append(new_input(dims, perms[k], lo, hi, t, np.asarray(dat).astype(t), steps[k]))
    vals = evaluate(tree, [a.toarray() for a in ins])
    vals = np.broadcast_to(vals, dims)
    lo, hi = _pads(N, 0)
    dperm = spec.get("dperm") or tuple(range(N))
    if op is None:
        out = new_dest(rng, dims, dperm, lo, hi, d, spec.get("dsteps"))
        result = convert(vals, d)
    else:
        kshape = tuple(1 if i in rdims else m for i, m in enumerate(dims))
        nk = int(np.prod(kshape))
        if initop == "zero":
            old, oldv = None, np.zeros(kshape, d)
        else:
            if op == "*":
                o = np.where(pattern(nk, 5, 1, 2, 0) == 0, 1, -1) if d.kind not in "bu" and types[0].kind not in "bu" else np.ones(nk, np.int64)
            elif op == "+":
                o = pattern(nk, 5, 1, 3, 0) if d != B else np.zeros(nk, np.int64)   # 0, 1, 2: in range of every type, scaled by at most 3
                if initop is not None and d.kind in "bu":
                    assert initop[1] >= 0
            else:
                o = pattern(nk, 5, 1, 2, 0) if d.kind in "bu" else pattern(nk, 5, 1, 7, 3)
            oldv = o.astype(np.int64).astype(d).reshape(kshape)
            old = oldv.ravel()
        out = new_dest(rng, dims, dperm, [l if i not in rdims else 0 for i, l in enumerate(lo)], [h if i not in rdims else 0 for i, h in enumerate(hi)],
                       d, spec.get("dsteps"), bcast=rdims, old=old)
        result = reduce_model(op, initop, np.asarray(vals), oldv, rdims, d)
    return Row(spec, [out] + ins, np.asarray(result))


# ---- the table --------------------------------------------------------------------------------------------------------------------------
REFUSED_INPUTS = (I64, U64)   # 64-bit integer inputs of a float class are refused (Float64 does not hold them)


def admitted_pairs():
    """(source, destination) pairs the converting path takes: one of the two is a float type, the types differ, and no 64-bit integer is
    read into a float class"""
    out = []
    for s in INTS + FLOATS:
        for d in INTS + FLOATS:
            if s == d or (is_int(s) and is_int(d)) or (s in REFUSED_INPUTS):
                continue
            out.append((s, d))
    return out


def _pair_name(s, d):
    return "%s<-%s" % (NAMES[d], NAMES[s])


def _spec(specs, **kw):
    kw.setdefault("tree", IDENT)
    kw["seed"] = len(specs)
    kw["name"] = "%s/%s/%s<-%s%s" % (kw["cell"], show(kw["tree"]), NAMES[np.dtype(kw["dest"])], ",".join(NAMES[np.dtype(t)] for t in kw["types"]),
                                   ("/%s%s" % (kw["op"], "" if kw.get("initop") is None else "/" + str(kw["initop"]))) if kw.get("op") else "")
    kw["name"] += "/%s" % "x".join(map(str, kw["dims"]))
    specs.append(kw)


def _reduce_op(s, d, k):
    """pure conversions in a reduction: max / min on the full value sets; + (exact data) where a complex type has no order"""
    if is_cx(s) or is_cx(d):
        return "+", ("zero", None)[k % 2]
    return ("max", "min")[k % 2], None


# mixed arithmetic: (tree, operand types, destinations, data, runtime-compiled too)
def _d_f32_i32(rng, n):
    i = conversion_data(rng, n, I32, F32)
    a = (rng.integers(-40, 41, size=n) / 8.0).astype(np.float32)
    a[i == 16777217] = 1.0            # Float32[1] .+ Int32[16777217]
    a[i == -16777217] = -1.0
    return [a, i]


def _d_f32_u32(rng, n):
    return [(rng.integers(-40, 41, size=n) / 8.0).astype(np.float32), conversion_data(rng, n, U32, F32)]


def _d_f32_i32_nz(rng, n):
    a, i = _d_f32_i32(rng, n)
    i[i == 0] = 3
    a[a == 0] = 0.375
    return [a, i]


def _d_f32_ints(rng, n):              # integer-valued, small: a32 + 16777217 into an Int32 is defined
    return [rng.integers(-9, 10, size=n).astype(np.float32)]


def _d_c32_i32(rng, n):
    z = np.empty(n, C32)
    z.real = rng.integers(1, 41, size=n) / 8.0 * rng.choice([-1, 1], size=n)
    z.imag = rng.integers(1, 41, size=n) / 16.0 * rng.choice([-1, 1], size=n)
    i = conversion_data(rng, n, I32, F32)
    i[i == 0] = 5                     # (a zero factor or part would make the sign of a zero part depend on how the product is formed)
    return [z, i]


def _d_f32_c32(rng, n):
    z = _d_c32_i32(rng, n)[0]
    return [(rng.integers(-40, 41, size=n) / 8.0).astype(np.float32), z]


def _d_f64_u8(rng, n):
    with np.errstate(over="ignore"):
        x = conversion_data(rng, n, F64, F32)
    x[~np.isfinite(x)] = 0.1
    return [x, conversion_data(rng, n, U8, F64)]


def _d_f32_mask(rng, n):
    return [rng.standard_normal(n).astype(np.float32), rng.integers(0, 2, size=n).astype(B)]


def _d_i32_i16(rng, n):
    j = conversion_data(rng, n, I16, F64)
    j[j == 0] = 7
    return [conversion_data(rng, n, I32, F64), j]


def _d_i16_f32(rng, n):
    return [np.abs(conversion_data(rng, n, I16, F64).astype(np.int32)).clip(0, 32767).astype(I16), rng.standard_normal(n).astype(np.float32)]


def _d_cmp(rng, n):
    a, i = _d_f32_i32(rng, n)
    a[::2] = i[::2].astype(np.float32)   # Float32(i): equal to i, or next to it where Float32 does not hold i
    return [a, i]


def _d_i32_i32_f32(rng, n):
    return [rng.integers(-2 ** 30, 2 ** 30, size=n).astype(I32), rng.integers(-2 ** 30, 2 ** 30, size=n).astype(I32),
            (rng.integers(-40, 41, size=n) / 8.0).astype(np.float32)]


def _d_i8_u8(rng, n):
    return [conversion_data(rng, n, I8, I8), conversion_data(rng, n, U8, U8)]


def _d_i32_u32(rng, n):
    return [conversion_data(rng, n, I32, I32), conversion_data(rng, n, U32, U32)]


BIG = 16777217
EXPRESSIONS = [
    # name, tree, operand types, destination types, data, compiled at runtime too
    ("a32+i32", ("add", A(0), A(1)), (F32, I32), (F32, F64), _d_f32_i32, True),
    ("a32*u32", ("mul", A(0), A(1)), (F32, U32), (F32, F64), _d_f32_u32, True),
    ("a32/i32", ("div", A(0), A(1)), (F32, I32), (F32,), _d_f32_i32_nz, True),
    ("a32+16777217", ("add", A(0), L(BIG)), (F32,), (F64, I32), _d_f32_ints, True),
    ("c32*i32", ("mul", A(0), A(1)), (C32, I32), (C32, C64), _d_c32_i32, True),
    ("a32+c32", ("add", A(0), A(1)), (F32, C32), (C32, C64), _d_f32_c32, True),
    ("a64+u8", ("add", A(0), A(1)), (F64, U8), (F64, F32), _d_f64_u8, False),
    ("a32*mask", ("mul", A(0), A(1)), (F32, B), (F32,), _d_f32_mask, False),
    ("i32/i16", ("div", A(0), A(1)), (I32, I16), (F64, F32), _d_i32_i16, False),
    ("sqrt(i16)*a32", ("mul", ("sqrt", A(0)), A(1)), (I16, F32), (F64, F32), _d_i16_f32, True),
    ("max(a32,i32)", ("max", A(0), A(1)), (F32, I32), (F32,), _d_f32_i32, True),
    ("a32<i32", ("lt", A(0), A(1)), (F32, I32), (B, U8), _d_cmp, True),
    # an integer-typed sub-expression (Int32 + Int32, kept below 2^31: the device adds in Float64 and does not wrap) as the argument of a
    # Float32 product: Julia converts the Int32 sum to Float32 before multiplying
    ("(i32+i32)*a32", ("mul", ("add", A(0), A(1)), A(2)), (I32, I32, F32), (F32,), _d_i32_i32_f32, False),
    # the all-integer class, where the typing of mixed signedness decides the destination: wrapping UInt8 / UInt32 sums
    ("i8+u8", ("add", A(0), A(1)), (I8, U8), (U8,), _d_i8_u8, False),
    ("i32+u32", ("add", A(0), A(1)), (I32, U32), (U32,), _d_i32_u32, False),
]
# typing only (no row): what E.result_dtype must say.  (Bool * Bool is not listed: Julia and the device's integer class give Bool, the host
# keeps its older rule and allocates an Int64 for it -- the values, 0 and 1, are the same.)
TYPING = [
    (("add", A(0), A(1)), (I64, U64)), (("div", A(0), A(1)), (F32, I64)), (("add", A(0), A(1)), (B, B)), (("sub", A(0), A(1)), (B, B)),
    (("mul", A(0), A(1)), (C32, I64)), (("add", A(0), A(1)), (I8, U16)), (("min", A(0), A(1)), (F32, I32)),
    (("max", A(0), A(1)), (I16, U16)), (("add", A(0), A(1)), (U8, I64)), (("mul", A(0), A(1)), (F32, F64)), (("add", A(0), A(1)), (C32, F64)),
    (("div", A(0), A(1)), (U8, U8)), (("add", A(0), L(1.5)), (F32,)), (("add", A(0), L(np.float32(1.5))), (F32,)), (("sqrt", A(0)), (U8,)),
    (("lt", A(0), A(1)), (F64, I8)),
]

# refusals: (tree, operand types, destination, reduction)
REFUSALS = [
    ("Float32<-Int64", IDENT, (I64,), F32, None),
    ("Float64<-UInt64", IDENT, (U64,), F64, None),
    ("ComplexF64<-Int64 sum", IDENT, (I64,), C64, "+"),
    ("UInt64 under an order test", ("lt", A(0), A(1)), (U64, U64), B, None),
    ("maximum of UInt64", IDENT, (U64,), U64, "max"),
]

CELL_SHAPES = {
    "stream0": [(4099,), (1500, 3)],
    "stream1": [(100, 40)],
    "stream2": [(257, 4096)],
    "stream2c": [(130, 2048)],
    "tiled": [(33, 35), (70, 50)],
    "tiled3": [(5, 7, 9)],
    "all:epilogue": [(64, 48)],
    "all:second-launch": [(300017,)],
    "row:split1": [(100, 90)],
    "row:in-launch": [(20000, 4)],
    "col:in-launch": [(100, 90)],
    "col:second-launch": [(16, 5000)],
    "accumulate": [(70, 50)],
}
REDUCTION_CELLS = ("all:epilogue", "all:second-launch", "row:split1", "row:in-launch", "col:in-launch", "col:second-launch", "accumulate")
# two float and two integer destinations for every cell that is not covered pair by pair
CELL_PAIRS = [(I32, F32), (U8, F64), (F64, I16), (F32, U64), (F64, F32), (U16, C32), (F64, I64)]


def _rdims(cell, dims):
    if cell.startswith("all"):
        return tuple(range(len(dims)))
    if cell.startswith("row"):
        return (0,)
    if cell.startswith("col"):
        return (1,)
    return ()


def table():
    """The specs of every row (cheap: a row's arrays are made by build(spec))."""
    specs = []
    pairs = admitted_pairs()
    # every admitted pair once in STREAM, once in TILED and once in a reduction epilogue
    for k, (s, d) in enumerate(pairs):
        _spec(specs, cell="stream1", dims=(100, 40), types=(s,), dest=d, jit=True, pair=True)
        _spec(specs, cell="tiled", dims=(33, 35), types=(s,), dest=d, perms=[(1, 0)], jit=True, pair=True)
        op, initop = _reduce_op(s, d, k)
        # (a step of 2 along dim 0: the padded box neither fuses into one run nor runs along dim 0, REDUCE_ALL walks it by index decomposition)
        _spec(specs, cell="all:epilogue", dims=(64, 48), types=(s,), dest=d, op=op, initop=initop, rdims=(0, 1), steps=[[2, 1]], jit=True, pair=True)
    # the other cells
    for s, d in CELL_PAIRS:
        _spec(specs, cell="stream0", dims=(4099,), types=(s,), dest=d)
        _spec(specs, cell="stream0", dims=(1500, 3), types=(s,), dest=d)
        _spec(specs, cell="tiled", dims=(70, 50), types=(s,), dest=d, perms=[(1, 0)])
        _spec(specs, cell="tiled3", dims=(5, 7, 9), types=(s,), dest=d, perms=[(2, 1, 0)])
        _spec(specs, cell="generic", dims=(7, 9, 5, 3), types=(s,), dest=d, perms=[(2, 0, 3, 1)], steps=[[2, 3, 2, 3]], dperm=(1, 3, 0, 2), dsteps=[2, 2, 3, 2])
    for s, d in ((I16, F32), (F32, F64), (F64, I32), (F64, U8)):
        _spec(specs, cell="stream2", dims=(257, 4096), types=(s,), dest=d)
    for s, d in ((C32, C64), (F64, C64), (C64, I32), (C64, U16)):
        _spec(specs, cell="stream2c", dims=(130, 2048), types=(s,), dest=d)
    # TILED: three operands of three different types
    _spec(specs, cell="tiled", dims=(70, 50), tree=("add", ("mul", A(0), A(1)), A(2)), types=(F32, I16, F64), dest=F32, perms=[(1, 0), (0, 1), (1, 0)],
          data=lambda rng, n: [(rng.integers(-40, 41, size=n) / 8.0).astype(np.float32), conversion_data(rng, n, I16, F64), rng.standard_normal(n)], jit=True)
    _spec(specs, cell="tiled", dims=(70, 50), tree=("add", ("mul", A(0), A(1)), A(2)), types=(F32, I16, F64), dest=I32, perms=[(1, 0), (0, 1), (1, 0)],
          data=lambda rng, n: [rng.integers(-40, 41, size=n).astype(np.float32), conversion_data(rng, n, I16, F64), rng.integers(-1000, 1000, size=n).astype(np.float64)])
    # reductions: every cell with + on exact data and with max / min on the value sets
    for cell in REDUCTION_CELLS:
        if cell == "all:epilogue":
            continue   # (covered pair by pair above)
        for k, (s, d) in enumerate(CELL_PAIRS):
            dims = CELL_SHAPES[cell][0]
            if cell == "row:in-launch" and (is_cx(s) or is_cx(d)):
                dims = (9000, 4)   # (the ComplexF64 class cuts rows of 20000 nine ways and folds them in a second launch)
            rd = _rdims(cell, dims)
            big = int(np.prod(dims)) > 100000
            if cell == "accumulate":
                for initop in (None, ("scale", 2)):
                    _spec(specs, cell=cell, dims=dims, types=(s,), dest=d, op="+", initop=initop, rdims=rd, perms=[(1, 0)], jit=(k == 0))
                if not (is_cx(s) or is_cx(d)):
                    _spec(specs, cell=cell, dims=dims, types=(s,), dest=d, op=("max", "min")[k % 2], initop=None, rdims=rd, perms=[(1, 0)])
                continue
            if not (is_cx(s) or is_cx(d)):
                _spec(specs, cell=cell, dims=dims, types=(s,), dest=d, op=("max", "min")[k % 2], initop=None, rdims=rd, jit=(k == 0))
            if not big or k % 2 == 0 or is_cx(d):
                _spec(specs, cell=cell, dims=dims, types=(s,), dest=d, op="+", initop=("zero", None, ("scale", 3))[k % 3], rdims=rd)
    # products (exact data: signs and a few factors of 2), accumulated into an old destination as it is and scaled
    for cell, dims in (("all:epilogue", (64, 48)), ("row:split1", (100, 90)), ("col:in-launch", (100, 90)), ("accumulate", (70, 50))):
        for k, (s, d) in enumerate(CELL_PAIRS):
            if not (is_cx(s) or is_cx(d)):
                _spec(specs, cell=cell, dims=dims, types=(s,), dest=d, op="*", initop=(None, ("scale", 2))[k % 2], rdims=_rdims(cell, dims),
                      steps=[[2, 1]] if cell == "all:epilogue" else None, perms=[(1, 0)] if cell == "accumulate" else None)
    # mixed arithmetic, in STREAM (short rows) and in TILED
    for name, tree, types, dests, data, jit in EXPRESSIONS:
        for d in dests:
            _spec(specs, cell="stream1", dims=(100, 40), tree=tree, types=types, dest=d, data=data, jit=jit, expression=name)
        _spec(specs, cell="tiled", dims=(33, 35), tree=tree, types=types, dest=dests[0], data=data, perms=[(1, 0)] + [(0, 1)] * (len(types) - 1), expression=name)
    return specs


TABLE = table()


def group_table():
    """Two grouped launches of Int16 -> Float32 conversions: members the linear body of smr_k_group.hip takes (inputs laid out like their
    destinations) and members its tiled body takes (transposed inputs)."""
    out = {"group:linear": [], "group:tiled": []}
    for dims in ((40, 30), (17,), (9, 8, 7), (100, 3)):
        _spec(out["group:linear"], cell="group:linear", dims=dims, types=(I16,), dest=F32)
    for dims in ((33, 35), (40, 24), (70, 50)):
        _spec(out["group:tiled"], cell="group:tiled", dims=dims, types=(I16,), dest=F32, perms=[(1, 0)])
    for cell, specs in out.items():
        for k, sp in enumerate(specs):
            sp["seed"] = 100000 + 10 * len(cell) + k
    return out


GROUP_TABLE = group_table()


def group_rows(cell):
    return [build(s) for s in GROUP_TABLE[cell]]


def build_group(members, arrays=None):
    """The group of the member rows, on their host views or on `arrays` (one tuple of views per member)."""
    built = [S.build_problem(r.f, None, None, r.dims, arrays[k] if arrays else r.arrays, stream=0) for k, r in enumerate(members)]
    return S._lib.Group([b[0] for b in built], keepalive=built)


def cells():
    return sorted({s["cell"] for s in TABLE})


def rows(cell):
    for s in TABLE:
        if s["cell"] == cell:
            yield build(s)


# ---- what describe() says ---------------------------------------------------------------------------------------------------------------
def stream_form(desc, types):
    """The STREAM kernel form (build_stream_args, smr_k_stream.hip) from describe()'s canonical dims and compute class: a converting call
    moves one element per access (V = 1) with U = 8 accesses in flight per lane (2 in the ComplexF64 class: 16-byte elements)."""
    assert "(mixed)" in desc and W.token(desc, "vec") == "1" and S.get_option("stream_pack_rows") == 1, desc   # what the rule below assumes
    ct = W.token(desc, "ct").split("(")[0]
    U = 2 if ct == "c64" else 8
    dims = [int(v) for v in W.token(desc, "dims").split("x")]
    n0 = dims[0]
    if len(dims) >= 2 and n0 <= 128:
        return 1
    if len(dims) >= 2 and n0 <= 128 * U:
        ncc = (n0 + 255) // 256
        if ncc <= 2 and int(np.prod(dims[1:])) // (U // ncc) >= 1024:
            return 2
    return 0


def reached(desc, types):
    """the cell a plan belongs to"""
    fam = W.family(desc)
    if fam == "stream":
        f = stream_form(desc, types)
        return "stream%d" % f
    if fam == "tiled":
        return "tiled"
    if fam == "reduce_all":
        return "all:" + W.token(desc, "fold")
    if fam == "reduce_part":
        form, fold, split = W.token(desc, "form"), W.token(desc, "fold"), int(W.token(desc, "split") or 1)
        if form == "general":
            return "accumulate"
        return "%s:%s" % (form, "split1" if split == 1 else fold)
    return fam
