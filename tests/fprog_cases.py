"""The conformance table of the f-program's arithmetic: one row per opcode (or literal form of one), with the Python lambda that
makes the front end emit it, the types it exists for, how its result is judged and which execution paths can run it.  No torch, no
mpmath: tests/golden/make_fprog_golden.py (mpmath) writes the exact expected values of the inexact rows into
tests/golden/fprog_golden.npz, tests/test_fprog_golden_host.py checks the fixture, the CPU references and the checkers without a
device, tests/test_gpu_fprog_conformance.py runs every (row, type) on the GPU.

Classes
  exact     correctly rounded or exact by definition: bit for bit against `ref` (NumPy in the row's own type, Julia's rules where
            they differ from C's: JL_* below); NaN payloads are not compared, the sign of zero is.
  faithful  library functions: the fixture brackets the exact result between two neighbouring values of the type (`lo`, `hi`); the
            result must be one of them (a neighbour of `lo` when `lo` is exact): DESIGN section 3's "<= 1 ulp".
  complex   |got - exact| <= (E_ref + L) * eps * |exact|, E_ref the measured error of the CPU reference on the same points (at most
            2), L the rounded real operations on the longest path of the device's formula (csrc/smr_device.h), counted beside
            each row.  The same bound holds on the row's edge points (finite inputs at the ends of the range).
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np

import strided_jl_amd as S

fn = S.fn
F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
TYPES = {"f32": F32, "f64": F64, "c64": C64, "c128": C128, "i8": np.int8, "u8": np.uint8, "i16": np.int16, "u16": np.uint16,
         "i32": np.int32, "u32": np.uint32, "i64": np.int64}
REAL, CPLX = ("f32", "f64"), ("c64", "c128")
INTERP, JIT, BOTH = ("interp",), ("jit",), ("interp", "jit")
FIXTURE_CAP = 157393  # bytes: the largest fixture committed before this one (strided_golden.npz)
NMAX = 131            # operand length: whole 16-byte vectors and a ragged tail in STREAM

# name: unique; f: the lambda; arity; types; cls; paths; ref: NumPy reference (Float64 / complex128 arguments for the inexact classes,
# the row's own type for exact rows) or "oracle" (the CPU oracle's std::complex, base opcodes); L and region: complex rows only
# alt: the same value, bit for bit, written so that the planner does NOT hand it to a precompiled functor (rows it does: add, mul, abs2)
Row = namedtuple("Row", "name f arity types cls paths ref L region out alt", defaults=(None, 0, "", None, None))


def real_of(tn):
    return F32 if tn in ("f32", "c64") else F64


# ---- Julia's rules where NumPy's differ (Base/math.jl, Base/float.jl); hand-checked rows in JULIA_AUTHORITY ----------------------
def jl_min(a, b):
    r = np.where(b < a, b, np.where(a < b, a, np.where(np.signbit(a), a, b)))
    return np.where(np.isnan(a), a, np.where(np.isnan(b), b, r))


def jl_max(a, b):
    r = np.where(a < b, b, np.where(b < a, a, np.where(np.signbit(a), b, a)))
    return np.where(np.isnan(a), a, np.where(np.isnan(b), b, r))


def jl_sign(a):
    return np.where((a == 0) | np.isnan(a), a, np.copysign(np.ones_like(a), a))


def jl_mod(a, b):
    """mod(x::T, y::T) where T<:AbstractFloat (Base/float.jl): rem, then the sign of y"""
    with np.errstate(all="ignore"):
        r = np.fmod(a, b)
        return np.where(r == 0, np.copysign(r, b), np.where((r > 0) != (b > 0), r + b, r))


def jl_rem(a, b):
    with np.errstate(all="ignore"):
        return np.fmod(a, b)


def _f64(g):
    def h(*a):
        with np.errstate(all="ignore"):
            return g(*a)
    return h


def jl_pow(a, b):
    with np.errstate(all="ignore"):
        return np.power(a, b)


def jl_hypot(a, b):
    with np.errstate(all="ignore"):
        return np.hypot(a, b)


# (row, arguments, result): what Julia's Base returns, written by hand; the generator and the host test assert the references on them
NAN, INF = float("nan"), float("inf")
JULIA_AUTHORITY = [
    ("min", (NAN, 1.0), NAN), ("min", (1.0, NAN), NAN), ("max", (NAN, 1.0), NAN), ("max", (1.0, NAN), NAN),
    ("min", (-0.0, 0.0), -0.0), ("min", (0.0, -0.0), -0.0), ("max", (-0.0, 0.0), 0.0), ("max", (0.0, -0.0), 0.0),
    ("sign", (0.0,), 0.0), ("sign", (-0.0,), -0.0), ("sign", (NAN,), NAN), ("sign", (-3.5,), -1.0),
    ("round", (0.5,), 0.0), ("round", (1.5,), 2.0), ("round", (2.5,), 2.0), ("round", (-0.5,), -0.0), ("round", (-2.5,), -2.0),
    ("mod", (-0.0, 3.0), 0.0), ("mod", (0.0, -3.0), -0.0), ("mod", (5.0, INF), 5.0), ("mod", (-5.0, INF), INF), ("mod", (5.0, -INF), -INF),
    ("mod", (-5.0, -INF), -5.0), ("mod", (5.0, 0.0), NAN), ("mod", (-7.0, 3.0), 2.0), ("mod", (7.0, -3.0), -2.0),
    ("rem", (-7.0, 3.0), -1.0), ("rem", (5.0, INF), 5.0), ("rem", (5.0, 0.0), NAN), ("rem", (-6.0, 3.0), -0.0),
    ("pow", (0.0, 0.0), 1.0), ("pow", (NAN, 0.0), 1.0), ("pow", (1.0, NAN), 1.0), ("pow", (-8.0, 1.0 / 3.0), NAN),
    ("pow", (-2.0, 3.0), -8.0), ("pow", (-0.0, -1.0), -INF), ("pow", (0.0, -2.0), INF),
    ("hypot", (INF, NAN), INF), ("hypot", (NAN, -INF), INF), ("hypot", (NAN, 1.0), NAN),
]


def same_value(got, want):
    """elementwise: equal bits up to NaN payloads (NaN == NaN, -0.0 != 0.0); complex: both parts"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "c":
        return same_value(got.real, want.real) & same_value(got.imag, want.imag)
    if got.dtype.kind != "f":
        return got == want
    return ((got == want) & (np.signbit(got) == np.signbit(want))) | (np.isnan(got) & np.isnan(want))


# ---- the faithful bracket ------------------------------------------------------------------------------------------------------
def hi_of(lo, exact):
    lo = np.asarray(lo)
    with np.errstate(over="ignore"):  # the neighbour above floatmax is Inf
        return np.where(exact, lo, np.nextafter(lo, lo.dtype.type(np.inf)))


def _ordinal(x):
    """the position of a float among the values of its type (monotone; -0.0 and +0.0 are one step apart)"""
    x = np.asarray(x)
    it = np.int32 if x.dtype == F32 else np.int64
    b = x.view(it).astype(np.int64)
    return np.where(b < 0, np.int64(-1) - (b & np.int64(np.iinfo(it).max)), b)


def steps_outside(got, lo, exact):
    """Steps of the type by which `got` misses the faithful bracket: 0 inside [lo, hi] (one more step either way when lo is exact).
    A NaN, or a zero of the wrong sign where the bracket ends at a zero, counts as outside (returns a large number)."""
    got, lo, exact = np.asarray(got), np.asarray(lo), np.asarray(exact, dtype=bool)
    assert got.dtype == lo.dtype
    hi = hi_of(lo, exact).astype(lo.dtype)
    g, a, b = _ordinal(got), _ordinal(lo) - exact, _ordinal(hi) + exact
    out = np.where(g < a, a - g, np.where(g > b, g - b, 0)).astype(np.int64)
    # an exact zero or infinity is asked for as it is (the zero with its sign)
    fixed = exact & ((lo == 0) | np.isinf(lo))
    out = np.where(fixed, np.where((got == lo) & (np.signbit(got) == np.signbit(lo)), 0, 1 << 40), out)
    return np.where(np.isnan(got), 1 << 40, out)


def special_ok(got, want):
    return same_value(got, want)


# ---- the complex measure -------------------------------------------------------------------------------------------------------
def cx_error(got, ex_hi, ex_lo, tn):
    """|got - exact| / (eps(real type) * |exact|) per point; exact = ex_hi + ex_lo (the nearest value of the type + the rest); a part
    that overflows the type asks for that infinity and for finite other parts (error 0 or inf); around zero the unit is the least subnormal"""
    R = real_of(tn)
    eps = float(np.finfo(R).eps)
    g = np.asarray(got).astype(C128)
    with np.errstate(all="ignore"):
        dre = (g.real - ex_hi.real) - ex_lo.real
        dim = (g.imag - ex_hi.imag) - ex_lo.imag
        # scaled against overflow / underflow of the norms
        sc = np.maximum(np.abs(ex_hi.real), np.abs(ex_hi.imag))
        sc = np.where((sc == 0) | ~np.isfinite(sc), 1.0, sc)
        num = np.hypot(dre / sc, dim / sc)
        den = np.hypot(ex_hi.real / sc, ex_hi.imag / sc)
        # below the least normal value the spacing of the type stops shrinking: an ulp is never less than the least subnormal
        err = num / np.maximum(eps * den, float(np.finfo(R).smallest_subnormal) / sc)
    inf_c = np.isinf(ex_hi.real) | np.isinf(ex_hi.imag)
    ok_inf = same_value(g.real, ex_hi.real) | ~np.isinf(ex_hi.real)
    ok_inf &= same_value(g.imag, ex_hi.imag) | ~np.isinf(ex_hi.imag)
    ok_inf &= np.isfinite(g.real) | np.isinf(ex_hi.real)
    ok_inf &= np.isfinite(g.imag) | np.isinf(ex_hi.imag)
    err = np.where(inf_c, np.where(ok_inf, 0.0, np.inf), err)
    return np.where(np.isnan(err), np.inf, err)


def axis_ok(got, ex_hi, ex_lo, sign_re, sign_im, bound, tn):
    """Real-axis points (imaginary part +-0), each component on its own: within `bound` ulp of its exact value, and where that value
    is zero, the zero of the stored sign.  Returns a boolean per point."""
    got = np.asarray(got).astype(C128)
    eps = float(np.finfo(real_of(tn)).eps)
    ok = np.ones(got.shape, dtype=bool)
    for g, h, l, sg in ((got.real, ex_hi.real, ex_lo.real, sign_re), (got.imag, ex_hi.imag, ex_lo.imag, sign_im)):
        with np.errstate(all="ignore"):
            near = np.abs((g - h) - l) <= bound * eps * np.abs(h)
        near = np.where(np.isinf(h), g == h, near)
        ok &= np.where(h == 0, (g == 0) & (np.signbit(g) == sg), near)
    return ok


# ---- the references ------------------------------------------------------------------------------------------------------------
def _cpow(n):
    return lambda z: np.power(z, n)


def _csign(z):
    """z / |z| of z scaled by a power of two to a larger part in [1, 2): |z| neither overflows nor falls among the subnormals"""
    with np.errstate(all="ignore"):
        _, e = np.frexp(np.maximum(np.abs(z.real), np.abs(z.imag)))
        w = np.ldexp(z.real, 1 - e) + 1j * np.ldexp(z.imag, 1 - e)
        return np.where(z == 0, z, w / np.abs(w))


def _cexp2(z):
    """2^re * cis(im * log(2)) with the real exp2: NumPy's complex exp2 goes through z * log(2) and loses |re| ulp"""
    with np.errstate(all="ignore"):
        e, th = np.exp2(z.real), z.imag * np.log(2.0)
        out = np.empty(z.shape, dtype=C128)
        out.real, out.imag = np.where(z.imag == 0, e, e * np.cos(th)), np.where(z.imag == 0, z.imag, e * np.sin(th))
        return out


def _powi_exact(n):
    def g(a):  # the correctly rounded power, from the rationals (n in -2..3: the device's products are exact in this test's inputs)
        return a ** n
    return g


ROWS = []


def _add(*a, **k):
    ROWS.append(Row(*a, **k))


# exact, float: base opcodes run interpreted and runtime-compiled, the math opcodes runtime-compiled only
_add("add", lambda a, b: a + b, 2, REAL, "exact", BOTH, lambda a, b: a + b, alt=lambda a, b: b + a)
_add("sub", lambda a, b: a - b, 2, REAL, "exact", BOTH, lambda a, b: a - b)
_add("mul", lambda a, b: a * b, 2, REAL, "exact", BOTH, lambda a, b: a * b, alt=lambda a, b: b * a)
_add("div", lambda a, b: a / b, 2, REAL, "exact", BOTH, lambda a, b: a / b)
_add("sqrt", fn.sqrt, 1, REAL, "exact", BOTH, np.sqrt)
_add("inv", fn.inv, 1, REAL, "exact", BOTH, lambda a: a.dtype.type(1) / a)
_add("neg", lambda a: -a, 1, REAL, "exact", BOTH, lambda a: -a)
_add("abs", fn.abs, 1, REAL, "exact", BOTH, np.abs)
_add("abs2", fn.abs2, 1, REAL, "exact", BOTH, lambda a: a * a, alt=lambda a: fn.abs2(fn.conj(a)))
_add("min", fn.min, 2, REAL, "exact", BOTH, jl_min)
_add("max", fn.max, 2, REAL, "exact", BOTH, jl_max)
for _n, _g in (("lt", np.less), ("le", np.less_equal), ("gt", np.greater), ("ge", np.greater_equal), ("eq", np.equal),
               ("ne", np.not_equal)):
    _add(_n, getattr(fn, _n), 2, REAL, "exact", BOTH, _g, out=np.bool_)
_add("floor", fn.floor, 1, REAL, "exact", JIT, np.floor)
_add("ceil", fn.ceil, 1, REAL, "exact", JIT, np.ceil)
_add("trunc", fn.trunc, 1, REAL, "exact", JIT, np.trunc)
_add("round", fn.round, 1, REAL, "exact", JIT, np.rint)
_add("sign", fn.sign, 1, REAL, "exact", JIT, jl_sign)
_add("rem", fn.rem, 2, REAL, "exact", JIT, jl_rem)
_add("mod", fn.mod, 2, REAL, "exact", JIT, jl_mod)
_add("fma", fn.fma, 3, REAL, "exact", JIT, "fraction")

# faithful: library functions in both real types
for _n, _g in (("exp", np.exp), ("log", np.log), ("sin", np.sin), ("cos", np.cos), ("tanh", np.tanh)):
    _add(_n, getattr(fn, _n), 1, REAL, "faithful", BOTH, _f64(_g))
for _n, _g in (("tan", np.tan), ("asin", np.arcsin), ("acos", np.arccos), ("atan", np.arctan), ("sinh", np.sinh), ("cosh", np.cosh),
               ("exp2", np.exp2), ("expm1", np.expm1), ("log2", np.log2), ("log10", np.log10), ("log1p", np.log1p), ("cbrt", np.cbrt)):
    _add(_n, getattr(fn, _n), 1, REAL, "faithful", JIT, _f64(_g))
_add("pow", lambda a, b: a ** b, 2, REAL, "faithful", JIT, jl_pow)
_add("atan2", lambda a, b: fn.atan(a, b), 2, REAL, "faithful", JIT, _f64(np.arctan2))
_add("hypot", fn.hypot, 2, REAL, "faithful", JIT, jl_hypot)
POWI_N = (5, 7, -3, 17, 127, -128)
for _n in POWI_N:
    _add("powi%d" % _n, (lambda n: lambda a: a ** n)(_n), 1, REAL, "faithful", JIT, (lambda n: _f64(lambda a: np.power(a, float(n))))(_n))

# complex: L counts the rounded real operations on the longest path from an input to an output component in csrc/smr_device.h
# (a library call, + - * / and sqrt count one each; exact scalings by powers of two, comparisons, copysign and negation count none)
_add("cabs", fn.abs, 1, CPLX, "complex", BOTH, "oracle", 1, "any finite z")  # L: hypot
_add("csqrt", fn.sqrt, 1, CPLX, "complex", BOTH, "oracle", 4, "any finite z")  # L: hypot + sqrt /
_add("cexp", fn.exp, 1, CPLX, "complex", BOTH, "oracle", 2, "|im| <= 2^20, away from zeros of sin / cos by 2^-6")  # L: exp | cos, *
_add("clog", fn.log, 1, CPLX, "complex", BOTH, "oracle", 4, "|z - 1| >= 0.25 (main points)")  # L: near 1: - * + log1p; elsewhere hypot log +
_add("csin", fn.sin, 1, CPLX, "complex", BOTH, "oracle", 2, "|re| <= 2^20, |im| <= 8, parts away from zeros by 2^-6")  # L: sin | cosh, *
_add("ccos", fn.cos, 1, CPLX, "complex", BOTH, "oracle", 2, "as sin")  # L: as sin
_add("ctanh", fn.tanh, 1, CPLX, "complex", BOTH, "oracle", 7, "away from i(pi/2 + k pi) by 0.1")  # L: sinh * + sqrt * * / (Base's form)
_add("cinv", fn.inv, 1, CPLX, "complex", BOTH, "oracle", 4, "any finite z != 0")  # L: Smith: / * + /
_add("cmul", lambda a, b: a * b, 2, CPLX, "complex", BOTH, "oracle", 2, "products within range", alt=lambda a, b: b * a)  # L: * -
_add("cdiv", lambda a, b: a / b, 2, CPLX, "complex", BOTH, "oracle", 4, "quotients within range; a numerator at floatmax only over a divisor of like size (libgcc's division overflows otherwise)")  # L: Smith: / * + /
_add("csinh", fn.sinh, 1, CPLX, "complex", JIT, _f64(np.sinh), 2, "as sin, parts exchanged")  # L: as sin
_add("ccosh", fn.cosh, 1, CPLX, "complex", JIT, _f64(np.cosh), 2, "as sin, parts exchanged")  # L: as sin
_add("cexp2", fn.exp2, 1, CPLX, "complex", JIT, _cexp2, 3, "|im| < 2 (th = im * log(2) is itself rounded), away from zeros by 2^-6")  # L: * cos *
_add("clog2", fn.log2, 1, CPLX, "complex", JIT, _f64(np.log2), 5, "|z - 1| >= 0.25")  # L: log, /
_add("clog10", fn.log10, 1, CPLX, "complex", JIT, _f64(np.log10), 5, "|z - 1| >= 0.25")  # L: log, /
_add("csign", fn.sign, 1, CPLX, "complex", JIT, _csign, 2, "any finite z != 0")  # L: hypot /
_add("cpowi5", lambda a: a ** 5, 1, CPLX, "complex", JIT, _f64(_cpow(5)), 6, "|z| in [2^-8, 2^8]")  # L: three products by squaring
_add("cpowi-3", lambda a: a ** -3, 1, CPLX, "complex", JIT, _f64(_cpow(-3)), 8, "|z| in [2^-8, 2^8]")  # L: the inverse and two products
_add("cfma", fn.fma, 3, CPLX, "complex", JIT, _f64(lambda a, b, c: a * b + c), 2, "|parts| in [2^-4, 2^4]")  # L: two fused steps

BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
BASE_UNARY = {"sqrt", "exp", "log", "sin", "cos", "tanh", "inv", "abs"}


def cases(cls=None):
    return [(r.name, tn) for r in ROWS for tn in r.types if cls is None or r.cls in cls]


# ---- integer class -------------------------------------------------------------------------------------------------------------
INTS = ("i8", "u8", "i16", "u16", "i32", "u32", "i64")


def int_edges(tn, n=NMAX, seed=7):
    """typemin, typemax, 0, +-1 and their neighbours, then random values of the type"""
    dt = np.dtype(TYPES[tn])
    info = np.iinfo(dt)
    edge = [info.min, info.max, 0, 1, 2, 3, 7, info.max - 1, info.min + 1]
    if info.min < 0:
        edge += [-1, -2, -3, -7]
    r = np.random.default_rng(seed + sum(map(ord, tn)))
    x = r.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    x[: len(edge)] = np.array(edge, dtype=np.int64 if info.min < 0 else np.uint64).astype(dt)
    return x


def _wrap(v, dt):
    """Python integers -> the wrapped values of dt"""
    dt = np.dtype(dt)
    bits = 8 * dt.itemsize
    m = 1 << bits
    out = [int(x) % m for x in v]
    if dt.kind == "i":
        out = [x - m if x >= m >> 1 else x for x in out]
    return np.array(out, dtype=dt)


def _trunc_rem(a, b):
    r = abs(a) % abs(b)
    return -r if a < 0 else r


# name -> (lambda, arity, python-integer reference over exact integers (wrapped into the type afterwards), paths, result kind)
INT_ROWS = {
    "add": (lambda a, b: a + b, 2, lambda a, b: a + b, BOTH, "same"),
    "sub": (lambda a, b: a - b, 2, lambda a, b: a - b, BOTH, "same"),
    "mul": (lambda a, b: a * b, 2, lambda a, b: a * b, BOTH, "same"),
    "neg": (lambda a: -a, 1, lambda a: -a, BOTH, "same"),
    "abs": (fn.abs, 1, lambda a: abs(a), BOTH, "same"),          # abs(typemin) wraps to typemin
    "abs2": (fn.abs2, 1, lambda a: a * a, BOTH, "same"),
    "min": (fn.min, 2, lambda a, b: min(a, b), BOTH, "same"),
    "max": (fn.max, 2, lambda a, b: max(a, b), BOTH, "same"),
    "lt": (fn.lt, 2, lambda a, b: a < b, BOTH, "bool"),
    "le": (fn.le, 2, lambda a, b: a <= b, BOTH, "bool"),
    "eq": (fn.eq, 2, lambda a, b: a == b, BOTH, "bool"),
    "ne": (fn.ne, 2, lambda a, b: a != b, BOTH, "bool"),
    "powi2": (lambda a: a ** 2, 1, lambda a: a ** 2, JIT, "same"),
    "powi5": (lambda a: a ** 5, 1, lambda a: a ** 5, JIT, "same"),
    "powi127": (lambda a: a ** 127, 1, lambda a: a ** 127, JIT, "same"),
    "mod7": (lambda a: a % 7, 1, lambda a: a % 7, JIT, "i64"),
    "mod-7": (lambda a: a % -7, 1, lambda a: a % -7, JIT, "i64"),
    "mod-1": (lambda a: a % -1, 1, lambda a: 0, JIT, "i64"),
    "rem7": (lambda a: fn.rem(a, 7), 1, lambda a: _trunc_rem(a, 7), JIT, "i64"),
    "rem-7": (lambda a: fn.rem(a, -7), 1, lambda a: _trunc_rem(a, -7), JIT, "i64"),
    "rem-1": (lambda a: fn.rem(a, -1), 1, lambda a: 0, JIT, "i64"),
    "and": (lambda a, b: a & b, 2, lambda a, b: a & b, JIT, "same"),
    "or": (lambda a, b: a | b, 2, lambda a, b: a | b, JIT, "same"),
    "xor": (lambda a, b: a ^ b, 2, lambda a, b: a ^ b, JIT, "same"),
    "not": (lambda a: ~a, 1, lambda a: ~a, JIT, "same"),
    "sign": (fn.sign, 1, lambda a: (a > 0) - (a < 0), JIT, "same"),
    "fma": (fn.fma, 3, lambda a, b, c: a * b + c, JIT, "same"),
}
INT_ALT = {"add": lambda a, b: b + a, "mul": lambda a, b: b * a, "abs2": lambda a: fn.abs2(fn.conj(a))}  # as Row.alt
# narrow operands stored into Int64: the value must have wrapped in the narrow type first (the planner's WRAP_* insertions)
INT_WIDE = ("add", "mul", "neg", "abs", "abs2", "powi5", "powi127", "fma", "not", "sub")


def int_cases():
    """(row, type, wide): every row on Int64 and on two narrow types, taken in turn so that every type meets every kind of row"""
    out = []
    for i, name in enumerate(INT_ROWS):
        narrow = [INTS[(2 * i) % 6], INTS[(2 * i + 3) % 6]]
        for tn in narrow + ["i64"]:
            out.append((name, tn, False))
        if name in INT_WIDE:
            out += [(name, tn, True) for tn in narrow]
    return out


def int_inputs(name, tn):
    ar = INT_ROWS[name][1]
    return [int_edges(tn, seed=11 + 5 * i) if i == 0 else np.roll(int_edges(tn, seed=11 + 5 * i), 5 * i) for i in range(ar)]


def int_expected(name, tn, wide, xs):
    """the row's result in Julia: computed in the operands' type (wrapping), then stored (into Int64 when wide)"""
    _, ar, ref, _, kind = INT_ROWS[name]
    vals = [ref(*[int(x[i]) for x in xs]) for i in range(len(xs[0]))]
    if kind == "bool":
        return np.array(vals, dtype=np.bool_)
    if kind == "i64":  # promote(IntN, Int64): the operation runs in Int64
        return _wrap(vals, np.int64) if tn != "u64" else None
    narrow = _wrap(vals, TYPES[tn])
    return narrow.astype(np.int64) if wide else narrow


# ---- exact float rows: inputs made at test time (no fixture) -------------------------------------------------------------------
CROSS = [0.0, -0.0, np.inf, -np.inf, np.nan, 3.0, -5.0, 1.0]  # binary exact rows: every one of these meets every other


def exact_inputs(name, tn):
    """The operands of an exact float row, made here from a fixed seed.  Unary and ternary rows: special values first, then random
    magnitudes over the whole range.  Binary rows: the 64 pairs of CROSS (zeros of either sign, infinities, NaN and finite values in
    every combination: min / max / comparisons of opposite zeros, zero and infinite divisors of either sign for rem / mod), then the
    argument pairs of JULIA_AUTHORITY for the row, then the other special values and random magnitudes."""
    R = TYPES[tn]
    fi = np.finfo(R)
    r = np.random.default_rng(1000 + sum(map(ord, name)) + (tn == "f64"))
    ar = BY_NAME[name].arity
    sp = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.0, -7.25, float(fi.max), -float(fi.max),
          float(fi.tiny), -float(fi.tiny), float(fi.smallest_subnormal), -float(fi.smallest_subnormal), float(fi.tiny) * 0.75,
          2.0 ** 23 + 1, 2.0 ** 52 + 1, -(2.0 ** 23) - 0.5, 4503599627370497.5]
    like = ("add", "sub", "rem", "mod", "fma", "min", "max", "floor", "ceil", "trunc", "round", "lt", "le", "gt", "ge", "eq", "ne")
    head = []  # per operand: the values every run must meet
    if ar == 2:
        pairs = [(x, y) for x in CROSS for y in CROSS] + [args for row, args, _ in JULIA_AUTHORITY if row == name]
        head = [[p[i] for p in pairs] + list(np.roll(sp[13:], 5 * i)) for i in range(2)]
    else:
        head = [list(np.roll(sp, 3 * i)) for i in range(ar)]
    k = len(head[0])
    assert k + 40 <= NMAX
    xs = []
    for i in range(ar):
        e = r.integers(fi.minexp - fi.nmant, fi.maxexp - 1, NMAX, endpoint=True)
        if name in like:
            e = np.where(r.random(NMAX) < 0.7, r.integers(-6, 6, NMAX), e)  # operands of like magnitude, where rounding happens
        with np.errstate(all="ignore"):
            x = (np.ldexp(r.uniform(1, 2, NMAX), e) * r.choice([-1.0, 1.0], NMAX)).astype(R)
            x[:k] = np.array(head[i], dtype=np.float64).astype(R)
        xs.append(x)
    t = k  # the targeted blocks follow the head
    if name in ("sqrt", "div", "inv"):  # subnormal operands and results
        xs[0][t:t + 10] = (np.ldexp(r.uniform(1, 2, 10), fi.minexp - r.integers(1, fi.nmant, 10))).astype(R)
        t += 10
    if name in ("eq", "ne", "le", "ge", "lt", "gt", "min", "max"):
        xs[1][t:t + 10] = xs[0][t:t + 10]
        t += 10
    if name == "fma":  # cancellation: a*b + c is the rounding error of the product, which only a fused operation keeps
        with np.errstate(all="ignore"):
            xs[2][t:t + 40] = -(xs[0][t:t + 40] * xs[1][t:t + 40])
    if name == "div":
        with np.errstate(all="ignore"):  # quotients that land among the subnormals
            xs[1][t:t + 15] = (np.ldexp(r.uniform(1, 2, 15), fi.maxexp - 3)).astype(R)
            q = (np.ldexp(r.uniform(1, 2, 15), r.integers(fi.minexp + 2, fi.minexp + fi.nmant, 15))).astype(R) * xs[1][t:t + 15]
            xs[0][t:t + 15] = np.where(np.isfinite(q), q, R(1))
    return xs


def round_fraction(q, dtype):
    """the correctly rounded (ties to even) value of the rational q in dtype; subnormal and overflowing results included"""
    fi = np.finfo(dtype)
    if q == 0:
        return dtype(0)
    s, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1
    e = max(e, fi.minexp)                       # subnormals share the least exponent
    ulp = Fraction(2) ** (e - fi.nmant)
    n = a / ulp
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2):
        k += 1
    v = k * ulp
    if v >= Fraction(2) ** fi.maxexp:
        return dtype(s * np.inf)
    return dtype(s * float(v))


def exact_expected(name, tn, xs):
    R = TYPES[tn]
    row = BY_NAME[name]
    if row.ref == "fraction":
        a, b, c = xs
        out = np.empty(len(a), dtype=R)
        for i in range(len(a)):
            v = [float(a[i]), float(b[i]), float(c[i])]
            if any(np.isnan(v)):
                out[i] = np.nan
            elif all(np.isfinite(v)):
                q = Fraction(v[0]) * Fraction(v[1]) + Fraction(v[2])
                if q == 0:  # IEEE: an exact zero product keeps its sign and (-0) + (-0) = -0; a cancelled sum is +0
                    out[i] = (a[i] * b[i]) + c[i] if (v[0] == 0 or v[1] == 0) else R(0)
                else:
                    out[i] = round_fraction(q, R)
            elif np.isfinite(v[0]) and np.isfinite(v[1]):
                out[i] = c[i]  # finite factors: their exact product is finite whatever its size, the infinite addend wins
            else:
                with np.errstate(all="ignore"):  # an infinite factor: Inf * 0 and Inf - Inf are NaN, as the type's own operations say
                    out[i] = (a[i] * b[i]) + c[i]
        return out
    with np.errstate(all="ignore"):
        out = np.asarray(row.ref(*xs))
    return out.astype(row.out or R)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def load_fixture(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def spacing_of(v):
    """the distance between neighbouring values of v's type at |v|, as Float64 (the least subnormal at zero, finite at floatmax, 0 at infinities)"""
    v = np.asarray(v)
    fi = np.finfo(v.dtype)
    a = np.abs(v.astype(F64))
    _, e = np.frexp(np.where(np.isfinite(a), a, 1.0))
    e = np.where(a == 0, fi.minexp, e - 1)
    return np.where(np.isfinite(a), np.ldexp(1.0, np.maximum(e, fi.minexp) - fi.nmant), 0.0)


def fixture_row(G, name, tn):
    """The stored arrays of one (row, type): x (list of operands) and the expectations.  The file holds one array per (type, kind),
    the rows one after another in the order of `names`, `n` points each."""
    row = BY_NAME[name]
    names = [str(s) for s in G[tn + ".names"]]
    counts = G[tn + ".n"].astype(np.int64)
    i = names.index(name)
    n = int(counts[i])
    o = int(counts[:i].sum())
    ox = int(sum(counts[j] * BY_NAME[names[j]].arity for j in range(i)))
    total = int(counts.sum())
    xs = [G[tn + ".x"][ox + k * n: ox + (k + 1) * n] for k in range(row.arity)]
    bits = lambda key: np.unpackbits(G[tn + "." + key])[:total].astype(bool)[o:o + n]  # noqa: E731
    d = {"x": xs, "n": n}
    if row.cls == "faithful":
        d["lo"], d["exact"], d["special"] = G[tn + ".lo"][o:o + n], bits("ex"), bits("sp")
    else:
        hi, l8 = G[tn + ".hi"][o:o + n], G[tn + ".lo8"][o:o + n]
        # the rest of the exact value, in 1/254 of the spacing of each part of hi (in the row's type)
        lo = l8[:, 0] / 254.0 * spacing_of(hi.real) + 1j * (l8[:, 1] / 254.0 * spacing_of(hi.imag))
        d["hi"], d["lo"], d["edge"], d["axis"] = hi.astype(C128), lo, bits("edge"), bits("axis")
        d["sign_re"], d["sign_im"] = bits("sre"), bits("sim")  # of exact zero parts on the real axis
    return d


def reference(name, tn, xs):
    """The CPU reference of an inexact row on inputs xs, in the row's type: the oracle's std::complex for the base opcodes of the
    complex classes, NumPy in Float64 / complex128 rounded once for everything else."""
    row = BY_NAME[name]
    T = TYPES[tn]
    if row.ref == "oracle":
        from util import run_oracle
        dst = S.StridedView(np.zeros(len(xs[0]), dtype=T, order="F"))
        src = tuple(S.StridedView(np.asfortranarray(x).copy(order="F")) for x in xs)
        return np.asarray(run_oracle(row.f, None, None, dst.size, (dst,) + src))
    wide = C128 if np.dtype(T).kind == "c" else F64
    with np.errstate(all="ignore"):
        return np.asarray(row.ref(*[x.astype(wide) for x in xs])).astype(T)


def complex_judge(name, tn, d):
    """The bound of a complex row from the CPU reference on the row's own points: err = the reference's error per point, keep = the
    points judged (edge and real-axis points always; the others where the reference is within 2 ulp), E_ref = its largest error on the kept main
    points, bound = E_ref + L."""
    row = BY_NAME[name]
    ref = reference(name, tn, d["x"])
    err = cx_error(ref, d["hi"], d["lo"], tn)
    keep = d["edge"] | d["axis"] | (err <= 2.0)
    e_ref = float(err[keep & ~d["edge"] & ~d["axis"]].max())
    return {"ref": ref, "err": err, "keep": keep, "E_ref": e_ref, "bound": e_ref + row.L, "dropped": int((~keep).sum()),
            "main": int((~d["edge"]).sum())}


def complex_failures(got, name, tn, d, j):
    """indices of the kept points where `got` misses the row's bound (normwise everywhere, part by part on the real axis)"""
    e = cx_error(got, d["hi"], d["lo"], tn)
    bad = j["keep"] & ~(e <= j["bound"])
    if d["axis"].any():
        bad |= d["axis"] & j["keep"] & ~axis_ok(got, d["hi"], d["lo"], d["sign_re"], d["sign_im"], j["bound"], tn)
    return np.nonzero(bad)[0], e
