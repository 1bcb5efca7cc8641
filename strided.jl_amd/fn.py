"""Whitelisted elementwise functions usable inside fused expressions -- on `Arg` placeholders when
tracing a map! closure, and on StridedView / Broadcasted operands for dot-fusion (the Python
spelling of `sin.(A)`, `max.(abs.(B1), real.(B3))`, ... from test/othertests.jl:46-66)."""
from __future__ import annotations

import builtins
import cmath
import math
import numbers

import numpy as np

from .expr import _OpsMixin, as_expr


def _node(op, *args):
    for a in args:
        if isinstance(a, _OpsMixin):
            return a._make(op, *args)
    for a in args:  # StridedView (gets _make from broadcast.py)
        if hasattr(a, "_make"):
            return a._make(op, *args)
    return None


def _unary(op, pyf):
    def g(x):
        n = _node(op, x)
        if n is not None:
            return n
        if isinstance(x, (numbers.Number, np.generic)):
            return pyf(x)
        raise TypeError(f"{op}: unsupported argument {type(x)}")
    g.__name__ = op
    return g


def _cm(realf, cplxf):
    return lambda x: cplxf(x) if isinstance(x, complex) else realf(x)


identity = lambda x: x  # noqa: E731
neg = _unary("neg", lambda x: -x)
abs = _unary("abs", lambda x: x.__abs__())  # noqa: A001
abs2 = _unary("abs2", lambda x: (x * x.conjugate()).real if isinstance(x, complex) else x * x)
conj = _unary("conj", lambda x: x.conjugate())
real = _unary("real", lambda x: x.real)
imag = _unary("imag", lambda x: x.imag)
sqrt = _unary("sqrt", _cm(math.sqrt, cmath.sqrt))
exp = _unary("exp", _cm(math.exp, cmath.exp))
log = _unary("log", _cm(math.log, cmath.log))
sin = _unary("sin", _cm(math.sin, cmath.sin))
cos = _unary("cos", _cm(math.cos, cmath.cos))
tanh = _unary("tanh", _cm(math.tanh, cmath.tanh))
inv = _unary("inv", lambda x: 1 / x)


def _binary(op, pyf):
    def g(x, y, *more):
        n = _node(op, x, y, *more)
        if n is not None:
            return n
        r = pyf(x, y)
        for m in more:
            r = pyf(r, m)
        return r
    g.__name__ = op
    return g


add = _binary("add", lambda a, b: a + b)
sub = _binary("sub", lambda a, b: a - b)
mul = _binary("mul", lambda a, b: a * b)
div = _binary("div", lambda a, b: a / b)
min = _binary("min", lambda a, b: b if b < a else a)  # noqa: A001
max = _binary("max", lambda a, b: b if a < b else a)  # noqa: A001
lt = _binary("lt", lambda a, b: a < b)
le = _binary("le", lambda a, b: a <= b)
gt = _binary("gt", lambda a, b: a > b)
ge = _binary("ge", lambda a, b: a >= b)
eq = _binary("eq", lambda a, b: a == b)
ne = _binary("ne", lambda a, b: a != b)


# ---- math opcodes: runtime-compiled kernels only (include/strided_hip.h) -----------------------------------------------
def _sign(x):
    if isinstance(x, complex):
        return x if x == 0 else x / builtins.abs(x)
    if isinstance(x, numbers.Integral):
        return type(x)((x > 0) - (x < 0))
    return x if (x == 0 or x != x) else math.copysign(1.0, x)


def _round(x):
    if isinstance(x, complex):
        return complex(builtins.round(x.real), builtins.round(x.imag))
    return x if isinstance(x, numbers.Integral) else float(builtins.round(x))  # Python's round: ties to even, like RoundNearest


def _rem(a, b):
    if isinstance(a, numbers.Integral) and isinstance(b, numbers.Integral):
        r = builtins.abs(a) % builtins.abs(b)
        return -r if a < 0 else r
    return math.fmod(a, b)


tan = _unary("tan", _cm(math.tan, cmath.tan))
asin = _unary("asin", _cm(math.asin, cmath.asin))
acos = _unary("acos", _cm(math.acos, cmath.acos))
sinh = _unary("sinh", _cm(math.sinh, cmath.sinh))
cosh = _unary("cosh", _cm(math.cosh, cmath.cosh))
exp2 = _unary("exp2", lambda x: 2.0 ** x)
expm1 = _unary("expm1", math.expm1)
log2 = _unary("log2", _cm(math.log2, lambda z: cmath.log(z) / math.log(2)))
log10 = _unary("log10", _cm(math.log10, cmath.log10))
log1p = _unary("log1p", math.log1p)
cbrt = _unary("cbrt", lambda x: math.copysign(builtins.abs(x) ** (1.0 / 3.0), x))
floor = _unary("floor", lambda x: x if isinstance(x, numbers.Integral) else float(math.floor(x)))
ceil = _unary("ceil", lambda x: x if isinstance(x, numbers.Integral) else float(math.ceil(x)))
trunc = _unary("trunc", lambda x: x if isinstance(x, numbers.Integral) else float(math.trunc(x)))
round = _unary("round", _round)  # noqa: A001  RoundNearest (ties to even)
sign = _unary("sign", _sign)
not_ = _unary("not", lambda x: not x if isinstance(x, (bool, np.bool_)) else ~x)  # Julia's ~ (! on Bool)
_atan1 = _unary("atan", _cm(math.atan, cmath.atan))
_atan2 = _binary("atan2", math.atan2)


def atan(y, x=None):
    """atan(y) or, with two arguments, atan(y, x) (the angle of the point (x, y))."""
    return _atan1(y) if x is None else _atan2(y, x)


hypot = _binary("hypot", math.hypot)
rem = _binary("rem", _rem)  # truncated (Julia's rem / %)
mod = _binary("mod", lambda a, b: a % b)  # floored (Julia's mod, Python's %)
pow = _binary("pow", lambda a, b: a ** b)  # noqa: A001  an int literal exponent in int8 range is Base.literal_pow (POWI)
and_ = _binary("and", lambda a, b: a & b)
or_ = _binary("or", lambda a, b: a | b)
xor = _binary("xor", lambda a, b: a ^ b)


def fma(a, b, c):
    """fma(a, b, c): a*b + c rounded once."""
    n = _node("fma", a, b, c)
    if n is not None:
        return n
    if all(isinstance(v, numbers.Real) for v in (a, b, c)) and hasattr(math, "fma"):
        return math.fma(a, b, c)
    return a * b + c


muladd = fma


def ifelse(c, a, b):
    n = _node("select", c, a, b)
    if n is not None:
        return n
    return a if c else b


select = ifelse
__all__ = [k for k in list(globals()) if not k.startswith("_") and k not in
           ("annotations", "cmath", "math", "numbers", "np", "as_expr", "builtins")]
