"""Symbolic form of the fused elementwise function `f` and its serialisation to the f-program
bytecode of include/strided_hip.h.

In the reference `f` is an arbitrary Julia closure: map!'s argument (src/mapreduce.jl:38-53) or
the `CaptureArgs` functor tree that broadcast lowering builds (src/broadcast.jl:67-98), whose
`Arg()` leaves consume the array values positionally, depth first, and whose inner nodes apply
`bc.f` left to right.  A closure cannot cross a C ABI, so the host side traces it: `f` is called
once with `Arg` placeholders and the resulting tree of whitelisted operations is emitted as
postfix code.  Anything outside the whitelist raises (the Julia shim would fall back to the CPU
method).
"""
from __future__ import annotations

import numbers

import numpy as np

from ._lib import OPCODES, SMR_MAXCONST, SMR_MAXPROG

_UNARY = {"neg": "NEG", "abs": "ABS", "abs2": "ABS2", "conj": "CONJ", "real": "REAL", "imag": "IMAG",
          "sqrt": "SQRT", "exp": "EXP", "log": "LOG", "sin": "SIN", "cos": "COS", "tanh": "TANH",
          "inv": "INV"}
_BINARY = {"add": "ADD", "sub": "SUB", "mul": "MUL", "div": "DIV", "min": "MIN", "max": "MAX",
           "lt": "LT", "le": "LE", "gt": "GT", "ge": "GE", "eq": "EQ", "ne": "NE"}
_NARY_FOLD = {"add", "mul", "min", "max"}  # Julia's +(a,b,c,d) folds left: ((a+b)+c)+d
# math opcodes (runtime-compiled kernels only, include/strided_hip.h).  "pow" with a Python int literal in int8 range as its
# exponent is Base.literal_pow: POWI, the exponent in the immediate; "not" on a Bool-typed value is XOR with true
_UNARY.update({"tan": "TAN", "asin": "ASIN", "acos": "ACOS", "atan": "ATAN", "sinh": "SINH", "cosh": "COSH", "exp2": "EXP2",
               "expm1": "EXPM1", "log2": "LOG2", "log10": "LOG10", "log1p": "LOG1P", "cbrt": "CBRT", "floor": "FLOOR",
               "ceil": "CEIL", "trunc": "TRUNC", "round": "ROUND", "sign": "SIGN", "not": "NOT"})
_BINARY.update({"pow": "POW", "atan2": "ATAN2", "hypot": "HYPOT", "rem": "REM", "mod": "MOD", "and": "AND", "or": "OR",
                "xor": "XOR"})
_TERNARY = {"fma": "FMA"}
_FLOAT_UNARY = {"sqrt", "exp", "log", "sin", "cos", "tanh", "inv", "tan", "asin", "acos", "atan", "sinh", "cosh", "exp2", "expm1",
                "log2", "log10", "log1p", "cbrt"}
_BITS = {"and", "or", "xor", "not"}
_NO_COMPLEX = {"floor", "ceil", "trunc", "cbrt", "hypot", "rem", "mod", "atan2"} | _BITS  # MethodError in Julia
_NO_COMPLEX_DEVICE = {"tan", "asin", "acos", "atan", "expm1", "log1p", "pow"}          # defined in Julia, not on the device


class _OpsMixin:
    """Operator overloading shared by Expr (map! closures) and Broadcasted (dot-fusion)."""

    # NumPy scalars on the LEFT (`np.float32(0.5) * a`) must reach __rmul__ & co. as they are: without this NumPy converts the
    # scalar to a Python float first and a Float32 literal would silently become a Float64 one (and widen the whole call)
    __array_ufunc__ = None

    @classmethod
    def _make(cls, op, *args):  # overridden
        raise NotImplementedError

    def __add__(self, o): return self._make("add", self, o)
    def __radd__(self, o): return self._make("add", o, self)
    def __sub__(self, o): return self._make("sub", self, o)
    def __rsub__(self, o): return self._make("sub", o, self)
    def __mul__(self, o): return self._make("mul", self, o)
    def __rmul__(self, o): return self._make("mul", o, self)
    def __truediv__(self, o): return self._make("div", self, o)
    def __rtruediv__(self, o): return self._make("div", o, self)
    def __neg__(self): return self._make("neg", self)
    def __pos__(self): return self
    def __abs__(self): return self._make("abs", self)
    def __lt__(self, o): return self._make("lt", self, o)
    def __le__(self, o): return self._make("le", self, o)
    def __gt__(self, o): return self._make("gt", self, o)
    def __ge__(self, o): return self._make("ge", self, o)
    def __pow__(self, o): return self._make("pow", self, o)
    def __rpow__(self, o): return self._make("pow", o, self)
    def __mod__(self, o): return self._make("mod", self, o)  # Python's % is floored, like Julia's mod
    def __rmod__(self, o): return self._make("mod", o, self)
    def __and__(self, o): return self._make("and", self, o)
    def __rand__(self, o): return self._make("and", o, self)
    def __or__(self, o): return self._make("or", self, o)
    def __ror__(self, o): return self._make("or", o, self)
    def __xor__(self, o): return self._make("xor", self, o)  # Python's ^ is xor; power is **
    def __rxor__(self, o): return self._make("xor", o, self)
    def __invert__(self): return self._make("not", self)
    # == / != stay Python identity semantics; use fn.eq / fn.ne for elementwise comparison
    __hash__ = object.__hash__


class Expr(_OpsMixin):
    @classmethod
    def _make(cls, op, *args):
        return Call(op, tuple(as_expr(a) for a in args))


class Arg(Expr):
    """Placeholder for the k-th array argument (1-based), `Arg()` of src/broadcast.jl:71-72."""

    def __init__(self, index: int):
        self.index = int(index)

    def __repr__(self):
        return f"a{self.index}"


class Const(Expr):
    """A captured scalar (src/broadcast.jl:81-83: Ref / 0-dim args are unwrapped, other
    non-array args captured as they are)."""

    def __init__(self, value):
        # a Python int literal: `x ** 3` is Base.literal_pow(^, x, Val(3))
        self.literal = int(value) if isinstance(value, numbers.Integral) and not isinstance(value, (bool, np.generic)) else None
        if isinstance(value, (np.generic,)):
            self.dtype = value.dtype           # strongly typed, like a Julia Float32 literal
            value = value.item()
        elif isinstance(value, bool):
            self.dtype = None                  # weak (Julia Bool/Int do not widen floats)
        elif isinstance(value, numbers.Integral):
            self.dtype = None
            # constants travel as Float64: an integer beyond 2^53 must survive that exactly -- or be one of the type
            # limits the integer class saturates to (typemax(Int64) / typemin(Int64), the seeds of min / max)
            iv = int(value)
            if abs(iv) > 2 ** 53 and int(float(iv)) != iv and iv not in (2 ** 63 - 1, -2 ** 63):
                raise OverflowError(f"integer constant {iv} is not representable in the f-program (Float64 constants)")
        elif isinstance(value, numbers.Rational):
            self.dtype = None                  # Fraction ~ Julia Rational: takes the array's float type
            value = value.numerator / value.denominator
        elif isinstance(value, numbers.Real):
            self.dtype = np.dtype(np.float64)  # a Python float is Julia's Float64
        elif isinstance(value, numbers.Complex):
            self.dtype = np.dtype(np.complex128)
        elif hasattr(value, "numerator") and hasattr(value, "denominator"):
            self.dtype = None                  # Fraction ~ Julia Rational: takes the array's float type
            value = value.numerator / value.denominator
        else:
            raise TypeError(f"cannot capture {type(value)} as a broadcast constant")
        self.value = complex(value)

    def __repr__(self):
        return f"{self.value.real:g}" if self.value.imag == 0 else f"{self.value:g}"


class Call(Expr):
    def __init__(self, op: str, args: tuple):
        if op not in _UNARY and op not in _BINARY and op not in _TERNARY and op != "select":
            raise NotImplementedError(f"operation {op!r} is outside the device whitelist")
        self.op, self.args = op, args

    def __repr__(self):
        return f"{self.op}({', '.join(map(repr, self.args))})"


def as_expr(x) -> Expr:
    if isinstance(x, Expr):
        return x
    if hasattr(x, "numerator") or isinstance(x, (numbers.Number, np.generic)):
        return Const(x)
    raise TypeError(f"cannot use {type(x)} inside a fused elementwise function")


# ---- tracing --------------------------------------------------------------------------------------
def trace(f, nargs: int) -> Expr:
    """Turn map!'s `f` into an Expr by calling it on placeholders.  `f` may already be an Expr
    (e.g. a CaptureArgs tree from broadcast lowering) or one of a few names."""
    if isinstance(f, Expr):
        return f
    if isinstance(f, str):
        from . import fn
        f = getattr(fn, f)
    out = f(*[Arg(i + 1) for i in range(nargs)])
    return as_expr(out)


# ---- serialisation ---------------------------------------------------------------------------------
def powi_exponent(n):
    """n of `x ** n` for a Python int literal n in int8 range (POWI), else None (POW)."""
    if isinstance(n, Call) and n.op == "pow" and isinstance(n.args[1], Const) and n.args[1].literal is not None \
            and -128 <= n.args[1].literal <= 127:
        return n.args[1].literal
    return None


def _jl_promote(*ts):
    """Julia's promote_type over real / complex NumPy dtypes (Bool yields to everything; Int8 with UInt16 is UInt16;
    a float wins over any integer: Float32 with Int64 is Float32)."""
    ts = [np.dtype(t) for t in ts]
    cx = any(t.kind == "c" for t in ts)
    re = [_real_of(t) for t in ts]
    fl = [t for t in re if t.kind == "f"]
    if fl:
        r = max(fl, key=lambda t: t.itemsize)
    else:
        ints = [t for t in re if t != np.bool_]
        if not ints:
            r = np.dtype(np.bool_)
        else:
            w = max(t.itemsize for t in ints)
            same = [t for t in ints if t.itemsize == w]
            r = same[0] if all(t.kind == "i" for t in same) else next(t for t in same if t.kind == "u")
    if cx:
        r = np.dtype(np.complex64) if r == np.float32 else np.dtype(np.complex128)
    return r


def _math_dtype(n, ts):
    """node_dtype of the math opcodes; raises where Julia has no method (TypeError) or the device has none."""
    strong = [t for t in ts if t is not None]
    if any(t.kind == "c" for t in strong):
        if n.op in _NO_COMPLEX:
            raise TypeError(f"{n.op} has no method for complex values")
        if n.op in _NO_COMPLEX_DEVICE and powi_exponent(n) is None:
            from ._lib import UnsupportedOnDevice, SMR_EUNSUPPORTED
            raise UnsupportedOnDevice(SMR_EUNSUPPORTED, f"complex {n.op} is not available on the device")
    if n.op in _BITS and any(t.kind in "fc" for t in strong):
        raise TypeError(f"bitwise {n.op} needs integer or Bool values")
    if n.op in _FLOAT_UNARY:
        return _float_of(strong[0]) if strong else np.dtype(np.float64)
    if n.op in ("atan2", "hypot"):
        return _float_of(_jl_promote(*strong)) if strong else np.dtype(np.float64)
    if n.op in ("floor", "ceil", "trunc", "round", "sign", "not"):
        return strong[0] if strong else None
    if n.op == "pow":
        k = powi_exponent(n)
        if ts[0] is None:
            return _jl_promote(*strong) if strong else None
        if k is not None and k < 0 and ts[0].kind in "biu":
            return np.dtype(np.float64)  # literal_pow: inv(x) of an integer
        if k is not None or (ts[1] is not None and ts[1].kind in "biu") or (ts[1] is None and n.args[1].literal is not None):
            return ts[0]  # x ^ n::Integer keeps the type of x
        return _jl_promote(*strong)
    if n.op in ("rem", "mod"):
        # an integer literal is an Int64: mod(::Int16, 7) is an Int64, mod(::Float32, 7) a Float32
        if any(t.kind in "biu" for t in strong) and not any(t.kind in "fc" for t in strong) and \
                any(isinstance(a, Const) and a.dtype is None for a in n.args):
            strong = strong + [np.dtype(np.int64)]
    if not strong:
        return None
    return _jl_promote(*strong)  # and / or / xor (Bool & Bool is a Bool), rem, mod, fma


def node_dtype(n, arg_dtypes):
    """Element type Julia would give this sub-expression (None = weakly typed constant)."""
    if isinstance(n, Arg):
        return np.dtype(arg_dtypes[n.index - 1])
    if isinstance(n, Const):
        return n.dtype
    ts = [node_dtype(a, arg_dtypes) for a in n.args]
    if n.op in _TERNARY or n.op in ("pow", "atan2", "hypot", "rem", "mod", "and", "or", "xor") or \
            (n.op in _UNARY and OPCODES[_UNARY[n.op]] >= OPCODES["POWI"]):
        return _math_dtype(n, ts)
    strong = [t for t in ts if t is not None]
    if n.op in ("lt", "le", "gt", "ge", "eq", "ne"):
        return np.dtype(np.bool_)
    if n.op in ("abs", "abs2", "real", "imag"):
        return _real_of(strong[0]) if strong else None
    if n.op in ("sqrt", "exp", "log", "sin", "cos", "tanh", "inv"):
        return _float_of(strong[0]) if strong else np.dtype(np.float64)
    if n.op == "select":
        strong = [t for t in ts[1:] if t is not None]
    if not strong:
        return None
    # + - * / min max ifelse: both arguments are converted to Julia's promote_type (a float beats any integer: Float32 + Int64 is a
    # Float32; Int32 + UInt32 is a UInt32) -- not NumPy's result_type, which widens until the type holds both
    r = _jl_promote(*strong)
    if n.op == "div" and r.kind not in "fc":
        r = np.dtype(np.float64)
    if r == np.bool_ and n.op in ("add", "sub", "mul"):
        r = np.dtype(np.int64)
    return np.dtype(r)


def serialize(e: Expr, arg_dtypes=None, wide: bool = False):
    """Expr -> (code bytes, constants as (re, im) list).  Post-order; leaves are visited left to
    right, which is the order `consume` pops array values in (src/broadcast.jl:86-98).

    Per-operation typing: Julia types every operation of the fused expression separately
    (`Float32 .* Float32` is a Float32 product even when the result is later widened), the device
    computes a whole call in one class.  When the call computes in Float64 (`wide`) although an
    operation's Julia type is Float32 / ComplexF32, a ROUND32 follows it: for + - * / sqrt the
    double-rounded result equals the Float32 operation exactly (53 >= 2*24 + 2 bits)."""
    code, consts = [], []
    narrow = (np.dtype(np.float32), np.dtype(np.complex64))

    def rounds(node) -> bool:
        if not wide or arg_dtypes is None or not isinstance(node, Call):
            return False
        if node.op == "select":
            return False  # picks one of two already rounded values
        return node_dtype(node, arg_dtypes) in narrow

    _F32_HOLDS_NOT = (np.dtype(np.int32), np.dtype(np.uint32), np.dtype(np.int64), np.dtype(np.uint64))

    def narrow_parent(node) -> bool:
        """Is `node` an operation Julia carries out in Float32 / ComplexF32 after converting its arguments (promotion), while the
        call computes wider?"""
        return wide and arg_dtypes is not None and isinstance(node, Call) and (node.op in ("add", "sub", "mul", "div", "min", "max")) \
            and node_dtype(node, arg_dtypes) in narrow

    def emit_arg(a, parent):
        """An argument of `parent`.  Julia converts it to the operation's type BEFORE operating: an Int32 / UInt32 / Int64 / UInt64
        value that Float32 does not hold is rounded there (`Float32[1] .+ Int32[16777217]` is 16777216, not the exact sum rounded
        once), so a ROUND32 follows the argument; a weak integer literal is folded to Float32 on the host."""
        if narrow_parent(parent):
            if isinstance(a, Const):
                integer = a.literal is not None if a.dtype is None else a.dtype in _F32_HOLDS_NOT
                if integer and float(np.float32(a.value.real)) != a.value.real:
                    code.extend((OPCODES["CONST"], const_index(complex(float(np.float32(a.value.real)), 0.0))))
                    return
            emit(a)
            if not isinstance(a, Const) and node_dtype(a, arg_dtypes) in _F32_HOLDS_NOT:
                code.extend((OPCODES["ROUND32"], 0))
            return
        emit(a)

    def const_index(v: complex) -> int:
        for i, c in enumerate(consts):
            if c == v and np.signbit(c.real) == np.signbit(v.real) and np.signbit(c.imag) == np.signbit(v.imag):
                return i
        consts.append(v)
        if len(consts) > SMR_MAXCONST:
            raise NotImplementedError("too many captured constants for the device f-program")
        return len(consts) - 1

    def emit(node):
        if isinstance(node, Arg):
            code.extend((OPCODES["ARG"], node.index))
        elif isinstance(node, Const):
            code.extend((OPCODES["CONST"], const_index(node.value)))
        elif isinstance(node, Call):
            k = powi_exponent(node)
            if k is not None:
                emit(node.args[0])
                code.extend((OPCODES["POWI"], k & 0xFF))
                if rounds(node):
                    code.extend((OPCODES["ROUND32"], 0))
            elif node.op == "not" and arg_dtypes is not None and node_dtype(node.args[0], arg_dtypes) == np.bool_:
                emit(node.args[0])  # !x / ~x on a Bool is xor(x, true): NOT would give ~1 = -2
                code.extend((OPCODES["CONST"], const_index(1 + 0j), OPCODES["XOR"], 0))
            elif node.op in _UNARY:
                emit(node.args[0])
                code.extend((OPCODES[_UNARY[node.op]], 0))
                if rounds(node):
                    code.extend((OPCODES["ROUND32"], 0))
            elif node.op == "select":
                for a in node.args:
                    emit(a)
                code.extend((OPCODES["SELECT"], 0))
            elif node.op in _TERNARY:
                if len(node.args) != 3:
                    raise ValueError(f"{node.op} takes three arguments")
                for a in node.args:
                    emit(a)
                code.extend((OPCODES[_TERNARY[node.op]], 0))
                if rounds(node):
                    code.extend((OPCODES["ROUND32"], 0))
            else:
                if len(node.args) < 2 or (len(node.args) > 2 and node.op not in _NARY_FOLD):
                    raise ValueError(f"{node.op} takes two arguments")
                if len(node.args) > 2:  # a left fold, typed step by step: +(i, j, a) is Float32(i + j) + a, (a32 + b32) + c64 rounds its first sum
                    emit(Call(node.op, (Call(node.op, node.args[:-1]), node.args[-1])))
                    return
                emit_arg(node.args[0], node)
                emit_arg(node.args[1], node)
                code.extend((OPCODES[_BINARY[node.op]], 0))
                if rounds(node):
                    code.extend((OPCODES["ROUND32"], 0))
        else:
            raise TypeError(type(node))

    emit(e)
    if wide and arg_dtypes is not None and not any(
            np.dtype(t) in (np.dtype(np.float64), np.dtype(np.complex128)) or np.issubdtype(np.dtype(t), np.integer) or np.dtype(t) == np.bool_
            for t in arg_dtypes):
        # the 64-bit class comes from a scalar, not from an operand: tell the library (SMR_OP_WIDEN)
        code.extend((OPCODES["WIDEN"], 0))
    if len(code) // 2 > SMR_MAXPROG:
        raise NotImplementedError("fused expression too long for the device f-program")
    return bytes(code), consts


def needs_wide(e: Expr, arg_dtypes) -> bool:
    """Does Julia evaluate some part of f in a 64-bit (or integer) type?  True for Float64 / ComplexF64 /
    integer arrays, and for strongly typed 64-bit scalars (`A32 .* 0.1`: a Float64 literal)."""
    wide = (np.dtype(np.float64), np.dtype(np.complex128))

    def walk(n):
        t = node_dtype(n, arg_dtypes)
        if t is not None and (t in wide or np.issubdtype(t, np.integer)):
            return True
        return isinstance(n, Call) and any(walk(a) for a in n.args)

    return walk(e)


def max_arg(e: Expr) -> int:
    if isinstance(e, Arg):
        return e.index
    if isinstance(e, Call):
        return max((max_arg(a) for a in e.args), default=0)
    return 0


# ---- result element type (Broadcast.combine_eltypes analogue) ---------------------------------------
def _real_of(dt):
    dt = np.dtype(dt)
    if dt == np.complex64:
        return np.dtype(np.float32)
    if dt == np.complex128:
        return np.dtype(np.float64)
    return dt


def _float_of(dt):
    dt = np.dtype(dt)
    if np.issubdtype(dt, np.inexact):
        return dt
    return np.dtype(np.float64)


def result_dtype(e: Expr, arg_dtypes):
    """Element type Julia would infer for f(args...): weak (Int/Bool/Rational) constants do not
    widen, a Python float is a Float64, comparisons give Bool."""

    r = node_dtype(e, arg_dtypes)
    return np.dtype(np.float64) if r is None else r
