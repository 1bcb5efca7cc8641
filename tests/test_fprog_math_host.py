"""The math opcodes of the f-program (powers, fma / muladd, more of Base's math, rem / mod and the bitwise operations), host side:
the tables of the three front ends agree, the Python front end serialises and types like Julia, the planner types the integer class,
refuses what it must, and the generated JIT source compiles with hiprtc for gfx950 in every kernel family (no device needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import strided_jl_amd as S
from strided_jl_amd import expr as E

fn = S.fn
L = S._lib
OP = dict(L.OPCODES, WRAP_I32=25, WRAP_U8=26, WRAP_U16=27)  # SMR_OP_WRAP_*: the library's own (strided_hip.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "strided_hip.h")).read()
JL = open(os.path.join(ROOT, "julia", "StridedHIP.jl")).read()
MATH = ["FMA", "POWI", "TAN", "ASIN", "ACOS", "ATAN", "SINH", "COSH", "EXP2", "EXPM1", "LOG2", "LOG10", "LOG1P", "CBRT", "FLOOR",
        "CEIL", "TRUNC", "ROUND", "SIGN", "NOT", "POW", "ATAN2", "HYPOT", "REM", "MOD", "AND", "OR", "XOR"]


def _v(shape, dtype=np.float64):
    return S.StridedView(np.zeros(shape, dtype=dtype, order="F"))


def _jl_dict(name):
    body = re.search(r"const " + name + r" = Dict\((.*?)\)\n", JL, re.S).group(1)
    out = {}
    for item in re.split(r",\s*", body.replace("\n", " ")):
        k, v = item.rsplit(" => ", 1)
        k = k.strip()
        out[k[1:-1] if k.startswith("(") else k] = int(v)
    return out


def ser(f, *dtypes, wide=None):
    """(opcode, imm) pairs and constants of f for input dtypes (destination of the first input's dtype)"""
    dts = [np.dtype(d) for d in dtypes]
    e = E.trace(f, len(dts))
    if wide is None:
        wide = any(d in (np.dtype(np.float64), np.dtype(np.complex128)) or d.kind in "biu" for d in dts) or E.needs_wide(e, dts)
    code, consts = E.serialize(e, dts, wide)
    return [(code[i], code[i + 1]) for i in range(0, len(code), 2)], consts


# ---- tables -------------------------------------------------------------------------------------------------------------------
def test_opcode_values_agree_across_header_python_and_julia():
    hdr = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSMR_OP_(\w+)\s*=\s*(\d+)", HDR)}
    for k in MATH:
        assert hdr[k] == OP[k], k
    assert OP["FMA"] == 65 and OP["POWI"] == 96 and OP["NOT"] == 114 and OP["POW"] == 128 and OP["XOR"] == 135
    un = _jl_dict("UNARY_MATH")
    names = {"tan": "TAN", "asin": "ASIN", "acos": "ACOS", "atan": "ATAN", "sinh": "SINH", "cosh": "COSH", "exp2": "EXP2",
             "expm1": "EXPM1", "log2": "LOG2", "log10": "LOG10", "log1p": "LOG1P", "cbrt": "CBRT", "floor": "FLOOR", "ceil": "CEIL",
             "trunc": "TRUNC", "round": "ROUND", "sign": "SIGN", "~": "NOT"}
    assert un == {k: OP[v] for k, v in names.items()}
    bi = _jl_dict("BINARY_MATH")
    names = {"^": "POW", "atan": "ATAN2", "hypot": "HYPOT", "rem": "REM", "mod": "MOD", "&": "AND", "|": "OR", "xor": "XOR"}
    assert bi == {k: OP[v] for k, v in names.items()}
    m = re.search(r"const OP_FMA, OP_POWI, OP_XOR, UNARY_ALL, BINARY_ALL = (0x\w+), (0x\w+), (0x\w+)", JL)
    assert [int(x, 16) for x in m.groups()] == [OP["FMA"], OP["POWI"], OP["XOR"]]
    # the shim's lowering rules: literal_pow, fma / muladd, Bool ! / ~ as xor(x, true), tracer methods
    assert "f === Base.literal_pow" in JL and "f in (fma, muladd)" in JL and "f in (!, ~)" in JL and "push!(p.code, OP_XOR" in JL
    assert "Base.:^(x::Traced, n::Integer)" in JL and "Base.literal_pow(::typeof(^), x::Traced" in JL
    assert "SMR_ABI_VERSION 1" in HDR


# ---- serialisation ----------------------------------------------------------------------------------------------------------------
def test_powers_serialise_as_powi_or_pow():
    f32 = np.float32
    assert ser(lambda a: a ** 2, f32) == ([(OP["ARG"], 1), (OP["POWI"], 2)], [])
    assert ser(lambda a: a ** -1, f32)[0] == [(OP["ARG"], 1), (OP["POWI"], 0xFF)]
    assert ser(lambda a: a ** -128, f32)[0][-1] == (OP["POWI"], 0x80)
    code, consts = ser(lambda a: a ** 2.5, np.float64)
    assert code == [(OP["ARG"], 1), (OP["CONST"], 0), (OP["POW"], 0)] and consts == [2.5]
    assert ser(lambda a: a ** 200, np.float64)[0][-1] == (OP["POW"], 0)  # outside int8: POW with the constant
    assert ser(lambda a, b: a ** b, np.float64, np.float64)[0] == [(OP["ARG"], 1), (OP["ARG"], 2), (OP["POW"], 0)]
    assert ser(lambda a: fn.pow(a, 3), np.float64)[0] == [(OP["ARG"], 1), (OP["POWI"], 3)]
    # through a broadcast of StridedViews: A ** 2 is a Broadcasted node, lowered the same way
    A = _v((4, 4))
    bc = A ** 2
    assert S.broadcast.make_capture(bc).op == "pow" and E.powi_exponent(S.broadcast.make_capture(bc)) == 2


def test_fma_mod_and_bit_operators():
    c, _ = ser(lambda a, b, d: fn.fma(a, b, d), np.float64, np.float64, np.float64)
    assert c == [(OP["ARG"], 1), (OP["ARG"], 2), (OP["ARG"], 3), (OP["FMA"], 0)]
    assert ser(lambda a, b, d: fn.muladd(a, b, d), np.float32, np.float32, np.float32)[0][-1] == (OP["FMA"], 0)
    c, k = ser(lambda a: a % 7, np.int32)
    assert c == [(OP["ARG"], 1), (OP["CONST"], 0), (OP["MOD"], 0)] and k == [7]
    assert ser(lambda a, b: fn.rem(a, b), np.float64, np.float64)[0][-1] == (OP["REM"], 0)
    # ~ on a Bool is xor(x, true); on Int32 the complement
    c, k = ser(lambda m: ~m, np.bool_)
    assert c == [(OP["ARG"], 1), (OP["CONST"], 0), (OP["XOR"], 0)] and k == [1]
    assert ser(lambda m: ~m, np.int32)[0] == [(OP["ARG"], 1), (OP["NOT"], 0)]
    assert ser(lambda a, b: fn.not_(a < b), np.float32, np.float32)[0][-2:] == [(OP["CONST"], 0), (OP["XOR"], 0)]
    c, _ = ser(lambda a, b: (a > 0) & (b < 1), np.float64, np.float64)
    assert c[-1] == (OP["AND"], 0)
    assert ser(lambda a, b: a | b, np.uint8, np.uint8)[0][-1] == (OP["OR"], 0)
    assert ser(lambda a, b: a ^ b, np.int16, np.int16)[0][-1] == (OP["XOR"], 0)
    assert ser(lambda a, b: fn.atan(a, b), np.float64, np.float64)[0][-1] == (OP["ATAN2"], 0)
    assert ser(lambda a: fn.atan(a), np.float64)[0][-1] == (OP["ATAN"], 0)
    # operators on StridedView build the same nodes
    M, A = _v((4,), np.bool_), _v((4,), np.int32)
    assert (~M).f == "not" and (A % 3).f == "mod" and (A & A).f == "and" and (A | A).f == "or" and (A ^ A).f == "xor"
    assert (2 ** A).f == "pow" and (A ** 2).f == "pow"


def test_round32_follows_narrow_math_in_wide_calls():
    # A32 ** 3 + B64: the Float32 power is rounded to Float32 before the Float64 addition
    c, _ = ser(lambda a, b: a ** 3 + b, np.float32, np.float64)
    assert c == [(OP["ARG"], 1), (OP["POWI"], 3), (OP["ROUND32"], 0), (OP["ARG"], 2), (OP["ADD"], 0)]
    c, _ = ser(lambda a, b, d: fn.fma(a, b, d), np.float32, np.float32, np.float64)
    assert c[-1] == (OP["FMA"], 0)  # Julia promotes first: a Float64 fma
    c, _ = ser(lambda a: fn.tan(a) * a, np.float32, wide=True)
    assert c[:6] == [(OP["ARG"], 1), (OP["TAN"], 0), (OP["ROUND32"], 0), (OP["ARG"], 1), (OP["MUL"], 0), (OP["ROUND32"], 0)]
    assert ser(lambda a: fn.tan(a), np.float32)[0] == [(OP["ARG"], 1), (OP["TAN"], 0)]  # a Float32 call: nothing to round


def test_round32_follows_wide_integer_arguments_of_narrow_operations():
    """+ - * / min max convert their arguments to the promoted type before they operate: an Int32 / UInt32 / Int64 / UInt64 argument of a
    Float32 / ComplexF32 operation is rounded right behind the argument (Float32[1] .+ Int32[16777217] is 16777216), a weak integer
    literal that Float32 does not hold is folded on the host.  Integers that Float32 holds (8 and 16 bits, Bool) and programs without such
    arguments serialise as before."""
    R, ARG, CONST = (OP["ROUND32"], 0), OP["ARG"], OP["CONST"]
    for op, f in (("ADD", lambda a, b: a + b), ("SUB", lambda a, b: a - b), ("MUL", lambda a, b: a * b), ("DIV", lambda a, b: a / b),
                  ("MIN", lambda a, b: fn.min(a, b)), ("MAX", lambda a, b: fn.max(a, b))):
        for it in (np.int32, np.uint32, np.int64, np.uint64):
            assert ser(f, np.float32, it)[0] == [(ARG, 1), (ARG, 2), R, (OP[op], 0), R], (op, it)
            assert ser(f, it, np.float32)[0] == [(ARG, 1), R, (ARG, 2), (OP[op], 0), R], (op, it)
        for it in (np.int8, np.uint8, np.int16, np.uint16, np.bool_):
            assert ser(f, np.float32, it)[0] == [(ARG, 1), (ARG, 2), (OP[op], 0), R], (op, it)
        assert ser(f, np.float64, np.int32)[0] == [(ARG, 1), (ARG, 2), (OP[op], 0)]      # a Float64 operation: Float64 holds every Int32
    assert ser(lambda z, i: z * i, np.complex64, np.int32)[0] == [(ARG, 1), (ARG, 2), R, (OP["MUL"], 0), R]
    # an integer-typed sub-expression as the argument: the Int32 sum is converted, its own arguments are not
    assert ser(lambda i, j, a: (i + j) * a, np.int32, np.int32, np.float32)[0] == [(ARG, 1), (ARG, 2), (OP["ADD"], 0), R, (ARG, 3), (OP["MUL"], 0), R]
    # an n-ary fold is typed step by step like Julia's +(a, b, c) = (a + b) + c: the Int32 sum is converted, not its terms; a Float32 step
    # in front of a Float64 one is rounded; folds of one type serialise as before
    assert ser(lambda i, j, a: fn.add(i, j, a), np.int32, np.int32, np.float32)[0] == [(ARG, 1), (ARG, 2), (OP["ADD"], 0), R, (ARG, 3), (OP["ADD"], 0), R]
    assert ser(lambda a, b, c: fn.add(a, b, c), np.float32, np.float32, np.float64)[0] == [(ARG, 1), (ARG, 2), (OP["ADD"], 0), R, (ARG, 3), (OP["ADD"], 0)]
    assert ser(lambda a, b, c, d: fn.max(a, b, c, d), *[np.float32] * 4, wide=True)[0][:-1] == \
        [(ARG, 1), (ARG, 2), (OP["MAX"], 0), R, (ARG, 3), (OP["MAX"], 0), R, (ARG, 4), (OP["MAX"], 0), R]
    assert ser(lambda a, b, c: fn.mul(a, b, c), *[np.float64] * 3)[0] == [(ARG, 1), (ARG, 2), (OP["MUL"], 0), (ARG, 3), (OP["MUL"], 0)]
    # comparisons are mathematical, sqrt of an integer is a Float64: nothing is rounded
    assert ser(lambda a, i: a < i, np.float32, np.int32)[0] == [(ARG, 1), (ARG, 2), (OP["LT"], 0)]
    assert ser(lambda i, a: fn.sqrt(i) * a, np.int32, np.float32)[0] == [(ARG, 1), (OP["SQRT"], 0), (ARG, 2), (OP["MUL"], 0)]
    # a weak integer literal above 2^24 beside a Float32 array in a wide call: folded to Float32(16777217) = 16777216
    c, k = ser(lambda a: a + 16777217, np.float32, wide=True)
    W_ = (OP["WIDEN"], 0)   # (only Float32 operands: the wide class is announced at the end)
    assert c == [(ARG, 1), (CONST, 0), (OP["ADD"], 0), R, W_] and k == [16777216.0]
    c, k = ser(lambda a: 16777219 * a, np.float32, wide=True)
    assert c == [(CONST, 0), (ARG, 1), (OP["MUL"], 0), R, W_] and k == [16777220.0]
    c, k = ser(lambda a: a + np.int32(16777217), np.float32)
    assert c == [(ARG, 1), (CONST, 0), (OP["ADD"], 0), R, W_] and k == [16777216.0]
    # ... a literal that Float32 holds, a Float64 operation and a Float32 call keep their bytes
    assert ser(lambda a: a + 16777216, np.float32, wide=True) == ([(ARG, 1), (CONST, 0), (OP["ADD"], 0), R, W_], [16777216.0])
    assert ser(lambda a: a + 16777217, np.float64) == ([(ARG, 1), (CONST, 0), (OP["ADD"], 0)], [16777217.0])
    assert ser(lambda a: a + 16777217, np.float32, wide=False) == ([(ARG, 1), (CONST, 0), (OP["ADD"], 0)], [16777217.0])   # the Float32 class converts it
    assert ser(lambda a: a < 16777217, np.float32, wide=True)[1] == [16777217.0]
    # typing of the arithmetic operators follows Julia's promote_type, not NumPy's result_type
    for f, ts, want in ((lambda a, b: a + b, (np.float32, np.int32), np.float32), (lambda a, b: a / b, (np.float32, np.int64), np.float32),
                        (lambda a, b: a * b, (np.complex64, np.int32), np.complex64), (lambda a, b: a + b, (np.int32, np.uint32), np.uint32),
                        (lambda a, b: a + b, (np.int8, np.uint8), np.uint8), (lambda a, b: a + b, (np.int64, np.uint64), np.uint64),
                        (lambda a, b: a / b, (np.int32, np.int16), np.float64), (lambda a, b: fn.max(a, b), (np.int16, np.uint16), np.uint16)):
        assert E.result_dtype(E.trace(f, 2), [np.dtype(t) for t in ts]) == np.dtype(want), ts
    # the shim carries the same rule
    assert "roundarg!(p, f, length(p.code), Ta, Tn); roundarg!(p, f, at, T, Tn)" in JL and "Ta in (Int32, UInt32, Int64, UInt64)" in JL


# ---- typing (expected types: what Julia infers for the expression beside each row) ------------------------------------------------
f32, f64, c64, c128 = np.float32, np.float64, np.complex64, np.complex128
i8, i16, i32, i64, u8, u16, b = np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.bool_
TYPING = [
    (lambda a: fn.tan(a), [f32], f32),                 # tan.(A32)                 Float32
    (lambda a: fn.log10(a), [i32], f64),               # log10.(I32)               Float64
    (lambda a: fn.cbrt(a), [f64], f64),                # cbrt.(A64)                Float64
    (lambda a, c: fn.atan(a, c), [f32, f64], f64),     # atan.(A32, B64)           Float64
    (lambda a, c: fn.hypot(a, c), [i16, i16], f64),    # hypot.(I16, I16)          Float64
    (lambda a: fn.floor(a), [f32], f32),               # floor.(A32)               Float32
    (lambda a: fn.round(a), [i16], i16),               # round.(I16)               Int16
    (lambda a: fn.sign(a), [c64], c64),                # sign.(Z32)                ComplexF32
    (lambda a: fn.sign(a), [b], b),                    # sign.(M)                  Bool
    (lambda a: a ** 2, [f32], f32),                    # A32 .^ 2                  Float32
    (lambda a: a ** 3, [i32], i32),                    # I32 .^ 3                  Int32
    (lambda a: a ** -1, [i32], f64),                   # I32 .^ -1 (inv)           Float64
    (lambda a: a ** 2.0, [f32], f64),                  # A32 .^ 2.0                Float64
    (lambda a: a ** np.float32(0.5), [f32], f32),      # A32 .^ 0.5f0              Float32
    (lambda a, c: a ** c, [f32, i32], f32),            # A32 .^ I32                Float32
    (lambda a, c: a ** c, [f32, f64], f64),            # A32 .^ B64                Float64
    (lambda a: a ** 2, [c64], c64),                    # Z32 .^ 2                  ComplexF32
    (lambda a: a % 7, [i16], i64),                     # mod.(I16, 7)              Int64
    (lambda a: fn.rem(a, 7), [f32], f32),              # rem.(A32, 7)              Float32
    (lambda a, c: fn.mod(a, c), [i8, u16], u16),       # mod.(I8, U16)             UInt16
    (lambda a, c: a & c, [i8, u16], u16),              # I8 .& U16                 UInt16
    (lambda a, c: a | c, [u8, i16], i16),              # U8 .| I16                 Int16
    (lambda a, c: a ^ c, [b, b], b),                   # xor.(M, N)                Bool
    (lambda a, c: a & c, [b, i32], i32),               # M .& I32                  Int32
    (lambda a: ~a, [u8], u8),                          # .~U8                      UInt8
    (lambda a: ~a, [b], b),                            # .!M                       Bool
    (lambda a, c, d: fn.fma(a, c, d), [f32, f32, f64], f64),  # fma.(A32, B32, C64)   Float64
    (lambda a, c, d: fn.muladd(a, c, d), [i32, i32, i64], i64),  # muladd.(I32, J32, K64)  Int64
    (lambda a, c, d: fn.fma(a, c, d), [c64, c64, c64], c64),     # muladd.(Z, W, V)   ComplexF32
    (lambda a: fn.exp2(a), [c128], c128),              # exp2.(Z64)                ComplexF64
]


@pytest.mark.parametrize("i", range(len(TYPING)))
def test_result_types_follow_julia(i):
    f, dts, want = TYPING[i]
    assert E.result_dtype(E.trace(f, len(dts)), dts) == np.dtype(want)


def test_refusals_follow_julia():
    for f, dts in [(lambda a, c: a & c, [f32, f32]), (lambda a: ~a, [f64]), (lambda a: fn.floor(a), [c64]),
                   (lambda a: fn.cbrt(a), [c128]), (lambda a, c: fn.hypot(a, c), [c64, c64]), (lambda a: a % 3, [c64]),
                   (lambda a, c: fn.atan(a, c), [c128, c128]), (lambda a, c: a | c, [c64, i32])]:
        with pytest.raises(TypeError):  # MethodError in Julia
            E.result_dtype(E.trace(f, len(dts)), dts)
    for f, dts in [(lambda a: fn.tan(a), [c64]), (lambda a: fn.asin(a), [c128]), (lambda a: fn.expm1(a), [c64]),
                   (lambda a: fn.log1p(a), [c128]), (lambda a: a ** 2.5, [c64]), (lambda a, c: a ** c, [c128, f64])]:
        with pytest.raises(L.UnsupportedOnDevice):  # defined in Julia, not on the device
            E.result_dtype(E.trace(f, len(dts)), dts)
    E.result_dtype(E.trace(lambda a: a ** -3, 1), [c64])  # a complex literal power is fine


def test_scalar_fallbacks():
    assert fn.floor(2.5) == 2.0 and fn.round(2.5) == 2.0 and fn.round(3.5) == 4.0 and fn.sign(-0.0) == 0.0
    assert fn.rem(-7, 3) == -1 and fn.mod(-7, 3) == 2 and fn.atan(1.0, 1.0) == pytest.approx(np.pi / 4)
    assert fn.fma(2.0, 3.0, 1.0) == 7.0 and fn.and_(6, 3) == 2 and fn.xor(6, 3) == 5 and fn.not_(True) is False


# ---- the planner: integer class, refusals, malformed programs ------------------------------------------------------------------------
def _problem(code, consts, dtypes, dims=(16,)):
    bufs = [np.zeros(dims, dtype=d) for d in dtypes]
    p = L.smr_problem()
    p.N, p.M = len(dims), len(dtypes)
    for i, d in enumerate(dims):
        p.dims[i] = d
    for k, (a, d) in enumerate(zip(bufs, dtypes)):
        p.ops[k].base = a.ctypes.data
        p.ops[k].strides[0] = 1
        p.ops[k].dtype = S.stridedview.smr_dtype(np.dtype(d))
    cb = (C.c_uint8 * max(1, len(code)))(*code)
    kb = (C.c_double * max(2, 2 * len(consts)))(*[x for v in consts for x in (float(v), 0.0)])
    p.fprog, p.fprog_len = C.cast(cb, C.POINTER(C.c_uint8)), len(code) // 2
    p.fconsts, p.nconsts = C.cast(kb, C.POINTER(C.c_double)), len(consts)
    return p, (bufs, cb, kb)


def canon(code, consts, dtypes):
    """(program pairs, wraps added, compute class) of the canonicalised problem, or the (negative) status"""
    p, keep = _problem(code, consts, dtypes)
    buf = (C.c_uint8 * (2 * L.SMR_MAXPROG))()
    nw, ct = C.c_int(0), C.c_int(0)
    n = L.load().smr_debug_canon_prog(C.byref(p), buf, len(buf), C.byref(nw), C.byref(ct), None)
    if n < 0:
        return n
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)], nw.value, ct.value


def flat(*pairs):
    return [x for pr in pairs for x in pr]


A1, A2, K0 = (OP["ARG"], 1), (OP["ARG"], 2), (OP["CONST"], 0)
I64 = S.stridedview.smr_dtype(np.dtype(np.int64))


def wrap(v, bits, sgn):
    v &= (1 << bits) - 1
    return v - (1 << bits) if sgn and v >> (bits - 1) else v


def test_integer_class_types_the_math_opcodes():
    # Int32 a^3 into Int64: the cube wraps at 32 bits in Julia -> one WRAP_I32 after the POWI
    prog, nw, ct = canon(flat(A1, (OP["POWI"], 3)), [], [np.int64, np.int32])
    assert ct == I64 and nw == 1 and prog == [A1, (OP["POWI"], 3), (OP["WRAP_I32"], 0)]
    for a in (7, -1291, 46341, -2 ** 31):
        assert wrap(wrap(a ** 3, 64, True), 32, True) == wrap(a ** 3, 32, True)  # what the device computes == Julia
    # ... into an Int32 destination the store truncates: no wrap needed
    prog, nw, ct = canon(flat(A1, (OP["POWI"], 3)), [], [np.int32, np.int32])
    assert ct == I64 and nw == 0
    # Int8 a & UInt16 b is a UInt16 (Julia promotion): exact into UInt16, one WRAP_U16 into Int64
    prog, nw, ct = canon(flat(A1, A2, (OP["AND"], 0)), [], [np.uint16, np.int8, np.uint16])
    assert ct == I64 and nw == 0
    prog, nw, ct = canon(flat(A1, A2, (OP["ADD"], 0), A2, (OP["AND"], 0)), [], [np.int64, np.int8, np.uint16])
    assert ct == I64 and prog[-1] == (OP["WRAP_U16"], 0)
    for a, c in ((-1, 0xFFFF), (-128, 0x8001), (127, 40000)):  # device: 64-bit sum & b then WRAP_U16; Julia: UInt16 arithmetic
        assert wrap(wrap(a + c, 64, True) & c, 16, False) == (((a + c) & 0xFFFF) & c)
    # Int16 mod(a, 7) stays in the integer class (the result is an Int64: no wrap)
    prog, nw, ct = canon(flat(A1, K0, (OP["MOD"], 0)), [7], [np.int64, np.int16])
    assert ct == I64 and nw == 0
    # Bool & Bool is a Bool; ~ on Int32 into Int64 is exact (signed); on UInt8 into Int64 wraps
    assert canon(flat(A1, A2, (OP["AND"], 0)), [], [np.bool_, np.bool_, np.bool_])[2] == I64
    prog, nw, _ = canon(flat(A1, (OP["NOT"], 0)), [], [np.int64, np.uint8])
    assert prog == [A1, (OP["NOT"], 0), (OP["WRAP_U8"], 0)]
    prog, nw, _ = canon(flat(A1, A2, A1, (OP["FMA"], 0)), [], [np.int64, np.int32, np.int64])
    assert nw == 0 and prog[-1] == (OP["FMA"], 0)
    for op in ("FLOOR", "CEIL", "TRUNC", "ROUND", "SIGN"):
        assert canon(flat(A1, (OP[op], 0)), [], [np.int32, np.int32])[2] == I64, op
    # transcendentals and pow leave the integers (Float64, like sqrt)
    assert canon(flat(A1, (OP["TAN"], 0)), [], [np.float64, np.int32])[2] == S.stridedview.smr_dtype(np.dtype(np.float64))
    assert canon(flat(A1, A2, (OP["POW"], 0)), [], [np.int32, np.int32, np.int32])[2] != I64


def test_integer_refusals():
    E_UN = L.SMR_EUNSUPPORTED
    assert canon(flat(A1, A2, (OP["MOD"], 0)), [], [np.int32, np.int32, np.int32]) == E_UN   # array divisor
    assert canon(flat(A1, K0, (OP["REM"], 0)), [0], [np.int32, np.int32]) == E_UN            # rem(a, 0): DivideError
    assert canon(flat(A1, (OP["SIGN"], 0)), [], [np.uint64, np.uint64]) == E_UN              # needs order on UInt64
    assert canon(flat(A1, (OP["POWI"], 0xFF)), [], [np.int32, np.int32]) == E_UN             # a ^ -1: DomainError
    assert canon(flat(A1, K0, (OP["REM"], 0)), [-1], [np.int64, np.int64])[2] == I64          # rem(typemin, -1) = 0 (device: no UB)


def test_malformed_math_programs_are_einval():
    E_IN = L.SMR_EINVAL
    for code in (flat((OP["POWI"], 2)), flat(A1, (OP["POW"], 0)), flat(A1, A1, (OP["FMA"], 0)), flat(A1, A1, (OP["HYPOT"], 0), (OP["TAN"], 0), A1),
                 flat(A1, (115, 0)), flat(A1, A1, (136, 0)), flat(A1, A1, A1, (66, 0)), flat(A1, (160, 0))):
        assert canon(code, [], [np.float64, np.float64]) == E_IN, code
    assert canon(flat(A1, (OP["WRAP_I32"], 0)), [], [np.int64, np.int32]) == E_IN  # still the library's own


def test_interpreter_refuses_math_opcodes():
    A = _v((64, 64))
    S.set_option("jit", 0)
    try:
        with pytest.raises(L.UnsupportedOnDevice):
            S.make_plan(lambda a: fn.tan(a), None, None, A.size, (A.similar(), A))
        with pytest.raises(L.UnsupportedOnDevice):
            S.make_plan(lambda a: a ** 2, None, None, A.size, (A.similar(), A))
        S.make_plan(lambda a: fn.sin(a), None, None, A.size, (A.similar(), A))  # the interpreter's own opcodes still plan
    finally:
        S.set_option("jit", 1)
    S.make_plan(lambda a: fn.tan(a), None, None, A.size, (A.similar(), A))


# ---- JIT source and compilation ---------------------------------------------------------------------------------------------------
def test_generated_source_uses_compile_time_constants():
    A, B, Cc = _v((64, 64)), _v((64, 64)), _v((64, 64))

    def src(f, *arrs):
        return S.make_plan(f, None, None, arrs[0].size, arrs).jit_source()

    assert "mathx<JT>::powi<2>(v0);" in src(lambda a: a ** 2, B, A)
    assert "mathx<JT>::powi<-3>(v0);" in src(lambda a: a ** -3, B, A)
    assert "mathx<JT>::fma3(v0, v1, v2);" in src(lambda a, c, d: fn.fma(a, c, d), B, A, Cc, B)
    s = src(lambda a, c: fn.hypot(fn.exp2(a), c) + fn.atan(a, c), B, A, Cc)
    assert "ext_un<103>(v0)" in s and "ext_bin<130>(v1, v2)" in s and "ext_bin<129>(v4, v5)" in s
    for name in MATH[2:]:
        code = OP[name]
        f = (lambda a, c: getattr(fn, "and_")(a, c)) if name == "AND" else None
        arrs = (B, A, Cc)
        prog = flat(A1, (code, 0)) if code < 128 else flat(A1, A2, (code, 0))
        p, keep = _problem(prog, [], [np.float64] * 3)
        pl = C.c_void_p()
        lib = L.load()
        assert lib.smr_plan_create(C.byref(p), C.byref(pl)) == 0, name
        buf = C.create_string_buffer(8192)
        assert lib.smr_plan_jit_source(pl, buf, len(buf)) == 0
        text = buf.value.decode()
        lib.smr_plan_destroy(pl)
        assert (f"ext_un<{code}>" if code < 128 else f"ext_bin<{code}>") in text, name
    # programs without a math opcode: the text (= the compiled-code cache key) is what it was
    s = src(lambda a, c: a * 2 + c / 3 - 1, B, A, Cc)
    assert "        const JT v2 = mathx<JT>::bin(34, v0, v1);\n" in s and "        const JT v5 = mathx<JT>::bin(35, v3, v4);\n" in s
    assert "truthy(v2) ? v3 : v4" in src(lambda a, c: fn.select(a < c, a, c), B, A, Cc)
    assert "ext_" not in s and "powi" not in s and "fma3" not in s


def _orbit(shape, dtype, perms):
    a = _v(shape, dtype)
    return (a.similar(),) + tuple(a.permutedims(q) for q in perms)


PROGS = {
    "powi": lambda a, c: a ** 3 * c + a ** -2,
    "fma": lambda a, c: fn.fma(a, c, a),
    "pow_atan2": lambda a, c: a ** c + fn.atan(a, c) + fn.sinh(a),
}


def _family_arrays(fam, dtype):
    if fam == "stream":
        return None, (_v((256, 256), dtype), _v((256, 256), dtype), _v((256, 256), dtype))
    if fam == "tiled":
        return None, (_v((256, 256), dtype), _v((256, 256), dtype).permutedims((1, 0)), _v((256, 256), dtype))
    if fam == "orbit":
        return None, _orbit((256, 256), dtype, [(0, 1), (1, 0)])
    if fam == "flat":
        x = _v((6, 5, 40000), dtype)  # short ragged leading dims of a transposing map (the same view twice: one input)
        return None, (_v((5, 6, 40000), dtype), x.permutedims((1, 0, 2)), x.permutedims((1, 0, 2)))
    if fam == "generic":
        return None, (_v((7, 9, 5), dtype), _v((5, 9, 7), dtype).permutedims((2, 1, 0)), _v((7, 9, 5), dtype))
    if fam == "reduce_all":
        x = _v((64, 64, 16), dtype)
        return "+", S.promoteshape(x.size, x.similar(size=(1,)).sreshape((1, 1, 1)), x, x)
    x = _v((32, 16, 32, 8), dtype)
    return "+", S.promoteshape(x.size, x.similar(size=(32, 1, 32, 1)), x, x)


# where the op exists: the integer class has x ^ n for n >= 0 only (its POWI is in "bits"), bit operations are integer-only
COMBOS = [(p, d) for p in sorted(PROGS) for d in (np.float32, np.float64, np.complex64, np.complex128)] + \
    [("fma", np.int64), ("bits", np.int64)]


@pytest.mark.parametrize("fam", ["stream", "tiled", "orbit", "flat", "generic", "reduce_all", "reduce_part"])
@pytest.mark.parametrize("prog,dtype", COMBOS)
def test_math_programs_compile_for_gfx950(fam, dtype, prog):
    cx, it = np.dtype(dtype).kind == "c", np.dtype(dtype).kind == "i"
    if prog == "bits":
        f = lambda a, c: ((a & c) ^ ~a | (c % 7)) + fn.sign(a) * a ** 2  # noqa: E731
    elif cx and prog == "pow_atan2":
        f = lambda a, c: a ** 5 * fn.sinh(c) + fn.log10(a) * fn.sign(c)  # noqa: E731  (complex: literal powers, the complex forms)
    else:
        f = PROGS[prog]
    op, arrays = _family_arrays(fam, dtype)
    if fam == "generic":
        S.set_option("force_family", 1)
    try:
        dims = arrays[1].size
        plan = S.make_plan(f, op, None, dims, arrays)
    finally:
        S.set_option("force_family", 0)
    d = plan.describe()
    assert f"family={fam}" in d, d
    assert ("ct=i64" in d) == it, d
    before = S.get_option("jit_failures")
    assert plan.jit_compile() > 1000, d
    assert S.get_option("jit_failures") == before
