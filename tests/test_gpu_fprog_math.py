"""The math opcodes on the MI355X: powers, fma / muladd, more of Base's math, rem / mod and the bitwise operations, in every compute
class, kernel family and reduction, against NumPy -- bit-exact where the operation is exact (rounding functions, x ^ n for
n in {0, 1, 2, -1}, rem / mod, fma against the correctly rounded exact result, bit operations), within the suite's tolerance
(sqrt(eps) relative, an absolute floor near zero) for the transcendentals.  That tolerance pins the plumbing (families, reductions,
mixed precision, dispatch paths), not the accuracy: each opcode's arithmetic is held to exact values, at the edges of its domain, by
test_gpu_fprog_conformance.py."""
from fractions import Fraction

import numpy as np
import pytest

import strided_jl_amd as S
from util import rtol

pytestmark = pytest.mark.gpu
fn = S.fn
F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128


def dview(arr):
    import torch
    a = np.asfortranarray(arr)
    t = torch.from_numpy(a.ravel(order="F").copy()).cuda()
    st, s = [], 1
    for d in a.shape:
        st.append(s)
        s *= d
    return S.StridedView(t, a.shape, tuple(st), 0)


def host(v):
    import torch
    torch.cuda.synchronize()
    return np.asarray(v.toarray())


def run(f, *arrays, dtype=None, shape=None):
    """dest .= f.(arrays...) on device copies; returns (host result, plan description)"""
    A = [dview(a) for a in arrays]
    T = np.dtype(dtype or arrays[0].dtype)
    D = dview(np.zeros(shape or arrays[0].shape, dtype=T))
    plan = S.make_plan(f, None, None, D.size, (D,) + tuple(A))
    plan.execute()
    return host(D), plan.describe()


def same(d, e):
    """bit-identical up to NaN payloads: NaN == NaN, -0.0 != 0.0"""
    d, e = np.ascontiguousarray(d), np.ascontiguousarray(e)
    assert d.dtype == e.dtype and d.shape == e.shape
    if d.tobytes() == e.tobytes():
        return True
    parts = (lambda x: (x.real, x.imag)) if d.dtype.kind == "c" else (lambda x: (x,))
    return all(np.array_equal(p, q, equal_nan=True) and np.array_equal(np.signbit(p), np.signbit(q)) for p, q in zip(parts(d), parts(e)))


def cmul(a, b):
    """the device's complex product (Julia's: four multiplications, no fma), evaluated with NumPy's real operations"""
    return (a.real * b.real - a.imag * b.imag) + 1j * (a.real * b.imag + a.imag * b.real)


def close(d, e, dtype):
    d, e = np.asarray(d).astype(np.complex128), np.asarray(e).astype(np.complex128)
    tol = rtol(np.finfo(np.dtype(dtype)).dtype)
    ok = np.abs(d - e) <= tol * np.maximum(np.abs(e), 1e-3)
    ok |= np.isnan(d) & np.isnan(e)
    ok |= (d == e)
    return bool(ok.all())


def rng_data(seed, shape, dtype, lo=-4.0, hi=4.0):
    r = np.random.default_rng(seed)
    x = r.uniform(lo, hi, shape)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * r.uniform(lo, hi, shape)
    return np.asfortranarray(x.astype(dtype))


SPECIAL = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.0, -0.0, np.inf, -np.inf, np.nan, 3.0, -7.25, 1e30, -1e-30]


def special_data(seed, n, dtype):
    x = rng_data(seed, (n,), dtype, -10, 10)
    x[: len(SPECIAL)] = np.array(SPECIAL, dtype=dtype)
    return x


# ---- bit-exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_rounding_and_sign_are_exact(dtype):
    x = special_data(1, 4099, dtype)
    sign = np.where((x == 0) | np.isnan(x), x, np.copysign(np.ones_like(x), x))
    for f, want in [(fn.floor, np.floor(x)), (fn.ceil, np.ceil(x)), (fn.trunc, np.trunc(x)), (fn.round, np.rint(x)), (fn.sign, sign)]:
        d, desc = run(f, x)
        assert "family=stream" in desc, desc
        assert same(d, want.astype(dtype)), f.__name__


@pytest.mark.parametrize("dtype", [F32, F64, C64, C128])
def test_small_literal_powers_are_exact(dtype):
    x = rng_data(2, (257, 33), dtype)
    one = np.ones_like(x)
    if np.dtype(dtype).kind == "c":  # the device's complex inverse: Smith's division (smr_device.h), evaluated the same way here
        re, im = x.real, x.imag
        big = np.abs(re) >= np.abs(im)
        r1 = np.where(big, im / re, re / im)
        den = np.where(big, re + im * r1, re * r1 + im)
        inv = np.where(big, 1 / den, r1 / den) + 1j * np.where(big, -r1 / den, -1 / den)
        inv = inv.astype(dtype)
    else:
        inv = (one / x).astype(dtype)
    mul = cmul if np.dtype(dtype).kind == "c" else (lambda a, b: a * b)
    cases = [(lambda a: a ** 0, one), (lambda a: a ** 1, x), (lambda a: a ** 2, mul(x, x)), (lambda a: a ** -1, inv),
             (lambda a: a ** 3, mul(mul(x, x), x)), (lambda a: a ** -2, mul(inv, inv))]
    for f, want in cases:
        d, _ = run(f, x)
        assert same(d, np.asarray(want, dtype=dtype)), (dtype, f)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_rem_and_mod_are_exact(dtype):
    a = rng_data(3, (4096,), dtype, -100, 100)
    b = rng_data(4, (4096,), dtype, -9, 9)
    b[b == 0] = 1
    d, _ = run(lambda x, y: fn.rem(x, y), a, b)
    assert same(d, np.fmod(a, b))
    d, _ = run(lambda x, y: x % y, a, b)
    assert same(d, np.mod(a, b))
    d, _ = run(lambda x: fn.mod(x, 7), a)
    assert same(d, np.mod(a, dtype(7)))


def _round_to(q: Fraction, dtype):
    """correctly rounded (ties to even) value of the rational q in dtype"""
    x = np.asarray(float(q), dtype=np.float64).astype(dtype)  # within one ulp of dtype
    best = x
    for c in (np.nextafter(x, dtype(-np.inf)), np.nextafter(x, dtype(np.inf))):
        if not np.isfinite(c):
            continue
        dc, db = abs(Fraction(float(c)) - q), abs(Fraction(float(best)) - q)
        if dc < db or (dc == db and int(c.view(np.uint32 if dtype == F32 else np.uint64)) % 2 == 0):
            best = c
    return best


@pytest.mark.parametrize("dtype", [F32, F64])
def test_fma_is_fused(dtype):
    n = 2048
    a, b = rng_data(5, (n,), dtype, -3, 3), rng_data(6, (n,), dtype, -3, 3)
    c = rng_data(7, (n,), dtype, -3, 3)
    c[: n // 2] = -(a[: n // 2] * b[: n // 2])  # cancellation: a*b + c is the rounding error of the product, which only fma keeps
    want = np.array([_round_to(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)), dtype) for x, y, z in zip(a, b, c)],
                    dtype=dtype)
    assert np.count_nonzero(want[: n // 2]) > n // 8
    for f in (fn.fma, fn.muladd):
        d, _ = run(lambda x, y, z: f(x, y, z), a, b, c)
        assert same(d, want), f.__name__


def test_bit_operations_are_exact():
    r = np.random.default_rng(8)
    for dt in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64):
        info = np.iinfo(dt)
        a = r.integers(info.min, info.max, 3001, dtype=dt, endpoint=True)
        b = r.integers(info.min, info.max, 3001, dtype=dt, endpoint=True)
        for f, want in [(lambda x, y: x & y, a & b), (lambda x, y: x | y, a | b), (lambda x, y: x ^ y, a ^ b)]:
            d, desc = run(f, a, b)
            assert "ct=i64" in desc and np.array_equal(d, want), (dt, desc)
        d, _ = run(lambda x: ~x, a)
        assert np.array_equal(d, ~a), dt


# ---- within tolerance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_transcendentals(dtype):
    x = rng_data(9, (64, 65), dtype, -3, 3)
    u = rng_data(10, (64, 65), dtype, -0.99, 0.99)
    p = rng_data(11, (64, 65), dtype, 0.01, 20)
    y = rng_data(12, (64, 65), dtype, -3, 3)
    cases = [(fn.tan, u, np.tan), (fn.asin, u, np.arcsin), (fn.acos, u, np.arccos), (fn.atan, x, np.arctan), (fn.sinh, x, np.sinh),
             (fn.cosh, x, np.cosh), (fn.exp2, x, np.exp2), (fn.expm1, u, np.expm1), (fn.log2, p, np.log2), (fn.log10, p, np.log10),
             (fn.log1p, p, np.log1p), (fn.cbrt, x, np.cbrt)]
    for f, a, g in cases:
        d, _ = run(f, a)
        assert close(d, g(a.astype(F64)).astype(dtype), dtype), f.__name__
    for f, g in [(lambda a, b: a ** b, lambda a, b: np.power(a, b)), (fn.hypot, np.hypot), (lambda a, b: fn.atan(a, b), np.arctan2)]:
        d, _ = run(f, p, y)
        assert close(d, g(p.astype(F64), y.astype(F64)).astype(dtype), dtype)
    q = rng_data(13, (64, 65), dtype, 0.5, 1.5)
    for n in (5, 7, -3, -5, 17, 127, -128):
        d, _ = run(lambda a, n=n: a ** n, q)
        assert close(d, np.power(q.astype(F64), float(n)).astype(dtype), dtype), n


# ---- kernel families ----------------------------------------------------------------------------------------------------------
PERMS = [(0, 1, 2, 3), (1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2)]


def test_families():
    a = rng_data(13, (300, 200), F32)
    A = dview(a)
    B = dview(np.zeros((200, 300), F32))
    p = S.make_plan(lambda x: x ** 2 + fn.floor(x), None, None, B.size, (B, A.permutedims((1, 0))))
    p.execute()
    assert "family=tiled" in p.describe(), p.describe()
    assert same(host(B), (a.T * a.T + np.floor(a.T)).astype(F32))
    # ORBIT: permuted views of ONE buffer, a 4-way fma / POWI
    q = rng_data(14, (32,) * 4, F64)
    Q = dview(q)
    C = dview(np.zeros_like(q))
    p = S.make_plan(lambda w, x, y, z: fn.fma(w, x, y) + z ** 3, None, None, Q.size, (C,) + tuple(Q.permutedims(pp) for pp in PERMS))
    p.execute()
    assert "family=orbit" in p.describe(), p.describe()
    t = [np.transpose(q, pp).ravel() for pp in PERMS]
    got = host(C).ravel()
    idx = np.random.default_rng(0).choice(got.size, 3000, replace=False)  # the exact fma on a sample of the 2^20 elements
    want = np.array([_round_to(Fraction(float(t[0][i])) * Fraction(float(t[1][i])) + Fraction(float(t[2][i])), F64) for i in idx])
    assert same(got[idx], want + t[3][idx] * t[3][idx] * t[3][idx])
    # FLAT: a transposing map with short ragged leading dims
    r = rng_data(15, (6, 5, 40000), F64)
    R = dview(r)
    D = dview(np.zeros((5, 6, 40000)))
    p = S.make_plan(lambda x: fn.round(x) ** 2 - fn.sign(x), None, None, D.size, (D, R.permutedims((1, 0, 2))))
    p.execute()
    assert "family=flat" in p.describe(), p.describe()
    rt = np.transpose(r, (1, 0, 2))
    assert same(host(D), np.rint(rt) * np.rint(rt) - np.sign(rt))


# ---- reductions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_reductions(dtype):
    a = rng_data(16, (96, 70, 9), dtype, -2, 2)
    A = dview(a)
    a64 = a.astype(F64)
    tot = S.mapreduce(lambda x: abs(x) ** 3, "+", A)
    assert close(tot, np.sum(np.abs(a64) ** 3), dtype)
    part = S.mapreduce(lambda x: abs(x) ** 3, "+", A, dims=(0, 2))
    assert close(host(part), np.sum(np.abs(a64) ** 3, axis=(0, 2), keepdims=True), dtype)
    pn = S.mapreduce(lambda x: abs(x) ** 2.5, "+", A)  # a p-norm with a Float64 p: POW
    assert close(pn, np.sum(np.abs(a64) ** 2.5), F64)


def test_sum_of_squares_equals_sum_abs2():
    a = rng_data(17, (512, 300), F64)
    A = dview(a)
    s1 = S.mapreduce(lambda x: x ** 2, "+", A)
    s2 = S.mapreduce(fn.abs2, "+", A)
    assert s1 == s2
    d1 = host(S.mapreduce(lambda x: x ** 2, "+", A, dims=(1,)))
    d2 = host(S.mapreduce(fn.abs2, "+", A, dims=(1,)))
    assert same(d1, d2)


# ---- mixed precision ----------------------------------------------------------------------------------------------------------
def test_mixed_precision():
    a = rng_data(18, (1000,), F32, 0, 9)
    d, desc = run(lambda x: x ** 0.5, a, dtype=F32)  # Float32 .^ 0.5 (a Float64 literal): computed in Float64, stored as Float32
    assert "f64" in desc and close(d, np.sqrt(a.astype(F64)), F32), desc
    b, c = rng_data(19, (1000,), F32), rng_data(20, (1000,), F64)
    d, _ = run(lambda x, y, z: fn.fma(x, y, z), a, b, c, dtype=F64)
    want = np.array([_round_to(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)), F64) for x, y, z in zip(a, b, c)])
    assert same(d, want)
    # A32 ** 2 + B64: the Float32 square is rounded to Float32 first (ROUND32), as Julia computes it (bit-exact for n = 2: the
    # product is exact in Float64); n = 3 in a mixed call is within 1 ulp of Julia's Float32 x*x*x
    d, _ = run(lambda x, y: x ** 2 + y, a, c, dtype=F64)
    assert same(d, (a * a).astype(F64) + c)
    d, _ = run(lambda x, y: x ** 3 + y, a, c, dtype=F64)
    assert close(d, (a * a * a).astype(F64) + c, F32)


# ---- integer class ------------------------------------------------------------------------------------------------------------
def test_integer_class():
    r = np.random.default_rng(21)
    a = r.integers(-2 ** 31, 2 ** 31, 5000, dtype=np.int32)
    d, desc = run(lambda x: x ** 3, a)
    assert "ct=i64" in desc and np.array_equal(d, a ** 3)  # wraps like Int32 / NumPy int32
    d, _ = run(lambda x: x ** 3, a, dtype=np.int64)  # into Int64: the Int32 cube still wraps at 32 bits (WRAP_I32)
    assert np.array_equal(d, (a ** 3).astype(np.int64))
    h = r.integers(-2 ** 15, 2 ** 15, 5000, dtype=np.int16)
    d, desc = run(lambda x: x % 7, h, dtype=np.int64)
    assert "ct=i64" in desc and np.array_equal(d, np.mod(h.astype(np.int64), 7))
    d, _ = run(lambda x: fn.rem(x, -7), h, dtype=np.int64)
    assert np.array_equal(d, np.fmod(h.astype(np.int64), -7))
    u = r.integers(0, 256, 5000, dtype=np.uint8)
    d, _ = run(lambda x: ~x, u)
    assert np.array_equal(d, ~u)
    x, y = rng_data(22, (5000,), F64), rng_data(23, (5000,), F64, -1, 3)
    d, _ = run(lambda p, q: (p > 0) & (q < 1), x, y, dtype=np.bool_)
    assert np.array_equal(d, (x > 0) & (y < 1))
    m = (x > 0)
    d, _ = run(lambda p: ~p, m)
    assert d.dtype == np.bool_ and np.array_equal(d, ~m)


# ---- complex class ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [C64, C128])
def test_complex_class(dtype):
    z, w, v = rng_data(24, (3000,), dtype, -2, 2), rng_data(25, (3000,), dtype, -2, 2), rng_data(26, (3000,), dtype, -2, 2)
    z128, w128, v128 = z.astype(C128), w.astype(C128), v.astype(C128)
    d, _ = run(lambda a: a ** 2, z)
    assert same(d, cmul(z, z).astype(dtype))
    d, _ = run(lambda a: a ** -3, z)
    assert close(d, z128 ** -3, dtype)
    d, _ = run(lambda a, b, c: fn.fma(a, b, c), z, w, v)
    assert close(d, z128 * w128 + v128, dtype)
    for f, g in [(fn.sinh, np.sinh), (fn.log10, np.log10), (fn.cosh, np.cosh), (fn.log2, np.log2), (fn.exp2, np.exp2)]:
        d, _ = run(f, z)
        assert close(d, g(z128), dtype), f.__name__
    zz = z.copy()
    zz[:3] = 0
    d, _ = run(fn.sign, zz)
    want = np.where(zz == 0, 0, zz.astype(C128) / np.abs(zz.astype(C128)))
    assert close(d, want, dtype) and np.all(d[:3] == 0)


# ---- dispatch paths -----------------------------------------------------------------------------------------------------------
def test_library_stream_and_sequence_replay():
    import torch
    a = rng_data(27, (128, 96), F64, 0.1, 4)
    A = dview(a)
    B = dview(np.zeros_like(a))
    st = S.Stream()
    with st:
        S.map_(lambda x: fn.hypot(x, 3.0) + x ** 2, B, A)
        out = B.toarray()
    st.close()
    assert close(out, np.hypot(a, 3.0) + a * a, F64)
    C = dview(np.zeros_like(a))
    p = S.make_plan(lambda x: fn.fma(x, x, -x) + fn.log2(x), None, None, A.size, (C, A))
    torch.cuda.synchronize()
    q = S.Sequence().add(p)
    q.run(2, int(torch.cuda.current_stream().cuda_stream))
    q.wait()
    assert close(host(C), a * a - a + np.log2(a), F64)
