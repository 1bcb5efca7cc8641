#!/usr/bin/env python3
"""Generates tests/golden/fprog_golden.npz: the stored inputs and the exact results of every inexact row of tests/fprog_cases.py,
computed with mpmath at 320 bits.  CPU only; the tests read the .npz and never import mpmath unconditionally.

    python tests/golden/make_fprog_golden.py            # rewrites the .npz, byte for byte the same on every run
    python tests/golden/make_fprog_golden.py --check    # regenerates in memory and compares with the committed file

Real rows (Float32, Float64), per point: the inputs, `lo` = the largest value of the type that is <= the exact result, one bit
`ex` saying that lo IS the exact result (the upper neighbour is then lo itself, else nextafter(lo, +Inf)), one bit `sp` marking the
special-value points (+-0, +-Inf, NaN, out-of-domain arguments: lo holds what Julia's Base returns, NaN where Julia throws
DomainError; taken from NumPy's Float64 functions, which follow C Annex F like Base, with the rows where Julia is the authority
asserted from tests/fprog_cases.JULIA_AUTHORITY).
Complex rows (ComplexF32, ComplexF64), per point: the inputs, `hi` = the exact result rounded to the nearest value of the row's own
type (complex64 / complex128), `lo8` = the rest of each part in 1/254 of the spacing of the type at that part (int8: a rest of
exactly half a spacing is +-127; hi + lo8 together carry 8 more bits than the type, 32 resp. 61 in all), bits `edge` (a point at the
ends of the range, judged like the others), `axis` (imaginary part +-0: each part is also judged on its own) and `sre` / `sim` (the
sign of an exact zero part
there, from C Annex G, which mpmath cannot give)."""
import io
import math
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import fprog_cases as FC  # noqa: E402

mp.mp.prec = 320
OUT = os.path.join(HERE, "fprog_golden.npz")
F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
N_REAL, N_POWI, N_CPLX = FC.NMAX, 64, 72
PI = mp.pi


# ---- exact functions (arguments: Python floats) -------------------------------------------------------------------------------
def _m(x):
    return mp.mpf(x)


def _atan2(y, x):
    return math.copysign(1.0, y) * mp.atan2(abs(_m(y)), _m(x))


def _cbrt(x):
    return mp.sign(_m(x)) * mp.cbrt(abs(_m(x)))


def _powr(x, y):
    return mp.power(_m(x), _m(y))


MPF = {"exp": lambda x: mp.exp(_m(x)), "log": lambda x: mp.log(_m(x)), "sin": lambda x: mp.sin(_m(x)), "cos": lambda x: mp.cos(_m(x)),
       "tanh": lambda x: mp.tanh(_m(x)), "tan": lambda x: mp.tan(_m(x)), "asin": lambda x: mp.asin(_m(x)), "acos": lambda x: mp.acos(_m(x)),
       "atan": lambda x: mp.atan(_m(x)), "sinh": lambda x: mp.sinh(_m(x)), "cosh": lambda x: mp.cosh(_m(x)),
       "exp2": lambda x: mp.power(2, _m(x)), "expm1": lambda x: mp.expm1(_m(x)), "log2": lambda x: mp.log(_m(x)) / mp.log(2),
       "log10": lambda x: mp.log10(_m(x)), "log1p": lambda x: mp.log1p(_m(x)), "cbrt": _cbrt, "pow": _powr, "atan2": _atan2,
       "hypot": lambda x, y: mp.hypot(_m(x), _m(y))}
for _n in FC.POWI_N:
    MPF["powi%d" % _n] = (lambda n: lambda x: _m(x) ** n)(_n)


def _c(z):
    return mp.mpc(z.real, z.imag)


MPC = {"cabs": lambda z: mp.mpc(abs(_c(z)), 0), "csqrt": lambda z: mp.sqrt(_c(z)), "cexp": lambda z: mp.exp(_c(z)), "clog": lambda z: mp.log(_c(z)),
       "csin": lambda z: mp.sin(_c(z)), "ccos": lambda z: mp.cos(_c(z)), "ctanh": lambda z: mp.tanh(_c(z)), "cinv": lambda z: 1 / _c(z),
       "cmul": lambda a, b: _c(a) * _c(b), "cdiv": lambda a, b: _c(a) / _c(b), "csinh": lambda z: mp.sinh(_c(z)),
       "ccosh": lambda z: mp.cosh(_c(z)), "cexp2": lambda z: mp.exp(_c(z) * mp.log(2)), "clog2": lambda z: mp.log(_c(z)) / mp.log(2),
       "clog10": lambda z: mp.log(_c(z)) / mp.log(10), "csign": lambda z: _c(z) / abs(_c(z)), "cpowi5": lambda z: _c(z) ** 5,
       "cpowi-3": lambda z: 1 / _c(z) ** 3, "cfma": lambda a, b, c: _c(a) * _c(b) + _c(c)}


# ---- bracketing -----------------------------------------------------------------------------------------------------------------
def bracket(v, R):
    """(lo, exact): the largest value of R that is <= the real number v, and whether it equals v"""
    fi = np.finfo(R)
    if mp.isinf(v):
        return R(np.inf if v > 0 else -np.inf), True
    big = _m(float(fi.max))
    if v > big:
        return R(fi.max), False
    if v < -big:
        return R(-np.inf), False
    with np.errstate(all="ignore"):
        c = R(float(v))
    if not np.isfinite(c):
        c = R(fi.max) if c > 0 else R(-fi.max)
    if c == 0:
        c = R(0.0)
    while _m(float(c)) > v:
        c = np.nextafter(c, R(-np.inf))
    while True:
        up = np.nextafter(c, R(np.inf))
        if np.isfinite(up) and _m(float(up)) <= v:
            c = up
        else:
            break
    return c, _m(float(c)) == v


def _trivial(y):
    """results that a special-value point is asked for exactly: NaN, zeros, infinities, integers"""
    return bool(np.isnan(y) or np.isinf(y) or y == np.trunc(y))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def lim(R):
    fi = np.finfo(R)
    return fi, fi.minexp - fi.nmant, fi.maxexp - 1


def rnd(rng, n, elo, ehi, signed=True):
    m = rng.uniform(1, 2, n)
    m = np.where(rng.random(n) < 0.5, np.round(m * 2.0 ** 20) / 2.0 ** 20, m)  # half of the mantissas are short: the file compresses
    x = np.ldexp(m, rng.integers(elo, ehi, n, endpoint=True))
    return x * rng.choice([-1.0, 1.0], n) if signed else x


def around(v, R, k=2):
    """the values of R nearest v and k steps either side"""
    with np.errstate(all="ignore"):
        c = R(v)
    out = [c]
    a = b = c
    for _ in range(k):
        a, b = np.nextafter(a, R(-np.inf)), np.nextafter(b, R(np.inf))
        out += [a, b]
    return [float(x) for x in out if np.isfinite(x)]


def sub_pts(R):
    fi = np.finfo(R)
    s = float(fi.smallest_subnormal)
    return [s, -s, 3 * s, -5 * s, float(fi.tiny) * 0.75, -float(fi.tiny) * 0.5, float(fi.tiny)]


COMMON_SPECIAL = [0.0, -0.0, np.inf, -np.inf, np.nan]


def real_inputs(name, tn, rng):
    """(list of Float64 arrays holding values of the type, index where the special points begin)"""
    R = FC.TYPES[tn]
    fi, esub, emax = lim(R)
    lnmax, lnsub, lntiny = math.log(float(fi.max)), math.log(float(fi.smallest_subnormal)), math.log(float(fi.tiny))
    top = 9 if R == F64 else 6
    kmant = [k for k in (1, 2, 5, 10, 20, 23, 24, 30, 40, 52, 53) if k <= fi.nmant + 1]
    trig_top = 100 if R == F64 else 60
    n = 400
    hard, special, main, arity = [], [(s,) for s in COMMON_SPECIAL], None, 1
    if name in ("exp", "expm1", "sinh", "cosh"):
        main = np.concatenate([rnd(rng, n, -40, top), rnd(rng, n // 2, -90, -30)])
        th = lnmax + (math.log(2) if name in ("sinh", "cosh") else 0)
        hard = around(th, R) + around(-th, R) + around(lnsub, R) + around(lntiny, R) + sub_pts(R) + [1.0, -1.0, 0.5, -40.0, 2.0 ** -60]
    elif name == "exp2":
        main = rnd(rng, n, -40, top + 1)
        ints = [-1075, -1074, -1023, -1022, -150, -149, -127, -126, -1, 1, 2, 10, 127, 128, 1023, 1024]
        hard = [float(i) for i in ints] + around(fi.maxexp, R, 1) + around(esub, R, 1) + around(fi.minexp, R, 1) + [0.5, -0.5] + sub_pts(R)[:3]
    elif name == "tanh":
        main = np.concatenate([rnd(rng, n, -40, 4), rnd(rng, n // 2, -4, 3)])
        t1 = 0.5 * math.log(2.0 ** (fi.nmant + 2))
        hard = [s * (t1 + d) for s in (1, -1) for d in (-0.6, -0.3, -0.1, 0.0, 0.1, 0.3, 0.6)] + sub_pts(R) + [40.0, -700.0]
    elif name in ("log", "log2", "log10"):
        main = np.concatenate([rnd(rng, n, esub, emax, False), rnd(rng, n // 2, -3, 3, False)])
        hard = [1 + s * 2.0 ** -k for k in kmant for s in (1, -1)] + sub_pts(R)[0:1] + sub_pts(R)[2:3] + [float(fi.tiny), float(fi.max)]
        hard += [2.0 ** k for k in (esub, fi.minexp, -7, 3, emax)] if name == "log2" else []
        hard += [10.0 ** k for k in (1, 2, 5, 10, -1, -3)] if name == "log10" else []
        hard += [math.e, 1.0] if name == "log" else [1.0]
        special += [(-1.0,), (-float(fi.smallest_subnormal),)]
    elif name == "log1p":
        main = np.concatenate([rnd(rng, n // 2, -90, -30), rnd(rng, n // 2, -30, emax, False), -rnd(rng, n // 2, -30, -1, False)])
        hard = [-1 + 2.0 ** -k for k in kmant if k <= fi.nmant] + sub_pts(R) + [float(fi.max), 1.0, -0.5]
        special += [(-1.0,), (-2.0,)]
    elif name in ("sin", "cos", "tan"):
        main = np.concatenate([rnd(rng, n, -60 if R == F64 else -40, 4), rnd(rng, n, 4, trig_top)])
        hard = [2.0 ** k for k in (0, 1, 2, 10, 20, 30, 40, 50, 60, 80, 100) if k <= trig_top]
        hard += [float(R(float(k * PI / 2))) for k in (1, 2, 3, 4, 5, 6, 7, 8, 100, 1001, 2 ** 20 + 1, -1, -2, -3)] + sub_pts(R)[:4]
    elif name in ("asin", "acos"):
        main = np.concatenate([rnd(rng, n, -60, -1), rnd(rng, n, -4, -1)])
        hard = [1.0, -1.0, 0.5, -0.5] + [s * (1 - 2.0 ** -k) for k in kmant for s in (1, -1)] + sub_pts(R)[:4]
        special += [(1.5,), (-1.5,), (float(np.nextafter(R(1), R(2))),)]
    elif name == "atan":
        main = np.concatenate([rnd(rng, n, -60, 60), rnd(rng, n // 2, -3, 3)])
        hard = [1.0, -1.0, float(fi.max), -float(fi.max), 2.0 ** 53, np.inf, -np.inf] + sub_pts(R)[:4]
        special = [(s,) for s in (0.0, -0.0, np.nan)]
    elif name == "cbrt":
        main = rnd(rng, n, esub, emax)
        hard = [8.0, -27.0, 1e-300 if R == F64 else 1e-40, 3.0 ** 30, -(5.0 ** 9), float(fi.max), -float(fi.max)] + sub_pts(R)
    elif name == "pow":
        arity = 2
        x = rnd(rng, n, -8, 8, False)
        y = rng.uniform(-1, 1, n) * (emax * 1.1) / np.maximum(np.abs(np.log2(x)), 0.05)
        y[::3] = rnd(rng, len(y[::3]), -3, 3)
        main = [x, y]
        xs = rnd(rng, 6, -20, 20, False)
        hard = [(-2.0, 3.0), (-1.5, 7.0), (-3.0, -3.0), (-2.0, 1000.0), (-0.5, 2001.0), (-0.5, 200.0), (1 + 2.0 ** -20, 2.0 ** 25), (1 - 2.0 ** -20, -2.0 ** 24),
                (10.0, 38.0), (10.0, -45.0), (10.0, 308.0), (10.0, -323.0), (2.0, 0.5), (2.0, -0.5)] + [(float(v), s * 0.5) for v in xs for s in (1, -1)]
        special = [(0.0, 0.0), (np.nan, 0.0), (1.0, np.nan), (-8.0, 1.0 / 3.0), (-0.0, -1.0), (0.0, -2.0), (np.inf, -1.0), (-np.inf, 3.0), (2.0, np.inf),
                   (0.5, np.inf), (2.0, -np.inf), (-1.0, np.inf), (-0.0, 3.0), (np.nan, 1.0), (0.0, 2.5)]
    elif name == "atan2":
        arity = 2
        main = [np.concatenate([rnd(rng, n, -20, 20), rnd(rng, n // 2, esub, emax)]), np.concatenate([rnd(rng, n, -20, 20), rnd(rng, n // 2, esub, emax)])]
        s, M = float(fi.smallest_subnormal), float(fi.max)
        hard = [(a * s, b * M) for a in (1, -1) for b in (1, -1)] + [(M, s), (-M, -s), (1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (0.0, -1.0), (-0.0, -1.0),
                                                                 (1.0, 0.0), (-1.0, 0.0), (1.0, -0.0), (np.inf, 1.0), (-np.inf, -1.0), (1.0, -np.inf), (-1.0, -np.inf),
                                                                 (np.inf, np.inf), (np.inf, -np.inf), (-np.inf, -np.inf)]
        special = [(0.0, 1.0), (-0.0, 1.0), (0.0, 0.0), (-0.0, 0.0), (np.nan, 1.0), (1.0, np.nan), (1.0, np.inf), (-1.0, np.inf)]
    elif name == "hypot":
        arity = 2
        main = [rnd(rng, n, -20, 20), rnd(rng, n, -20, 20)]
        E = 500 if R == F64 else 60
        s, M = float(fi.smallest_subnormal), float(fi.max)
        m = rng.uniform(1, 2, 8)
        hard = [(m[0] * 2.0 ** E, m[1] * 2.0 ** E), (m[2] * 2.0 ** -E, -m[3] * 2.0 ** -E), (2.0 ** E, 2.0 ** -E), (m[4] * 2.0 ** -E, 2.0 ** E), (0.7 * M, 0.71 * M),
                (0.7 * M, 0.72 * M), (M, M), (3 * s, 4 * s), (s, s), (3.0, 4.0), (-5.0, 12.0), (M, s), (m[5] * float(fi.tiny), m[6] * float(fi.tiny))]
        special = [(np.inf, np.nan), (np.nan, -np.inf), (np.nan, 1.0), (0.0, 0.0), (-0.0, 5.0), (np.inf, 1.0), (-0.0, -0.0)]
    elif name.startswith("powi"):
        k = int(name[4:])
        u = rng.uniform(-1, 1, n // 4) / 64
        edge = [s * 2.0 ** (e / abs(k)) * (1 + u) for e in (emax + 1, esub - 1) for s in (1, -1)]
        main = np.concatenate([1 + rnd(rng, n, -30, -2), rnd(rng, n, -1, 0)] + edge * 3)
        hard = [2.0, -2.0, 0.5, 3.0, -3.0, 10.0]
    else:
        raise KeyError(name)
    if arity == 1:
        main, hard, special = [main], [(h,) for h in hard], special
    with np.errstate(all="ignore"):
        hard = [tuple(float(R(v)) for v in h) for h in hard]
        special = [tuple(float(R(v)) for v in s) for s in special]
        nm = (N_POWI if name.startswith("powi") else N_REAL) - len(hard) - len(special)
        assert nm >= 40, (name, nm)
        pick = rng.permutation(len(main[0]))[:nm]
        cols = []
        for i in range(arity):
            col = np.concatenate([np.asarray(main[i])[pick].astype(R).astype(F64), [h[i] for h in hard], [s[i] for s in special]])
            cols.append(col)
    return cols, nm + len(hard)


def real_row(name, tn, rng):
    R = FC.TYPES[tn]
    cols, sp0 = real_inputs(name, tn, rng)
    n = len(cols[0])
    ref = np.asarray(FC.BY_NAME[name].ref(*cols)).astype(F64)  # NumPy in Float64 on the (exactly widened) inputs
    lo, ex, sp = np.zeros(n, dtype=R), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for i in range(n):
        args = [float(c[i]) for c in cols]
        with np.errstate(all="ignore"):
            want = R(ref[i])
        plain = all(math.isfinite(a) and a != 0 for a in args)
        v = None
        if not any(math.isnan(a) for a in args) and not (np.isnan(want)):
            try:
                v = MPF[name](*args)
                if isinstance(v, mp.mpc):
                    v = v.real if v.imag == 0 else None
                if v is not None and mp.isnan(v):
                    v = None
            except (ZeroDivisionError, ValueError, OverflowError):
                v = None
        if v is None or (not plain and _trivial(want)) or v == 0:
            # a special value: NumPy's Float64 result is exact here (NaN, a zero with its sign, an infinity, an integer)
            assert _trivial(want) or v is None, (name, tn, args, want)
            if v is not None and v == 0:
                assert want == 0, (name, args, want)
            lo[i], ex[i], sp[i] = want, True, True
        else:
            lo[i], ex[i] = bracket(v, R)
            # NumPy's Float64 result, rounded once, lies in or next to the bracket: a guard against a slip in this file
            assert FC.steps_outside(np.array([want]), np.array([lo[i]]), np.array([ex[i]]))[0] <= 1, (name, tn, args, want, lo[i])
    assert sp[sp0:].sum() >= 1
    return [c.astype(R) for c in cols], lo, ex, sp


# ---- complex rows -----------------------------------------------------------------------------------------------------------
def crnd(rng, n, elo, ehi):
    return rnd(rng, n, elo, ehi) + 1j * rnd(rng, n, elo, ehi)


def dist_to(x, period, phase):
    """distance of x from the nearest phase + k * period"""
    r = np.mod(x - phase, period)
    return np.minimum(r, period - r)


AXIS_ROWS = ("csqrt", "cexp", "clog", "csin", "ccos", "ctanh", "csinh", "ccosh", "cexp2", "clog2", "clog10")


def axis_signs(name, x, negzero):
    """C Annex G / Base: signs (True = negative) of the real and imaginary parts of f(x + i*(+-0)), used where a part is exactly zero"""
    s = bool(negzero)
    if name == "csqrt":
        return False, s
    if name in ("cexp", "cexp2", "ctanh", "csinh"):
        return x < 0, s
    if name in ("clog", "clog2", "clog10"):
        return False, s
    if name == "csin":
        return x < 0, s != (math.cos(x) < 0)
    if name == "ccos":
        return False, s != (math.sin(x) > 0)
    if name == "ccosh":
        return False, s != (x < 0)
    raise KeyError(name)


def cplx_inputs(name, tn, rng):
    """(columns, edge mask, axis mask)"""
    R = FC.real_of(tn)
    fi, esub, emax = lim(R)
    M, s, tiny = float(fi.max), float(fi.smallest_subnormal), float(fi.tiny)
    d64 = R == F64
    n = 600
    arity = FC.BY_NAME[name].arity
    pi = math.pi
    edge, axis = [], []
    wide = crnd(rng, n // 3, esub + 2, emax - 2)
    if name in ("cabs", "csqrt", "csign"):
        main = np.concatenate([crnd(rng, n, -30, 30), wide])
        edge = [M * (1 + 1j), M * (-1 + 0.5j), complex(-M, s), complex(s, s), complex(3 * s, -4 * s), complex(M, s), complex(-s, 5 * s), complex(tiny, -tiny * 0.5),
                (1e308 if d64 else 1e38) * (1 + 1j)]
        axis = [4.0, 2.0, 0.3, -4.0, -2.0, -0.3, M, -M, 11 * s, -11 * s] if name == "csqrt" else []
    elif name in ("cexp", "cexp2"):
        c = math.log(2) if name == "cexp2" else 1.0
        top = (5 if d64 else 2) if name == "cexp" else (6 if d64 else 3)
        z = rnd(rng, n, -20, top) + 1j * rnd(rng, n, -20, 20 if name == "cexp" else 0)  # exp2: th = im * log(2) is rounded, |th| < 1.4
        with np.errstate(all="ignore"):
            zi = z.imag.astype(R).astype(F64) * c
        main = z[dist_to(zi, pi / 2, 0.0) >= 2.0 ** -6]
        if name == "cexp":
            edge = [complex(709.7, 1), complex(-745, 1), complex(-800, 1), complex(700, -2)] if d64 else [complex(88.7, 1), complex(-103, 1), complex(-120, 1), complex(80, -2)]
            axis = [1.0, -1.0, 700.0, -700.0, 800.0, 11 * s] if d64 else [1.0, -1.0, 80.0, -80.0, 100.0, 11 * s]
        else:
            edge = [complex(1023.5, 1), complex(-1074, 1), complex(-1100, 1), complex(1000, -2)] if d64 else [complex(127.5, 1), complex(-149, 1), complex(-160, 1), complex(100, -2)]
            axis = [3.0, 0.5, -1070.0, 1023.0, 1024.0, -0.5] if d64 else [3.0, 0.5, -140.0, 127.0, 128.0, -0.5]
    elif name in ("clog", "clog2", "clog10"):
        z = np.concatenate([crnd(rng, n, -30, 30), crnd(rng, n, -2, 1), wide])
        main = z[np.abs(z - 1) >= 0.25]
        edge = [(1.5e308 if d64 else 1.5e38) * (1 + 1j), M * (1 + 1j), complex(1, 1e-9), complex(1, 2.0 ** -30), complex(s, s), complex(-3 * s, 4 * s), complex(0.6, 0.8),
                complex(-1, 1e-20), complex(1 + 2.0 ** -20, -2.0 ** -12), complex(0.9999, 0.01), complex(M, -s), complex(tiny, tiny)]
        axis = [2.0, 0.5, -2.0, -0.5, M, 11 * s, 1.0, 1 + 2.0 ** -20, -1.0]
    elif name in ("csin", "ccos", "csinh", "ccosh"):
        z = rnd(rng, n, -20, 20) + 1j * rnd(rng, n, -20, 2)
        ph = 0.0 if name in ("csin", "csinh") else pi / 2
        with np.errstate(all="ignore"):
            zr = z.real.astype(R).astype(F64)
        main = z[(np.abs(z.imag) >= 2.0 ** -6) | (dist_to(zr, pi, ph) >= 2.0 ** -6)]
        big, mid = (800.0, 710.2) if d64 else (100.0, 89.0)
        axis = [1.0, -2.0, 3.0, 11 * s, 100.0]
        edge = [complex(1, big), complex(-2, -big), complex(1, mid), complex(0.0, big), complex(-0.0, -big), complex(0.0, 1.0), complex(-0.0, 2.0)]
        if name in ("csinh", "ccosh"):  # the same points with the parts exchanged
            main = main.imag + 1j * main.real
            edge = [complex(e.imag, e.real) for e in edge[:3]]
            axis += [big, -big, mid]
    elif name == "ctanh":
        z = np.concatenate([rnd(rng, n, -20, 5) + 1j * rnd(rng, n, -20, 4), rnd(rng, n, -3, 1) + 1j * rnd(rng, n, -3, 2)])
        with np.errstate(all="ignore"):
            zi = z.imag.astype(R).astype(F64)
        pole = (np.abs(z.real) >= 0.1) | (dist_to(zi, pi, pi / 2) >= 0.1)
        zero = (np.abs(z.real) >= 0.1) | (dist_to(zi, pi, 0.0) >= 0.1) | (np.abs(z) < 1)
        main = z[pole & zero]
        edge = [complex(400, 1), complex(-400, -1), complex(50, 1), complex(-30, 2), complex(177.0, 1), complex(178.0, 1), complex(22.0, -1), complex(23.0, 2),
                complex(11 * s, 11 * s), complex(700, 3)]
        if not d64:
            edge = [e for e in edge if abs(e.real) < 1e38]
        axis = [0.5, -3.0, 20.0, 400.0, 11 * s, -50.0]
    elif name == "cinv":
        main = np.concatenate([crnd(rng, n, -30, 30), crnd(rng, n // 3, -(emax - 3), emax - 3)])
        edge = [M * (1 + 1j), complex(M, s), complex(-M * 0.5, M), tiny * (1 + 1j), complex(tiny * 1.5, tiny / 256), complex(1.0 / M, 0.25 / M) * 4]
    elif name == "cmul":
        main = [crnd(rng, n, -30, 30), crnd(rng, n, -30, 30)]
        h = 2.0 ** ((emax - 3) // 2)
        edge = [(h * (1 + 1j), h * (1 - 0.5j)), (complex(M / 4, M / 8), complex(1, 1)), (complex(tiny, tiny), complex(1, -2))]
    elif name == "cdiv":
        main = [crnd(rng, n, -30, 30), crnd(rng, n, -30, 30)]
        edge = [(M * (1 + 1j), M * (1 + 1j)), (s * (1 + 1j), s * (1 - 1j)), (complex(1, 1), M * (1 + 1j)), (M * (1 + 1j), complex(M, s)),
                (complex(M, -M / 2), complex(M / 2, M)), (tiny * (1 + 1j), complex(3, 4)), (complex(3, 4), tiny * (2 + 1j) * 2.0 ** 30), (complex(7 * s, -9 * s), complex(0.5, 0.25))]
    elif name in ("cpowi5", "cpowi-3"):
        main = crnd(rng, n, -8, 7)
    elif name == "cfma":
        main = [crnd(rng, n, -4, 3), crnd(rng, n, -4, 3), crnd(rng, n, -4, 3)]
    else:
        raise KeyError(name)
    if arity == 1:
        main, edge = [main], [(e,) for e in edge]
    ax = [(complex(x, z0),) for x in axis for z0 in (0.0, -0.0)]
    nm = N_CPLX - len(edge) - len(ax)
    assert nm >= 24 and len(main[0]) >= nm, (name, tn, nm, len(main[0]))
    pick = rng.permutation(len(main[0]))[:nm]
    T = FC.TYPES[tn]
    cols = []
    with np.errstate(all="ignore"):
        for i in range(arity):
            col = np.concatenate([np.asarray(main[i])[pick], np.array([e[i] for e in edge], dtype=C128), np.array([a[i] for a in ax], dtype=C128)])
            cols.append(col.astype(T))
    ntot = len(cols[0])
    em, am = np.zeros(ntot, dtype=bool), np.zeros(ntot, dtype=bool)
    em[nm:nm + len(edge)] = True
    am[nm + len(edge):] = True
    return cols, em, am


def split_dd(v, R):
    """(nearest value of R, the rest in 1/254 of its spacing as int8) of a real mpf; overflow gives an infinity"""
    if v == 0:
        return R(0), 0
    lo, exact = bracket(v, R)
    h = lo
    if not exact:
        up = np.nextafter(lo, R(np.inf))
        if np.isinf(lo):
            h = up if v > -_m(float(np.finfo(R).max)) * (1 + _m(2) ** -(np.finfo(R).nmant + 2)) else lo
        elif np.isinf(up):
            h = lo if v < _m(float(lo)) * (1 + _m(2) ** -(np.finfo(R).nmant + 2)) else up
        else:
            dl, du = v - _m(float(lo)), _m(float(up)) - v
            h = lo if (dl < du or (dl == du and int(np.abs(lo).view(np.uint32 if R == F32 else np.uint64)) % 2 == 0)) else up
    if np.isinf(h) or h == 0:
        return (h if h != 0 else R(math.copysign(0.0, v))), (0 if np.isinf(h) else max(-127, min(127, int(mp.nint(v / _m(float(FC.spacing_of(R(np.finfo(R).smallest_subnormal)))) * 254)))))
    r = (v - _m(float(h))) / _m(float(FC.spacing_of(h)))
    return h, max(-127, min(127, int(mp.nint(r * 254))))


def cplx_row(name, tn, rng):
    cols, em, am = cplx_inputs(name, tn, rng)
    n = len(cols[0])
    R = FC.real_of(tn)
    hi, lo8 = np.zeros(n, dtype=FC.TYPES[tn]), np.zeros((n, 2), dtype=np.int8)
    sre, sim = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for i in range(n):
        args = [complex(c[i]) for c in cols]
        v = MPC[name](*args)
        if am[i] and math.copysign(1.0, args[0].imag) < 0:  # mpmath has one zero: below the axis f(z) = conj(f(conj(z)))
            v = mp.conj(MPC[name](args[0].conjugate()))
        (hr, lr), (hj, lj) = split_dd(mp.re(v), R), split_dd(mp.im(v), R)
        hi[i] = complex(hr, hj)
        lo8[i] = (lr, lj)
        if am[i]:
            x, z0 = args[0].real, args[0].imag
            assert z0 == 0
            sre[i], sim[i] = axis_signs(name, x, math.copysign(1.0, z0) < 0)
    return cols, hi, lo8, em, am, sre, sim


# ---- the file -------------------------------------------------------------------------------------------------------------------
def generate():
    """One array per (type, kind), the rows of FC.ROWS one after another: `names` and `n` (points per row) index them; x holds a
    row's operands one after another."""
    parts = {}
    for row in FC.ROWS:
        if row.cls == "exact":
            continue
        for tn in row.types:
            rng = np.random.default_rng([20261020, sum(map(ord, row.name)), len(row.name), FC.TYPES[tn]().itemsize])
            if row.cls == "faithful":
                cols, lo, ex, sp = real_row(row.name, tn, rng)
                d = {"lo": lo, "ex": ex, "sp": sp}
            else:
                cols, hi, lo8, em, am, sre, sim = cplx_row(row.name, tn, rng)
                d = {"hi": hi, "lo8": lo8, "edge": em, "axis": am, "sre": sre, "sim": sim}
            d["x"] = np.concatenate(cols)
            d["n"] = np.array([len(cols[0])], dtype=np.int32)
            d["names"] = np.array([row.name])
            for k, v in d.items():
                parts.setdefault(tn + "." + k, []).append(v)
    G = {}
    for k, v in parts.items():
        a = np.concatenate(v)
        G[k] = np.packbits(a) if a.dtype == bool else a
    return G


def check_authority():
    for name, args, want in FC.JULIA_AUTHORITY:
        ref = FC.BY_NAME[name].ref
        for R in (F32, F64):
            got = np.asarray(ref(*[np.array([a], dtype=R) for a in args])).astype(R)
            assert FC.same_value(got, np.array([want], dtype=R))[0], (name, args, want, got)


def write_npz(G, path):
    """a .npz with fixed member order and time stamps: the same bytes for the same arrays"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(G):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(G[k]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
    check_authority()
    G = generate()
    if "--check" in sys.argv:
        buf = io.BytesIO()
        write_npz(G, buf)
        same = buf.getvalue() == open(OUT, "rb").read()
        print("fixture reproduced byte for byte" if same else "fixture DIFFERS from the generator's output")
        sys.exit(0 if same else 1)
    write_npz(G, OUT)
    size = os.path.getsize(OUT)
    assert size <= FC.FIXTURE_CAP, size
    print("wrote", OUT, size, "bytes,", len(G), "arrays")
