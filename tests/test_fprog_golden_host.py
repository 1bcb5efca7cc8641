"""The conformance fixture of the f-program's arithmetic (tests/golden/fprog_golden.npz), without a device:
  1. the fixture is self-consistent, within the size cap, and (where mpmath is installed) what its generator writes;
  2. the CPU references meet every row: the oracle and NumPy on the exact rows, NumPy in Float64 rounded once inside every faithful
     bracket, the oracle's std::complex / NumPy's complex128 within 2 ulp of every kept complex point, at most a quarter dropped;
  3. the checkers detect a result two steps off and a zero of the wrong sign;
  4. the formulas csrc/smr_device.h had for complex tanh, sqrt, exp and log, restated in NumPy, are rejected on the edge rows."""
import importlib.util
import os

import numpy as np
import pytest

import fprog_cases as FC
from fprog_cases import C64, C128, F32, F64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fprog_golden.npz")
G = FC.load_fixture(GOLDEN)
FAITHFUL, COMPLEX = FC.cases(("faithful",)), FC.cases(("complex",))


def test_fixture_is_consistent_and_small():
    assert os.path.getsize(GOLDEN) <= FC.FIXTURE_CAP
    for name, tn in FAITHFUL:
        d = FC.fixture_row(G, name, tn)
        R = FC.TYPES[tn]
        assert 0 < d["n"] <= FC.NMAX and all(x.dtype == R and len(x) == d["n"] for x in d["x"]) and d["lo"].dtype == R
        hi = FC.hi_of(d["lo"], d["exact"]).astype(R)
        b = ~d["special"]
        assert np.all(d["lo"][b] <= hi[b]) and not np.isnan(d["lo"][b]).any()
        assert np.all(d["exact"][d["special"]])                  # a special value is asked for as it is
        assert np.all((hi == d["lo"])[b] == d["exact"][b])       # the exact bit and the upper neighbour say the same
        assert d["special"].sum() >= 3 and b.sum() >= 40
    for name, tn in COMPLEX:
        d = FC.fixture_row(G, name, tn)
        assert 0 < d["n"] <= FC.NMAX and all(x.dtype == FC.TYPES[tn] and len(x) == d["n"] for x in d["x"])
        assert not np.isnan(d["hi"]).any() and np.isfinite(np.concatenate([np.asarray(x) for x in d["x"]])).all()  # finite inputs only
        assert np.all(d["x"][0].imag[d["axis"]] == 0) and not np.any(d["edge"] & d["axis"])


def test_generator_reproduces_the_fixture():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_fprog_golden", os.path.join(os.path.dirname(GOLDEN), "make_fprog_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.check_authority()
    with np.errstate(all="ignore"):
        new = gen.generate()
    assert sorted(new) == sorted(G)
    for k in G:
        assert new[k].dtype == G[k].dtype and new[k].tobytes() == G[k].tobytes(), k


def test_julia_authority_rows():
    for name, args, want in FC.JULIA_AUTHORITY:
        for R in (F32, F64):
            got = np.asarray(FC.BY_NAME[name].ref(*[np.array([a], dtype=R) for a in args])).astype(R)
            assert FC.same_value(got, np.array([want], dtype=R))[0], (name, args, want, got)


# ---- 2. the references -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tn", [c for c in FC.cases(("exact",)) if "interp" in FC.BY_NAME[c[0]].paths])
def test_oracle_meets_the_exact_rows(name, tn):
    """criterion 1 on the CPU: the oracle (the compiler's own IEEE arithmetic) against the NumPy expectation, bit for bit"""
    from util import run_oracle
    import strided_jl_amd as S
    row = FC.BY_NAME[name]
    xs = FC.exact_inputs(name, tn)
    want = FC.exact_expected(name, tn, xs)
    dst = S.StridedView(np.zeros(len(xs[0]), dtype=want.dtype, order="F"))
    got = np.asarray(run_oracle(row.f, None, None, dst.size, (dst,) + tuple(S.StridedView(x.copy(order="F")) for x in xs)))
    bad = np.nonzero(~FC.same_value(got, want))[0]
    assert bad.size == 0, (name, tn, [(tuple(x[i] for x in xs), got[i], want[i]) for i in bad[:5]])


def _py_float(name, a, b=None):
    """the JIT-only exact float rows on Python's own floats (CPython's fmod / floor / %: none of it NumPy's or the device's code)"""
    import math
    if name in ("floor", "ceil", "trunc"):
        if not math.isfinite(a):
            return a
        return math.copysign(float(getattr(math, name)(a)), a)  # the integer loses the sign of -0.0 and of (-1, 0)
    if name == "round":
        return a if not math.isfinite(a) else math.copysign(float(round(a)), a)
    if name == "sign":
        return a if (a == 0 or a != a) else math.copysign(1.0, a)
    if a != a or b != b or math.isinf(a) or b == 0:
        return math.nan
    if name == "rem":
        return math.fmod(a, b)
    r = a % b  # Python's float %: floored, the sign of the divisor, (+-0) by the divisor's sign
    return math.inf * (1 if b > 0 else -1) if (math.isinf(b) and r != a) else r


@pytest.mark.parametrize("name", ["floor", "ceil", "trunc", "round", "sign", "rem", "mod"])
def test_python_floats_meet_the_jit_only_exact_rows(name):
    """criterion 1 for the rows no CPU engine of the project runs: the expectation against Python's float arithmetic"""
    for tn in FC.REAL:
        R = FC.TYPES[tn]
        xs = FC.exact_inputs(name, tn)
        want = FC.exact_expected(name, tn, xs)
        got = np.array([_py_float(name, *[float(x[i]) for x in xs]) for i in range(len(xs[0]))], dtype=np.float64).astype(R)
        bad = np.nonzero(~FC.same_value(got, want))[0]
        assert bad.size == 0, (name, tn, [(tuple(x[i] for x in xs), got[i], want[i]) for i in bad[:5]])


@pytest.mark.parametrize("name,tn,wide", FC.int_cases())
def test_numpy_and_the_oracle_meet_the_integer_rows(name, tn, wide):
    """criterion 1 for the integer class: the expectation (Python's unbounded integers, wrapped) against NumPy's arithmetic in the
    operands' own type, and against the oracle where the row is a base opcode"""
    f, ar, _, paths, kind = FC.INT_ROWS[name]
    xs = FC.int_inputs(name, tn)
    want = FC.int_expected(name, tn, wide, xs)
    T = FC.TYPES[tn]
    a = xs[0]
    with np.errstate(all="ignore"):
        if name.startswith("powi"):
            got = np.power(a, T(int(name[4:])))
        elif name.startswith(("mod", "rem")):
            k, w = np.int64(int(name[3:])), a.astype(np.int64)
            got = np.zeros_like(w) if k == -1 else (np.mod(w, k) if name.startswith("mod") else np.fmod(w, k))
        elif name == "sign":
            got = np.sign(a.astype(np.int64)).astype(T)
        elif name == "abs":
            got = np.abs(a)
        elif name == "abs2":
            got = a * a
        elif name == "fma":
            got = xs[0] * xs[1] + xs[2]
        elif name == "not":
            got = ~a
        elif name == "neg":
            got = (-a.astype(np.int64)).astype(T) if T == np.int64 else (np.zeros_like(a) - a)
        else:
            op = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "min": np.minimum, "max": np.maximum, "lt": np.less,
                  "le": np.less_equal, "eq": np.equal, "ne": np.not_equal, "and": np.bitwise_and, "or": np.bitwise_or, "xor": np.bitwise_xor}[name]
            got = op(xs[0], xs[1])
    got = np.asarray(got)
    if wide:
        got = got.astype(np.int64)
    assert got.dtype == want.dtype and np.array_equal(got, want), (name, tn, wide)
    if "interp" in paths:
        from util import run_oracle
        import strided_jl_amd as S
        dst = S.StridedView(np.zeros(len(a), dtype=want.dtype, order="F"))
        o = np.asarray(run_oracle(f, None, None, dst.size, (dst,) + tuple(S.StridedView(x.copy(order="F")) for x in xs)))
        assert np.array_equal(o, want), (name, tn, wide, "oracle")


def test_round_fraction_is_the_ieee_rounding():
    """the exact-rational rounding behind the fma row against the hardware's + and *, subnormal and overflowing results included"""
    from fractions import Fraction
    for tn in FC.REAL:
        R = FC.TYPES[tn]
        a, b = FC.exact_inputs("mul", tn)
        with np.errstate(all="ignore"):
            for x, y, p, s in zip(a, b, a * b, a + b):
                if np.isfinite(x) and np.isfinite(y):
                    q = Fraction(float(x)) * Fraction(float(y))
                    if q != 0:
                        assert FC.round_fraction(q, R) == p, (x, y)
                    q = Fraction(float(x)) + Fraction(float(y))
                    if q != 0:
                        assert FC.round_fraction(q, R) == s, (x, y)


@pytest.mark.parametrize("name,tn", FAITHFUL)
def test_numpy_float64_rounded_once_is_inside_every_bracket(name, tn):
    d = FC.fixture_row(G, name, tn)
    ref = FC.reference(name, tn, d["x"])
    sp = d["special"]
    assert FC.same_value(ref[sp], d["lo"][sp]).all()
    out = FC.steps_outside(ref, d["lo"], d["exact"])
    bad = np.nonzero((out != 0) & ~sp)[0]
    assert bad.size == 0, (name, tn, [(tuple(x[i] for x in d["x"]), ref[i], d["lo"][i], int(out[i])) for i in bad[:5]])


@pytest.mark.parametrize("name,tn", COMPLEX)
def test_complex_reference_is_within_two_ulp(name, tn):
    """criterion 3's condition (and where E_ref comes from), and criterion 4 for the reference: every edge point within the row's
    own bound, parts on the real axis included"""
    d = FC.fixture_row(G, name, tn)
    j = FC.complex_judge(name, tn, d)
    assert j["dropped"] * 4 <= j["main"], (name, tn, j["dropped"], j["main"])
    assert j["E_ref"] <= 2.0
    bad, e = FC.complex_failures(j["ref"], name, tn, d, j)
    assert bad.size == 0, (name, tn, j["bound"], [(tuple(x[i] for x in d["x"]), j["ref"][i], d["hi"][i], float(e[i])) for i in bad[:5]])


# ---- 3. the checkers -------------------------------------------------------------------------------------------------------------
def test_the_checkers_detect_two_steps_and_a_flipped_zero():
    for tn in FC.REAL:
        R = FC.TYPES[tn]
        d = FC.fixture_row(G, "exp", tn)
        ref = FC.reference("exp", tn, d["x"])
        b = ~d["special"] & (d["lo"] > np.finfo(R).tiny) & (d["lo"] < np.finfo(R).max / 4)
        up2 = np.nextafter(np.nextafter(FC.hi_of(d["lo"], d["exact"]).astype(R), R(np.inf)), R(np.inf))
        dn2 = np.nextafter(np.nextafter(d["lo"], R(-np.inf)), R(-np.inf))
        assert np.all(FC.steps_outside(up2, d["lo"], d["exact"])[b & ~d["exact"]] == 2)
        assert np.all(FC.steps_outside(dn2, d["lo"], d["exact"])[b & ~d["exact"]] == 2)
        assert np.all(FC.steps_outside(up2, d["lo"], d["exact"])[b & d["exact"]] == 1)  # an exact lo admits one step either way
        assert np.all(FC.steps_outside(ref, d["lo"], d["exact"])[b] == 0)
        # a zero of the wrong sign: sin(-0.0) must be -0.0, tiny negative results may not round to +0.0
        d = FC.fixture_row(G, "sin", tn)
        z = np.nonzero(d["special"] & (d["lo"] == 0))[0]
        assert z.size >= 2
        assert not FC.same_value(-d["lo"][z], d["lo"][z]).any() and FC.same_value(d["lo"][z], d["lo"][z]).all()
        assert FC.steps_outside(np.array([R(0.0)]), np.array([R(-0.0)]), np.array([True]))[0] > 0
        s = np.finfo(R).smallest_subnormal
        assert FC.steps_outside(np.array([R(0.0)]), np.array([-s]), np.array([False]))[0] == 1  # bracket [-s, -0.0]
        assert FC.steps_outside(np.array([R(-0.0)]), np.array([-s]), np.array([False]))[0] == 0
    for tn in FC.CPLX:
        T, R = FC.TYPES[tn], FC.real_of(tn)
        d = FC.fixture_row(G, "csqrt", tn)
        j = FC.complex_judge("csqrt", tn, d)
        ref = j["ref"]
        assert FC.complex_failures(ref, "csqrt", tn, d, j)[0].size == 0
        # the whole value moved by twice the bound (and the reference's own two ulp)
        off = (ref.astype(C128) * (1 + (2 * j["bound"] + 4) * float(np.finfo(R).eps))).astype(T)
        m = j["keep"] & np.isfinite(d["hi"]) & (np.abs(d["hi"]) > np.finfo(R).tiny)
        assert np.all(FC.cx_error(off, d["hi"], d["lo"], tn)[m] > j["bound"])
        # sqrt(-4 - 0i) = +0 - 2i: the zero real part with the other sign, the imaginary part with the other sign
        ax = np.nonzero(d["axis"])[0]
        flip = ref.copy()
        flip.real[ax] = -ref.real[ax]
        bad = FC.complex_failures(flip, "csqrt", tn, d, j)[0]
        zero_re = ax[d["hi"].real[ax] == 0]
        assert zero_re.size >= 4 and set(zero_re) <= set(bad)


# ---- 4. the formulas this fixture was written against ----------------------------------------------------------------------------
def _parent(name, z):
    """csrc/smr_device.h before the complex functions followed Base/complex.jl, operation for operation in the real type"""
    R = z.real.dtype.type
    x, y = z.real, z.imag
    with np.errstate(all="ignore"):
        if name == "ctanh":
            x2, y2 = x + x, y + y
            den = np.cosh(x2) + np.cos(y2)
            re, im = np.sinh(x2) / den, np.sin(y2) / den
        elif name == "csqrt":
            r = np.hypot(x, y)
            t = np.sqrt((r + np.abs(x)) * R(0.5))
            u = np.abs(y) / (t + t)
            re, im = np.where(x >= 0, t, u), np.where(x >= 0, y / (t + t), np.copysign(t, y))
            re, im = np.where(r == 0, R(0), re), np.where(r == 0, y, im)
        elif name == "cexp":
            e = np.exp(x)
            re, im = e * np.cos(y), e * np.sin(y)
        elif name == "clog":
            re, im = np.log(np.hypot(x, y)), np.arctan2(y, x)
        return (re + 1j * im).astype(z.dtype)


# the issue's table: (row, type, argument) -> what the old formula gave
PARENT_ROWS = [("ctanh", "c128", 400 + 1j), ("ctanh", "c64", 50 + 1j), ("csqrt", "c128", 1e308 + 1e308j), ("cexp", "c128", 800 + 0j),
               ("clog", "c128", 1.5e308 + 1.5e308j), ("clog", "c128", 1 + 1e-9j)]


@pytest.mark.parametrize("name,tn,z", PARENT_ROWS)
def test_edge_rows_reject_the_old_formulas(name, tn, z):
    d = FC.fixture_row(G, name, tn)
    j = FC.complex_judge(name, tn, d)
    x = d["x"][0]
    i = np.nonzero((x == FC.TYPES[tn](z)) & ~np.signbit(x.imag))[0]
    assert i.size == 1, (name, tn, z)
    old = _parent(name, np.ascontiguousarray(x))
    bad, e = FC.complex_failures(old, name, tn, d, j)
    assert i[0] in bad, (name, tn, z, old[i[0]], d["hi"][i[0]], float(e[i[0]]), j["bound"])
    # and only there: on the main points (away from the ends of the range, the axis and |z| = 1) the old formula is inside the bound,
    # which is why the tests before this one could not see it
    # (tanh apart: near the poles cosh(2x) + cos(2y) cancels, and the old formula misses main points there as well)
    main = j["keep"] & ~d["edge"] & ~d["axis"]
    assert main.sum() >= 24 and name == "ctanh" or not np.isin(bad, np.nonzero(main)[0]).any(), (name, tn, [(x[i], old[i], float(e[i])) for i in bad if main[i]][:5])
