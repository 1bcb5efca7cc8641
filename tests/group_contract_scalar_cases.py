"""Deterministic table of CONTRACTION GROUPS WITH PER-MEMBER CONSTANTS of f -- SMR_GROUP_CONTRACT_SCALARS, an alpha per block
(tests/test_group_contract_scalars_host.py, tests/test_gpu_group_contract_scalars.py).

Built on tests/group_contract_cases.py: a row is a list of members, windows of padded parents with integer-valued data, and every
member now has constants of f of its own.  The functions:
  mula     x * y * alpha                 the mul! form: natively compiled in a scalars=member group (f=mul2scale), W = 2
  dist2    (x - y) * (x - y) * c + d     two constants, W = 4: a program
  plusc    x + y + c                     with op = min
Data and constants are chosen so that every result is exact in NumPy whatever the order: small integers, alpha a small dyadic
rational (complex: a Gaussian integer) -- the base values -1, 1, -2, 2, 3, 0.5, -0.25, 4, shifted by 8 per round so that every member
of a row has a DISTINCT alpha -- and for Int64 a wrapping row with alpha = 2^62 on data whose sums are not multiples of 4.  (The
constants of an f-program travel as Float64: 2^62 + 1 is not representable and expr.Const refuses it, so the row takes 2^62, the
largest power of two whose products with this data still wrap.)  A constant is typed like the arrays (np.float32 for Float32
members: a Python float is Julia's Float64 and would widen the call).  Pattern `ends`: every alpha equal but the first and the
last member's.  Pattern `same`: all equal -- the flag is set and the plan is the shared one.  Nothing here imports torch."""
import numpy as np

import contract_cases as CC
import strided_jl_amd as S
from group_contract_cases import LAYOUTS, Row, _mm, mismatch, specs_for, tk_of  # noqa: F401  (mismatch: for the tests)
from strided_jl_amd import _lib as L

TYPES = CC.TYPES
BASE = (-1, 1, -2, 2, 3, 0.5, -0.25, 4)
BASE_INT = (-1, 1, -2, 2, 3, 8, -3, 4)      # (distinct modulo 8: shifted by 8 per round they never meet)
WRAP = 2 ** 62


def scalar_of(tn, v):
    """The constant `v` typed like the arrays of a row of type `tn` (see the module docstring)."""
    if tn == "i64":
        return int(v)
    if tn == "f32":
        return np.float32(v)
    if tn == "c32":
        return np.complex64(v)
    if tn == "c64":
        return complex(v)
    return float(v)   # f64, and mixed (Float32 inputs into a Float64 destination: computed in Float64)


def alpha_of(tn, i, count, pattern, salt=0):
    """Member i's constant under the row's pattern; `salt` shifts the base values (the second constant of dist2: never equal to the first)."""
    if pattern == "same":
        j = 3
    elif pattern == "ends":
        j = 4 if i == 0 else (6 if i == count - 1 else 3)
    else:
        j = i
    j += salt
    integer = tn in ("i64", "c32", "c64")
    re = (BASE_INT if integer else BASE)[j % 8] + 8 * (j // 8)
    if tn in ("c32", "c64"):
        return scalar_of(tn, complex(re, 1 + j % 3))
    return scalar_of(tn, re)


def make_f(fname, cs):
    """(f for the library, the same for NumPy) of one member with constants `cs`."""
    if fname == "mula":
        a, = cs
        return (lambda x, y: x * y * a), (lambda x, y: (x * y) * a)
    if fname == "dist2":
        c, d = cs
        return (lambda x, y: (x - y) * (x - y) * c + d), (lambda x, y: (x - y) * (x - y) * c + d)
    c, = cs
    return (lambda x, y: x + y + c), (lambda x, y: x + y + c)


NCONST = {"mula": 1, "dist2": 2, "plusc": 1}


class SRow(Row):
    """A row of group_contract_cases with constants per member.  `split` is option "group_contract_split" for the row (0 = unsplit)."""

    def __init__(self, name, tn, specs, kind, tile, f="mula", op="+", pattern="distinct", split=0, consts=None):
        super().__init__(name, tn, TYPES[tn], specs, kind, tile, f="mul", op=op)
        self.fname, self.pattern, self.split = f, pattern, split
        n = len(self.members)
        self.consts = consts or [tuple(alpha_of(tn, i, n, pattern, 5 * s) for s in range(NCONST[f])) for i in range(n)]
        for c, cs in zip(self.members, self.consts):
            c.fname = f
            c.f, c.npf = make_f(f, cs)
        self.needs_prog = f != "mula" or tn == "mixed"
        self.W = 2 * NCONST[f]

    @property
    def shared(self):
        return len({repr(cs) for cs in self.consts}) == 1

    @property
    def f_tag(self):
        """describe()'s f= under the flag: the mul! form is native only with a row of constants per member."""
        return "prog" if self.needs_prog or self.shared else "mul2scale"

    def expected(self, built):
        with np.errstate(all="ignore"):   # (the wrapping Int64 row)
            return super().expected(built)

    def problems(self, built, stream=0, member0=False):
        """[(smr_problem, keepalive), ...]; `member0`: every member with member 0's constants (the unflagged group of the same shape)."""
        f0 = self.members[0].f
        return [S.build_problem(f0 if member0 else c.f, c.op, self.initop(i), c.dims, S.promoteshape(c.dims, *ops), stream=stream)
                for i, (c, ops) in enumerate(zip(self.members, built))]

    def group(self, built, independent=False, stream=0, flag=True, member0=False):
        ps = self.problems(built, stream, member0)
        with CC.option("group_contract_tile", self.tile), CC.option("group_contract_split", self.split):
            return L.Group([p[0] for p in ps], independent, keepalive=(ps, built), contract_scalars=flag)


def wrap_consts(n):
    """Distinct constants around 2^62, each exact in Float64: 2^62, -2^62, 3 * 2^60, -3 * 2^60, 2^61, -2^61, ..."""
    vals = (WRAP, -WRAP, 3 * 2 ** 60, -3 * 2 ** 60, 2 ** 61, -2 ** 61, 5 * 2 ** 59, -5 * 2 ** 59)
    assert n <= len(vals)
    return [(vals[i],) for i in range(n)]


_TABLE = None


def table():
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    R = SRow
    tk = tk_of("f32")
    # members with several workgroups on tile 16: ragged (17, 33), whole (32), vector loads (aligned parents, 40 = whole tiles + a ragged one)
    wg = [_mm(17, 33, 5, LAYOUTS[0]), _mm(33, 40, tk + 1, LAYOUTS[1]), _mm(32, 32, tk, LAYOUTS[5]), _mm(40, 40, 2 * tk, LAYOUTS[6]), _mm(40, 17, 3, LAYOUTS[7]),
          _mm(17, 17, 2 * tk + 1, LAYOUTS[2])]
    blocks = [_mm(16, 16, 3, LAYOUTS[(i % 3) * 2]) for i in range(2049)]
    long_ = lambda t: [_mm(16, 16, 600, LAYOUTS[0]), _mm(12, 9, 5, LAYOUTS[1]), _mm(8, 24, 1200, LAYOUTS[5 if t else 2]), _mm(20, 7, 5, LAYOUTS[0]), _mm(16, 16, 600, LAYOUTS[7])]  # noqa: E731
    rows = [
        # member counts, both alpha patterns, every class, both tiles, the four kinds of initop
        R("f64/mula/n2/t0/distinct", "f64", specs_for("f64", 2), "scale", 0),
        R("f32/mula/n3/t16/distinct", "f32", specs_for("f32", 3), "zero", 16),
        R("c32/mula/n3/t32/ends", "c32", specs_for("c32", 3), "none", 32, pattern="ends"),
        R("c64/mula/n37/t16/distinct", "c64", specs_for("c64", 37), "const", 16),
        R("f64/mula/n37/t32/ends", "f64", specs_for("f64", 37), "scale", 32, pattern="ends"),
        R("i64/mula/n37/t0/distinct", "i64", specs_for("i64", 37), "none", 0),
        R("f32/mula/n300/t32/distinct", "f32", specs_for("f32", 300), "none", 32),
        R("f64/mula/n2049/t16/distinct", "f64", blocks, "zero", 16),
        R("i64/mula/n6/t16/wrap", "i64", wg, "scale", 16, consts=wrap_consts(6)),
        R("f32/mula/wg6/t16/distinct", "f32", wg, "scale", 16),
        R("c64/mula/wg6/t32/ends", "c64", wg, "zero", 32, pattern="ends"),
        # programs: two constants (W = 4), another op, converted operand types
        R("f32/dist2/n12/t16/distinct", "f32", specs_for("f32", 37)[:11] + specs_for("f32", 2)[1:], "scale", 16, f="dist2"),
        R("c64/dist2/n3/t32/distinct", "c64", specs_for("c64", 3), "zero", 32, f="dist2"),
        R("i64/dist2/n3/t16/ends", "i64", specs_for("i64", 3), "const", 16, f="dist2", pattern="ends"),
        R("f64/dist2/n120/t0/distinct", "f64", specs_for("f64", 120), "none", 0, f="dist2"),
        R("f64/plusc_min/n9/t32/distinct", "f64", specs_for("f64", 37)[:8] + specs_for("f64", 2)[1:], "none", 32, f="plusc", op="min"),
        R("mixed/mula/n12/t16/distinct", "mixed", specs_for("mixed", 37)[:11] + specs_for("mixed", 2)[1:], "scale", 16),
        # split and unsplit members in one group: forced slices on both tiles, and the group rule
        R("f64/mula/split4/t16/distinct", "f64", long_(0), "scale", 16, split=4),
        R("f32/dist2/split4/t32/distinct", "f32", long_(1), "none", 32, f="dist2", split=4),
        R("c64/mula/rule/t0/distinct", "c64", long_(0), "zero", 0, split=1),
        # the flag is set and every alpha is the same: the shared plan
        R("f64/mula/n12/t0/same", "f64", specs_for("f64", 37)[:11] + specs_for("f64", 2)[1:], "scale", 0, pattern="same"),
    ]
    _TABLE = rows
    return rows


def row(name):
    return {r.name: r for r in table()}[name]
