"""Deterministic table of CONTRACTION GROUPS (tests/test_group_contract_host.py, tests/test_gpu_group_contract.py).

A row is a list of members, each a contract_cases.Case -- an outer-product reduction over windowed operands of its own: NaN / poison
surrounds the inputs, random finite bits surround the destination, the data is integer-valued so that every order gives the same
bits -- with one f, one op, one kind of initop (beta per member under `scale`), and a tile: 0 = the planner's rule, 16 / 32 forced
through option "group_contract_tile".  Tile extents and reduced lengths come from CC.tile_numbers, so the table follows the tuned
tile.  Every member's expected parent is Case.expected (NumPy in a wide type).  Nothing here imports torch."""
import numpy as np

import contract_cases as CC
import strided_jl_amd as S
import window_cases as W
from strided_jl_amd import _lib as L

MN = (2, 15, 16, 17, 31, 32, 33, 48)
LAYOUTS = [("col", "col", "col"), ("col", "trans", "col"), ("trans", "col", "trans"), ("step", "step", "step"), ("rev", "col", "rev"),
           ("whole", "whole", "whole_trans"), ("whole", "whole_trans", "whole"), ("whole", "whole", "whole")]
TWO_RED = ((0, 1), (0, 2, 3), (1, 2, 3))
TYPES = dict(CC.TYPES)
TYPES.pop("i32_i64")                     # (the issue's types: f32, f64, c32, c64, i64 and the mixed row)
BOOL3 = (CC.BOOL, CC.BOOL, CC.BOOL)
COUNTS = (1, 2, 3, 37, 300)


def tk_of(tn):
    """The chunk of the inner reduced dim: the same for 16 x 16 and 32 x 32 tiles (asserted), read from describe()."""
    key = "i64" if tn == "bool" else tn
    tk16, tk32 = CC.tile_numbers(key, 16)[2], CC.tile_numbers(key, 32)[2]
    assert tk16 == tk32
    return tk16


def initop_of(kind, i, dts):
    """The member's initop for the row's kind: beta differs from member to member under `scale`."""
    if kind == "scale":
        return ("scale", 2 + i % 3)
    return {"zero": "zero", "none": None, "const": ("const", 3)}[kind]


class BoolCase(CC.Case):
    """Case.build for Bool operands of any size: the destination's parent is surrounded by random True / False (window_cases.finite_bits
    draws whole 8-byte words), the inputs' by True."""

    def build(self, seed=0):
        rng = np.random.default_rng([seed, len(self.name)])
        ops = []
        for k, (ax, dt, lay, cj) in enumerate(zip(self.axes, self.dts, self.layouts, self.conjs)):
            sub = [self.dims[d] for d in ax]
            fill = (lambda n: rng.integers(0, 2, size=n).astype(np.bool_)) if k == 0 else (lambda n: np.ones(n, dtype=np.bool_))
            v = CC._window(sub, lay, dt, fill, cj)
            idx = W.element_index(v).ravel()
            v.parent[idx] = CC.int_values(idx.size, dt, 5 if k == 0 else k)
            ops.append(CC._expand(v, ax, len(self.dims)))
        return tuple(ops)


class Row:
    def __init__(self, name, tn, dts, specs, kind, tile, f="mul", op="+", plant=False):
        self.name, self.tn, self.dts, self.kind, self.tile, self.fname, self.op, self.plant = name, tn, dts, kind, tile, f, op, plant
        self.members = [(BoolCase if tn == "bool" else CC.Case)("%s#%d" % (name, i), dims, axes, dts, CC.CONTRACT, layouts=lay, conjs=cj, f=f, op=op)
                        for i, (dims, axes, lay, cj) in enumerate(specs)]
        self.needs_prog = f != "mul" or tn in ("mixed", "bool")

    def __repr__(self):
        return self.name

    def initop(self, i):
        return initop_of(self.kind, i, self.dts)

    def build(self):
        """Host operands of every member: [(destination, input 1, input 2), ...].  The inputs of member i are rotated by an amount of
        its own, so that members of one shape hold different data."""
        out = []
        for i, c in enumerate(self.members):
            ops = c.build(seed=i)
            for k in (1, 2):
                u = np.unique(W.element_index(ops[k]).ravel())
                ops[k].parent[u] = np.roll(ops[k].parent[u], 7 * i + k)
            if self.plant and min(c.dims[:2]) >= 12 and c.dims[-1] >= 5 and c.axes in (CC.MM, CC.BATCH):   # NaN wins where it meets an output, -Inf otherwise
                A, B = ops[1], ops[2]
                ia, ib = W.element_index(A), W.element_index(B)
                A.parent[ia[(3,) + (0,) * (ia.ndim - 2) + (1,)]] = np.nan
                A.parent[ia[(5,) + (0,) * (ia.ndim - 2) + (2,)]] = -np.inf
                B.parent[ib[(0, 9) + (0,) * (ib.ndim - 3) + (2,)]] = np.inf
                B.parent[ib[(0, 11) + (0,) * (ib.ndim - 3) + (4,)]] = np.inf
            out.append(ops)
        return out

    def expected(self, built):
        with np.errstate(all="ignore"):  # (planted -Inf + Inf)
            return [c.expected(ops, self.initop(i)) for i, (c, ops) in enumerate(zip(self.members, built))]

    def problems(self, built, stream=0):
        """[(smr_problem, keepalive), ...] of the members over the given operands."""
        return [S.build_problem(c.f, c.op, self.initop(i), c.dims, S.promoteshape(c.dims, *ops), stream=stream)
                for i, (c, ops) in enumerate(zip(self.members, built))]

    def group(self, built, independent=False, stream=0):
        ps = self.problems(built, stream)
        with CC.option("group_contract_tile", self.tile):
            return L.Group([p[0] for p in ps], independent, keepalive=(ps, built))

    def single_descs(self, built):
        """describe() of every member's single plan under contract = 2."""
        out = []
        with CC.option("contract", 2):
            for i, (c, ops) in enumerate(zip(self.members, built)):
                p = c.plan(ops, self.initop(i))
                out.append(p.describe())
                p.close()
        return out


def mismatch(case, got_parent, want_parent, desc=""):
    """CC.mismatch, with NaN positions compared as positions (payloads are not defined) and everything else byte for byte."""
    want = want_parent
    got = np.ascontiguousarray(got_parent).reshape(-1)
    if want.dtype.kind in "fc" and got.size == want.size and np.isnan(want).any():
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            return "%s: NaN positions differ | %s" % (case.name, desc)
        got, want = got.copy(), want.copy()
        got[np.isnan(want)] = 0
        want[np.isnan(want)] = 0
    return CC.mismatch(case, got, want, desc)


# ---- members -------------------------------------------------------------------------------------------------------------------------
def _mm(m, n, k, lay, cj=None):
    return ((m, n, k), CC.MM, lay, cj)


def with_conj(specs, cj):
    """The same members with these conj flags (destination, input 1, input 2): one signature per group."""
    return [(dims, axes, lay, cj) for dims, axes, lay, _ in specs]


def specs_for(tn, count):
    """`count` members: the first and the last have a single workgroup (on either tile), a member of many sits in the middle, then
    members that pin the kernel's paths on both tiles -- whole tiles with vector loads along the tiled dim and along k, whole tiles
    of padded windows (element loads), ragged tiles, a batch dim, two reduced dims -- then the walk over
    m, n in MN x K in {2, TK, TK + 1, 2 TK + 1} x LAYOUTS."""
    tk = tk_of(tn)
    first, last = _mm(15, 2, 2, LAYOUTS[0]), _mm(2, 15, tk, LAYOUTS[1])
    many = ((48, 48, 3, 2), CC.BATCH, ("col", "trans", "col"), None)   # 9 x 3 workgroups of 16 x 16, 4 x 3 of 32 x 32
    if count == 1:
        return [_mm(15, 16, tk + 1, LAYOUTS[2])]
    if count == 2:
        return [first, last]
    pins = [
        many,
        _mm(32, 32, tk, LAYOUTS[5]),               # whole tiles, vectors along the tiled dim / along k
        _mm(32, 32, 2 * tk, LAYOUTS[6]),           # ... along k / along the tiled dim
        _mm(32, 32, 2 * tk + 1, LAYOUTS[7]),       # ... along the tiled dim, a ragged last chunk
        _mm(32, 32, tk + 1, LAYOUTS[0]),           # whole tiles of padded windows: element loads
        _mm(33, 17, 2 * tk + 1, ("step", "rev", "col")),
        ((17, 33, 3, tk + 1), CC.BATCH, ("col", "trans", "col"), None),
        ((33, 15, tk + 1, 2), TWO_RED, ("col", "col", "col"), None),
        _mm(17, 31, 5, ("trans", "col", "trans")),
        _mm(31, 17, 5, ("col", "col", "trans")),
    ]
    if count == 3:
        return [first, many, last]
    walk = []
    i = 0
    while len(walk) + len(pins) + 2 < count:
        walk.append(_mm(MN[(3 * i + 1) % 8], MN[(5 * i + 2 + i // 8) % 8], (2, tk, tk + 1, 2 * tk + 1)[(i + i // 4) % 4], LAYOUTS[(i // 2) % 8]))
        i += 1
    return [first] + pins + walk + [last]


_TABLE = None


def table():
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    rows = []
    kinds = ("zero", "none", "const", "scale")
    n = 0
    for tn, dts in TYPES.items():
        for count in (1, 2, 3, 37):
            for tile in ((0,) if count < 3 else (0, 16, 32)):
                rows.append(Row("%s/mul/n%d/t%d" % (tn, count, tile), tn, dts, specs_for(tn, count), "scale" if count == 37 and tile == 0 else kinds[n % 4], tile))
                n += 1
    # conj flags are part of the signature every member shares: a conj'd input (the adjoint's), a conj'd destination and input
    for tn, tile, kind, cj in (("c64", 16, "scale", (False, True, False)), ("c32", 32, "none", (True, False, True)), ("c64", 32, "const", (True, True, True)),
                               ("c32", 16, "scale", (False, False, True))):
        rows.append(Row("%s/conj%d%d%d/n12/t%d" % ((tn,) + tuple(int(x) for x in cj) + (tile,)), tn, TYPES[tn],
                        with_conj(specs_for(tn, 37)[:11] + specs_for(tn, 2)[1:], cj), kind, tile))
    rows.append(Row("f64/mul/n300/t0", "f64", TYPES["f64"], specs_for("f64", 300), "scale", 0))
    # enough members that fill 32 x 32 tiles at least half: the rule's own choice of the larger tile (256 workgroups and more)
    tk = tk_of("f32")
    full = [(31, 32, 2), (32, 32, tk), (32, 48, tk + 1), (48, 31, 5), (24, 24, 2 * tk + 1), (17, 32, 3)]
    specs = [_mm(*full[i % 6], LAYOUTS[i % 8]) for i in range(278)] + [_mm(24, 24, 2, LAYOUTS[1])]
    specs.insert(140, ((48, 48, 3, 2), CC.BATCH, ("col", "trans", "col"), None))
    rows.append(Row("f32/mul/n280/t0", "f32", TYPES["f32"], specs, "scale", 0))
    rows.append(Row("f32/mul/n300/t32", "f32", TYPES["f32"], specs_for("f32", 300), "none", 32))
    # other f / op: runtime-compiled (or interpreted under jit = 0)
    for tn, tile, kind in (("f32", 16, "none"), ("c64", 32, "scale"), ("i64", 16, "zero")):
        rows.append(Row("%s/dist/n3/t%d" % (tn, tile), tn, TYPES[tn], specs_for(tn, 3), kind, tile, f="dist"))
    for tn, tile, kind in (("f64", 32, "scale"), ("i64", 16, "const")):
        rows.append(Row("%s/asym/n12/t%d" % (tn, tile), tn, TYPES[tn], specs_for(tn, 37)[:11] + specs_for(tn, 2)[1:], kind, tile, f="asym"))
    for tile in (16, 32):  # planted NaN and +-Inf in every member that is large enough
        rows.append(Row("f64/minplus/n9/t%d" % tile, "f64", TYPES["f64"], specs_for("f64", 37)[:8] + specs_for("f64", 2)[1:], "none", tile, f="plus", op="min", plant=True))
    rows.append(Row("bool/or_and/n3/t32", "bool", BOOL3, specs_for("bool", 3), "none", 32, f="and", op="|"))
    rows.append(Row("bool/or_and/n37/t0", "bool", BOOL3, specs_for("bool", 37), "zero", 0, f="and", op="|"))
    _TABLE = rows
    return rows


def row(name):
    return {r.name: r for r in table()}[name]
