"""Case table of outer-product reductions for the CONTRACT family (tests/test_contract_host.py, tests/test_gpu_contract.py).

A case is a box `dims` and, per operand, the box dims it varies along (`axes`): the destination first, then the inputs.  The generic
product is dims = (m, n, k) with axes ((0, 1), (0, 2), (1, 2)).  Every operand is a window of a padded column-major parent
(window_cases.layout): NaN (integers: the type's minimum, Bool: True) surrounds the inputs, random finite bits surround the
destination, and the destination's WHOLE parent is compared byte for byte with the expected result written into a copy.

The data is integer-valued and bounded like tests/reduce_exact_cases.py (its `pattern`): every partial result of every order is exact,
so the expected result is computed by NumPy in a wide type.  `family` is the family the shape rules give the row under contract = 2,
written here by hand.  Shapes around the tile come from the tile numbers describe() reports (tile_numbers), so the table follows the
tuned tile.  Nothing here imports torch."""
import numpy as np

import strided_jl_amd as S
import window_cases as W
from reduce_exact_cases import pattern

fn = S.fn
F32, F64, C32, C64, I32, I64, BOOL = np.float32, np.float64, np.complex64, np.complex128, np.int32, np.int64, np.bool_
CONTRACT, PART, ALL = "contract", "reduce_part", "reduce_all"


class option:
    """with option("contract", 2): ... sets and restores a library option."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = S.get_option(self.name)
        S.set_option(self.name, self.value)

    def __exit__(self, *a):
        S.set_option(self.name, self.old)


def field(desc, key):
    for tok in desc.split():
        if tok.startswith(key + "="):
            return tok.split("=", 1)[1]
    raise KeyError(key + " not in: " + desc)


def family(desc):
    return field(desc, "family")


def tile_of(desc):
    """(di, TI, dj, TJ, TK) of a CONTRACT plan's describe()."""
    a, b = field(desc, "tile").split("x")
    di, ti = a[1:].split(":")
    dj, tj = b[1:].split(":")
    return int(di), int(ti), int(dj), int(tj), int(field(desc, "k"))


# ---- operands ----------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("col", "trans", "step", "rev", "whole", "whole_trans")


def _window(sub, layout, dt, fill, conj):
    """A view of size `sub` inside a padded parent.  col: column-major; trans: unit stride along the LAST dim; step: stride 2 along
    dim 0; rev: dim 0 reversed; whole / whole_trans: no pads at all (aligned: the vector loads)."""
    N = len(sub)
    perm = tuple(reversed(range(N))) if layout.endswith("trans") else tuple(range(N))
    steps = [1] * N
    if layout == "step":
        steps[0] = 2
    if layout == "rev":
        steps[0] = -1
    pad = not layout.startswith("whole")
    lo = [(1, 2, 1, 2)[i] if pad else 0 for i in range(N)]
    hi = [(2, 1, 3, 1)[i] if pad else 0 for i in range(N)]
    n, strides, off = W.layout(sub, perm, lo, hi, steps)
    root = W.aligned_root(n, dt)
    root[:] = fill(n)
    return S.StridedView(root, tuple(sub), strides, off, "conj" if conj else "identity")


def _expand(v, axes, N):
    """The view as an operand of the N-dim box: size 1 and stride 0 along the dims it does not vary along."""
    size, strides = [1] * N, [0] * N
    for i, d in enumerate(axes):
        size[d], strides[d] = v.size[i], v.strides[i]
    return S.StridedView(v.parent, tuple(size), tuple(strides), v.offset, v.op)


def _poison(dt):
    return True if np.dtype(dt) == np.bool_ else W.poison(dt)


def _is_cx(dt):
    return np.dtype(dt).kind == "c"


def int_values(n, dt, seed, kind="small"):
    """kind small: integers of [-3, 3] (complex: both parts); pm: +-1, +-2, +-0.5 (products stay powers of two); big: Int32 values whose
    products leave Int32; bool: mostly False."""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return pattern(n, 29 + seed, 3 + seed, 11, 0) == 0
    if kind == "pm":
        sgn = np.where(pattern(n, 11 + seed, 1, 5, 0) == 0, -1.0, 1.0)
        e = pattern(n, 7 + seed, 3, 23, 0)
        e = np.where(e == 1, 1, np.where(e == 2, -1, 0))
        v = sgn * np.ldexp(1.0, e) if dt.kind != "i" else sgn
        return v.astype(dt)
    if kind == "big":
        return (pattern(n, 37 + seed, 5 + seed, 7, 3) * 70001 + 13).astype(dt)
    re = pattern(n, 37 + seed, 5 + seed, 7, 3)
    if dt.kind == "c":
        return (re + 1j * pattern(n, 53 + seed, 11 + seed, 7, 2)).astype(dt)
    return re.astype(dt)


F_TABLE = {
    "mul": (lambda a, b: a * b, lambda a, b: a * b),
    "mul3": (lambda a, b, c: a * b * c, lambda a, b, c: a * b * c),
    "ident": (lambda a: a, lambda a: a),
    "dist": (lambda a, b: fn.abs2(a - b), lambda a, b: (a - b) * np.conj(a - b)),
    "plus": (lambda a, b: a + b, lambda a, b: a + b),
    "and": (lambda a, b: a & b, lambda a, b: a & b),
    # not symmetric in its arguments: inputs handed to f in the wrong order, or staged with each other's tile dim, change the result
    "asym": (lambda a, b: a - 2 * b, lambda a, b: a - 2 * b),
}


class Case:
    def __init__(self, name, dims, axes, dts, family, *, layouts=None, conjs=None, f="mul", op="+", values="small", note=""):
        self.name, self.dims, self.axes, self.dts, self.family = name, tuple(dims), tuple(tuple(a) for a in axes), tuple(dts), family
        self.layouts = tuple(layouts or ("col",) * len(axes))
        self.conjs = tuple(conjs or (False,) * len(axes))
        self.fname, self.op, self.values, self.note = f, op, values, note
        self.f, self.npf = F_TABLE[f]

    def __repr__(self):
        return self.name

    @property
    def rdims(self):
        return tuple(d for d in range(len(self.dims)) if d not in self.axes[0])

    def build(self, seed=0):
        """Fresh host operands: (destination, inputs...) as box operands; the destination's parent holds random finite bits, its view
        small integers (the old content)."""
        N = len(self.dims)
        rng = np.random.default_rng([seed, len(self.name)])
        ops = []
        for k, (ax, dt, lay, cj) in enumerate(zip(self.axes, self.dts, self.layouts, self.conjs)):
            sub = [self.dims[d] for d in ax] or [1]  # (a destination of one element: a complete reduction)
            if k == 0:
                v = _window(sub, lay, dt, lambda n: W.finite_bits(rng, n, dt), cj)
                idx = W.element_index(v).ravel()
                old = int_values(idx.size, dt, 5, "pm" if self.op == "*" else "small")
                v.parent[idx] = old
            else:
                v = _window(sub, lay, dt, lambda n: np.full(n, _poison(dt), dtype=dt), cj)
                idx = W.element_index(v).ravel()
                v.parent[idx] = int_values(idx.size, dt, k, "pm" if self.op == "*" else self.values)
            ops.append(_expand(v, ax, N))
        return tuple(ops)

    def expected(self, ops, initop):
        """The destination's parent after the call, computed by NumPy in a wide type (exact on this data)."""
        dest = ops[0]
        ddt = np.dtype(dest.dtype)
        wide = np.complex128 if ddt.kind == "c" else (np.float64 if ddt.kind == "f" else (np.bool_ if ddt == np.bool_ else np.int64))
        ins = [a.toarray() for a in ops[1:]]
        if np.dtype(self.dts[1]) == np.int32 and ddt == np.int64:
            with np.errstate(all="ignore"):
                mapped = np.asarray(self.npf(*ins)).astype(np.int64)  # f in Int32 (it wraps), accumulated in Int64
        else:
            mapped = np.asarray(self.npf(*[x.astype(wide) for x in ins]))
        mapped = np.broadcast_to(mapped, self.dims)
        if self.op is None:  # a map
            out = dest.parent.copy()
            out[W.element_index(dest).ravel()] = (np.conj(mapped) if dest.op == "conj" else mapped).astype(ddt).ravel()
            return out
        red = {"+": np.add, "*": np.multiply, "max": np.maximum, "min": np.minimum, "|": np.logical_or, "&": np.logical_and}[self.op]
        with np.errstate(all="ignore"):
            part = red.reduce(mapped, axis=self.rdims, keepdims=True) if self.rdims else mapped
        old = dest.toarray().astype(wide)
        if initop is None or initop == "identity":
            init = old
        elif initop == "zero":
            init = np.zeros_like(old)
        elif initop == "conj":
            init = np.conj(old)
        elif initop[0] == "scale":
            init = old * wide(initop[1]) if wide != np.bool_ else old
        else:
            init = np.full_like(old, wide(initop[1]))
        with np.errstate(all="ignore"):
            want = red(init, part).astype(ddt)
        if dest.op == "conj":
            want = np.conj(want)
        out = dest.parent.copy()
        out[W.element_index(dest).ravel()] = want.ravel()
        return out

    def call(self, ops, initop):
        S._mapreducedim_(self.f, self.op, initop, self.dims, ops)

    def plan(self, ops, initop="zero"):
        return S.make_plan(self.f, self.op, initop, self.dims, S.promoteshape(self.dims, *ops))


def mismatch(case, got_parent, want_parent, desc=""):
    g = np.ascontiguousarray(got_parent).reshape(-1).view(np.uint8)
    w = want_parent.view(np.uint8)
    if g.size == w.size and np.array_equal(g, w):
        return None
    isz = want_parent.dtype.itemsize
    ne = np.flatnonzero(g[:w.size] != w[:g.size])
    e = int(ne[0]) // isz if ne.size else -1
    return "%s: %d bytes differ, first at parent element %d: got %r want %r | %s" % (
        case.name, ne.size, e, g[e * isz:(e + 1) * isz].view(want_parent.dtype)[0] if e >= 0 else None, want_parent[e] if e >= 0 else None, desc)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
MM = ((0, 1), (0, 2), (1, 2))  # C (m, n), A (m, k), B (n, k)
TYPES = {"f32": (F32, F32, F32), "f64": (F64, F64, F64), "c32": (C32, C32, C32), "c64": (C64, C64, C64), "i64": (I64, I64, I64),
         "i32_i64": (I64, I32, I32), "mixed": (F64, F32, F32)}
BATCH = ((0, 1, 2), (0, 2, 3), (1, 2, 3))  # C (m, n, b), A (m, b, k), B (n, b, k): both inputs vary along the batch dim b
_TILES = {}
# The planner picks the tile by the number of workgroups it gives (64 x 64 from 512 tiles on, else 32 x 32 from 256 on, else 16 x 16),
# so a small problem reaches the larger tiles only through a batch dim, which multiplies the tiles and is never tiled itself.  Per
# tile: (m, n, b) with ragged tiles along both dims (and one whole tile), (m, n, b) for the vector loads -- m and n whole vectors but
# not whole tiles: the operands' strides and the first tile allow 16-byte loads, the other tiles are ragged -- and the box the tile
# numbers are read from.  test_contract_host.py asserts that each of these gets the tile it is listed under.
TILE_SHAPES = {16: ((65, 63), (64, 64)), 32: ((33, 33, 64), (36, 36, 64)), 64: ((65, 65, 128), (68, 68, 128))}


def tile_numbers(tn, tile=16):
    """(TI, TJ, TK) of the plan a problem that gets `tile` x `tile` tiles is given under contract = 2, read from describe()."""
    if (tn, tile) not in _TILES:
        with option("contract", 2):
            kept = (64, 64) if tile == 16 else TILE_SHAPES[tile][0]
            c = Case("probe", kept + (16 if tile == 16 else 4,), MM if tile == 16 else BATCH, TYPES[tn], CONTRACT)
            p = c.plan(c.build())
            d = p.describe()
            p.close()
        assert family(d) == CONTRACT, d
        _, ti, _, tj, tk = tile_of(d)
        assert ti == tile and tj == tile, d
        _TILES[(tn, tile)] = (ti, tj, tk)
    return _TILES[(tn, tile)]


def chunk_rows(tn, tile):
    """Rows that run whole chunks, and more than one, through the 32 x 32 or 64 x 64 tile: k = TK, TK + 1 and 2 TK + 1 on ragged
    problems (one of their tiles is whole: the bounds-free scalar body), 2 TK and 2 TK + 1 on aligned ones with a whole tile (the vector loads
    along the tiled dim and along k, at k0 > 0), and two reduced dims (the outer reduced index advances between chunks)."""
    dts = TYPES[tn]
    tk = tile_numbers(tn, tile)[2]
    ragged, whole = TILE_SHAPES[tile]
    big = "big" if tn == "i32_i64" else "small"
    rows = [Case("%s/t%d_k_2tk+1" % (tn, tile), ragged + (2 * tk + 1,), BATCH, dts, CONTRACT, layouts=("step", "rev", "col"), values=big)]
    if tn not in ("f32", "f64", "c64", "i64"):
        return rows
    rows += [
        Case("%s/t%d_k_tk" % (tn, tile), ragged + (tk,), BATCH, dts, CONTRACT, layouts=("col", "trans", "col")),
        Case("%s/t%d_k_tk+1" % (tn, tile), ragged + (tk + 1,), BATCH, dts, CONTRACT, layouts=("trans", "col", "trans")),
        Case("%s/t%d_vec_2tk" % (tn, tile), whole + (2 * tk,), BATCH, dts, CONTRACT, layouts=("whole", "whole", "whole_trans")),
        Case("%s/t%d_vec_2tk+1" % (tn, tile), whole + (2 * tk + 1,), BATCH, dts, CONTRACT, layouts=("whole", "whole", "whole")),
        Case("%s/t%d_two_reduced" % (tn, tile), ragged + (tk + 1, 2), ((0, 1, 2), (0, 2, 3, 4), (1, 2, 3, 4)), dts, CONTRACT),
    ]
    return rows


def table():
    """Every row, built lazily from the tile numbers."""
    rows = []

    def add(name, dims, axes, dts, fam, **kw):
        rows.append(Case(name, dims, axes, dts, fam, **kw))

    for tn, dts in TYPES.items():
        ti, tj, tk = tile_numbers(tn)
        big = "big" if tn == "i32_i64" else "small"
        # around one tile; whole tiles on aligned parents take the vector loads (both unit-stride axes)
        add("%s/tile" % tn, (ti, tj, tk), MM, dts, CONTRACT, layouts=("whole", "whole", "whole_trans"), values=big)
        add("%s/tile_kfast" % tn, (ti, tj, 2 * tk), MM, dts, CONTRACT, layouts=("whole", "whole_trans", "whole"), values=big)
        add("%s/tile_ragged" % tn, (ti + 1, tj - 1, tk + 1), MM, dts, CONTRACT, layouts=("col", "col", "trans"), values=big)
        # (a reduced extent of 1 is dropped like a kept one: an accumulating map, REDUCE_PART's general form)
        add("%s/k1" % tn, (ti + 1, tj - 1, 1), MM, dts, PART, layouts=("col", "col", "col"))
        add("%s/k_tk-1" % tn, (ti + 1, tj - 1, tk - 1), MM, dts, CONTRACT, layouts=("col", "trans", "col"))
        add("%s/k_tk" % tn, (ti + 1, tj - 1, tk), MM, dts, CONTRACT, layouts=("trans", "col", "trans"))
        add("%s/k_2tk+1" % tn, (ti + 1, tj - 1, 2 * tk + 1), MM, dts, CONTRACT, layouts=("step", "step", "step"))
        add("%s/tile_vec_2tk+1" % tn, (ti, tj, 2 * tk + 1), MM, dts, CONTRACT, layouts=("whole", "whole", "whole"), values=big)
        if tn in ("f32", "f64", "c64", "i64"):  # several chunks per outer reduced index
            add("%s/tile_two_reduced" % tn, (ti + 1, tj - 1, tk + 1, 2), ((0, 1), (0, 2, 3), (1, 2, 3)), dts, CONTRACT)
        add("%s/2x2x1" % tn, (2, 2, 1), MM, dts, PART)
        add("%s/2x2x2" % tn, (2, 2, 2), MM, dts, CONTRACT)
        add("%s/thin_i" % tn, (3, 4 * tj + 2, 5), MM, dts, CONTRACT, layouts=("rev", "col", "rev"))
        add("%s/thin_j" % tn, (4 * ti + 2, 3, 2 * tk + 1), MM, dts, CONTRACT, layouts=("col", "rev", "trans"))
        # a kept extent of 1 drops the dim in canonical form: one input left varying along a kept dim, not this family's shape
        add("%s/m1" % tn, (1, tj, tk), MM, dts, PART)
        add("%s/n1" % tn, (ti, 1, tk), MM, dts, PART)
    for tn in ("f32", "f64", "c64", "i64"):
        dts = TYPES[tn]
        add("%s/two_reduced" % tn, (33, 34, 5, 3), ((0, 1), (0, 2, 3), (1, 2, 3)), dts, CONTRACT)
        add("%s/batch" % tn, (33, 34, 3, 9), ((0, 1, 2), (0, 2, 3), (1, 2, 3)), dts, CONTRACT, layouts=("col", "trans", "col"))
        add("%s/extra_i" % tn, (33, 34, 4, 7), ((0, 1, 2), (0, 2, 3), (1, 3)), dts, CONTRACT)
        # 64 x 64 tiles (4 x 4 outputs per lane) need a grid that fills the device: ragged in both dims
        add("%s/big_tiles" % tn, (1985, 1100, 5), MM, dts, CONTRACT, layouts=("col", "col", "trans"))
        # 32 x 32 tiles (2 x 2 per lane): at least 256 of them, fewer than 512 tiles of 64 x 64
        add("%s/mid_tiles" % tn, (515, 509, 5), MM, dts, CONTRACT, layouts=("col", "col", "trans"))
        add("%s/mid_tiles_vec" % tn, (512, 512, 8), MM, dts, CONTRACT, layouts=("whole", "whole", "whole_trans"))
        add("%s/big_tiles_vec" % tn, (2048, 1024, 4), MM, dts, CONTRACT, layouts=("whole", "whole", "whole_trans"))
    for tile in (32, 64):
        for tn in TYPES:
            rows.extend(chunk_rows(tn, tile))
    for tn in ("f64", "c64", "i64"):
        add("%s/asym" % tn, (35, 33, 17), MM, TYPES[tn], CONTRACT, f="asym", layouts=("col", "trans", "col"))
    for tn in ("c32", "c64"):  # the adjoint / conj / transpose views of tests/cases.py's ALLOPS, and a conj destination
        dts = TYPES[tn]
        add("%s/adjoint" % tn, (33, 34, 9), MM, dts, CONTRACT, layouts=("col", "trans", "trans"), conjs=(False, True, True))
        add("%s/conj" % tn, (33, 34, 9), MM, dts, CONTRACT, layouts=("col", "col", "col"), conjs=(False, True, False))
        add("%s/conj_dest" % tn, (33, 34, 9), MM, dts, CONTRACT, layouts=("trans", "col", "trans"), conjs=(True, False, True))
    add("f64/trans_dest", (33, 34, 9), MM, TYPES["f64"], CONTRACT, layouts=("trans", "col", "col"))
    add("f32/step_dest", (33, 34, 9), MM, TYPES["f32"], CONTRACT, layouts=("step", "col", "col"))
    add("f32/rev_dest", (33, 34, 9), MM, TYPES["f32"], CONTRACT, layouts=("rev", "rev", "col"))
    add("bool/or_and", (37, 35, 19), MM, (BOOL, BOOL, BOOL), CONTRACT, f="and", op="|")
    for op in ("max", "min", "*"):
        add("f32/%s" % op, (35, 33, 17), MM, TYPES["f32"], CONTRACT, op=op)
        add("f64/%s" % op, (35, 33, 17), MM, TYPES["f64"], CONTRACT, op=op, layouts=("col", "trans", "col"))
        add("i64/%s" % op, (35, 33, 17), MM, TYPES["i64"], CONTRACT, op=op)
    add("f32/dist", (35, 33, 17), MM, TYPES["f32"], CONTRACT, f="dist")
    add("f64/minplus", (35, 33, 17), MM, TYPES["f64"], CONTRACT, f="plus", op="min")
    # what the shape rules refuse
    add("refused/three_inputs", (33, 34, 9), ((0, 1), (0, 2), (1, 2), (0, 1, 2)), (F64,) * 4, PART, f="mul3")
    add("refused/both_tile_dims", (33, 34, 9), ((0, 1), (0, 1, 2), (1, 2)), (F64,) * 3, PART)
    add("refused/complete", (33, 34), ((), (0, 1), (0, 1)), (F64,) * 3, PART)  # (a complete reduction of a sub-box: REDUCE_PART's ROW form)
    add("refused/map", (33, 34), ((0, 1), (0,), (1,)), (F64,) * 3, "stream", op=None)
    add("refused/one_input", (33, 34, 9), ((0, 1), (0, 1, 2)), (F64,) * 2, PART, f="ident")
    return rows


def exact_rows():
    """The rows of the family itself (test 1 / A/B of tests/test_gpu_contract.py)."""
    return [c for c in table() if c.family == CONTRACT]
