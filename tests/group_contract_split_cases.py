"""Deterministic table of SPLIT CONTRACTION GROUPS (tests/test_group_contract_split_host.py, tests/test_gpu_group_contract_split.py).

A row is a group_contract_cases.Row -- members that are contract_cases.Case: windowed operands in poisoned parents, integer-valued
data on which every accumulation order is exact, whole destination parents compared byte for byte -- with a FORCED tile (option
"group_contract_tile") and a FORCED number of slices (option "group_contract_split" = S >= 2).  The reduced extents come from the
tile numbers describe() reports (TK), so each member is the smallest shape at which its mechanism can go wrong:

  K = 2 TK, S = 2           one whole chunk per slice; whole tiles on aligned parents: the vector loads, k0 > 0 at a slice start
  K = 3 TK + 1, S = 2       cps = 2: unequal slices, the last chunk of the last slice is one row
  K = 3 TK + 1, S = 4, 64   one chunk per slice; a forced S above the chunks clamps to 4
  K = 5 TK, S = 3           cps = 2, 3 slices, the last one short
  (TK + 1, 3), S = 2, 3     two reduced dims: 2 chunks per q, 6 in all: S = 2 starts its second slice inside a q, S = 3 at q boundaries
  K <= TK                   a single chunk: the member stays UNSPLIT (S_i = 1) inside a split group -- first, last and in between

Kept extents are whole tiles (T x T) and ragged ones (T + 1 x T - 1); some members carry a batch dim, so one group holds members of
different rank.  Nothing here imports torch."""
import numpy as np

import contract_cases as CC
import group_contract_cases as GC

TILES = (16, 32)
MM, BATCH, TWO_RED = CC.MM, CC.BATCH, GC.TWO_RED
TYPES = {tn: CC.TYPES[tn] for tn in ("f32", "f64", "c32", "c64", "i64")}
INITOPS = ("zero", "none", "scale", "const", "conj")


class split_option:
    """with split_option(S): "group_contract_split" set and restored."""

    def __init__(self, S):
        self.opt = CC.option("group_contract_split", S)

    def __enter__(self):
        self.opt.__enter__()

    def __exit__(self, *a):
        self.opt.__exit__(*a)


class Row(GC.Row):
    """A group_contract_cases.Row with its forced slices; `kind` may also be "conj" (the initop that conjugates the old value)."""

    def __init__(self, name, tn, dts, specs, kind, tile, S, **kw):
        GC.Row.__init__(self, name, tn, dts, specs, kind, tile, **kw)
        self.S = S
        self.needs_prog = self.needs_prog or tn == "i32_i64"

    def initop(self, i):
        return "conj" if self.kind == "conj" else GC.Row.initop(self, i)

    def expected(self, built):
        """Row.expected; for max / min over real floats with the sign of a zero result as the library defines it (Julia's: max(-0.0,
        0.0) is 0.0 and min is -0.0, whatever the order -- NumPy keeps whichever comes first, and products like -3 * 0.0 are -0.0)."""
        if self.op not in ("max", "min") or np.dtype(self.dts[0]).kind != "f":
            return GC.Row.expected(self, built)
        red = np.maximum if self.op == "max" else np.minimum
        below = np.nextafter(0.0, -1.0)   # stands for -0.0 while comparing: the data is integer-valued, nothing else is that small

        def down(x):
            return np.where((x == 0) & np.signbit(x), below, x)

        out = []
        for i, (c, ops) in enumerate(zip(self.members, built)):
            A, B = (x.toarray().astype(np.float64) for x in ops[1:])
            part = red.reduce(down(np.broadcast_to(A, c.dims) * np.broadcast_to(B, c.dims)), axis=c.rdims, keepdims=True)
            old, initop = ops[0].toarray().astype(np.float64), self.initop(i)
            init = old if initop is None else (np.zeros_like(old) if initop == "zero" else (old * initop[1] if initop[0] == "scale" else np.full_like(old, initop[1])))
            res = red(down(init), part)
            w = ops[0].parent.copy()
            w[GC.W.element_index(ops[0]).ravel()] = np.where(res == below, -0.0, res).astype(w.dtype).ravel()
            out.append(w)
        return out

    def group(self, built, independent=False, stream=0, S=None):
        with split_option(self.S if S is None else S):
            return GC.Row.group(self, built, independent, stream)

    def chunks(self, built):
        """Per member the chunks Q * nkc of its walk and its tiles on the row's tile, from the member's single plan under contract = 2
        and the forced tile: describe() lists the canonical extents (kept dims first, the inner reduced dim first among the reduced)."""
        out = []
        with CC.option("contract", 2), CC.option("contract_tile", self.tile):
            for i, (c, ops) in enumerate(zip(self.members, built)):
                p = c.plan(ops, self.initop(i))
                d = p.describe()
                p.close()
                assert CC.family(d) == CC.CONTRACT and CC.tile_of(d)[1] == self.tile, d
                cdims = [int(x) for x in CC.field(d, "dims").split("x")]
                red = cdims[len(cdims) - len(c.rdims):]
                tk = CC.tile_of(d)[4]
                out.append((int(np.prod(red[1:], dtype=np.int64)) * -(-red[0] // tk), int(CC.field(d, "grid"))))
        return out


def cut(nchunks, want):
    """contract_cut in Python: (S, cps); (1, nchunks) when the walk is not cut."""
    S = min(want, nchunks)
    if S < 2:
        return 1, nchunks
    cps = -(-nchunks // S)
    S = -(-nchunks // cps)
    return (S, cps) if S >= 2 else (1, nchunks)


# ---- members -------------------------------------------------------------------------------------------------------------------------
def _whole(t, red, lay=("whole", "whole", "whole_trans")):
    return ((t, t) + tuple(red), MM if len(red) == 1 else TWO_RED, lay, None)


def _ragged(t, red, lay=("col", "trans", "col")):
    return ((t + 1, t - 1) + tuple(red), MM if len(red) == 1 else TWO_RED, lay, None)


def _batch(t, k, lay=("col", "trans", "col")):
    return ((t + 1, t - 1, 3, k), BATCH, lay, None)


def _small(i):
    """A single-chunk member: it stays unsplit."""
    return GC._mm((15, 2, 17, 3)[i % 4], (2, 15, 5, 16)[i % 4], (2, 1 + i % 3 + 1, 3, 2)[i % 4], GC.LAYOUTS[i % 5])


def members_3tk1(t, tk):
    return [_ragged(t, (3 * tk + 1,), ("step", "rev", "col")), _batch(t, 3 * tk + 1), _whole(t, (3 * tk + 1,), ("whole", "whole", "whole"))]


def members_mixed(t, tk, count):
    """Unsplit members first, last and between split ones; ranks 3 and 4 in one group."""
    core = [_small(0), _ragged(t, (5 * tk,), ("rev", "step", "trans")), _small(1), _ragged(t, (tk + 1, 3)), _whole(t, (5 * tk,), ("whole", "whole_trans", "whole_trans")),
            _small(2), _batch(t, 2 * tk), _whole(t, (2 * tk,)), _ragged(t, (3 * tk + 1,), ("trans", "col", "trans")), _small(3)]
    i = 0
    while len(core) < count:
        core.insert(len(core) - 1, _small(4 + i) if i % 2 else _ragged((16, 32)[i % 4 == 0], ((2 * tk, 3 * tk + 1, tk + 1)[i % 3],), GC.LAYOUTS[i % 5]))
        i += 1
    return core[:count - 1] + [core[-1]]


_TABLE = []


def table():
    if _TABLE:
        return _TABLE
    rows = _TABLE
    n = 0

    def add(name, tn, specs, tile, S, kind=None, dts=None, **kw):
        nonlocal n
        kind = kind or INITOPS[n % 5]
        if kind == "conj" and tn not in ("c32", "c64"):
            kind = "scale"
        n += 1
        rows.append(Row("%s/t%d/%s" % (tn, tile, name), tn, dts or TYPES[tn], specs, kind, tile, S, **kw))

    for ti, tile in enumerate(TILES):
        for ni, tn in enumerate(TYPES):
            tk = GC.tk_of(tn)
            cx = tn in ("c32", "c64")
            add("n1_2tk_s2_vec", tn, [_whole(tile, (2 * tk,))], tile, 2)
            s = (2, 4, 64)[(ni + ti) % 3]
            specs = members_3tk1(tile, tk)
            add("n3_3tk+1_s%d" % s, tn, GC.with_conj(specs, (True, False, True)) if cx else specs, tile, s)
            specs = [_small(0), _ragged(tile, (tk + 1, 3)), _whole(tile, (2 * tk,), ("whole", "whole_trans", "whole")), _small(1)]
            add("n4_two_s2", tn, specs, tile, 2)
            specs = members_mixed(tile, tk, 17)
            add("n17_mixed_s3", tn, GC.with_conj(specs, (False, True, False)) if cx and tile == 32 else specs, tile, 3)
    tk = GC.tk_of("f64")
    for tile in TILES:  # every forced S on the three-member row, for one type
        for s in (2, 4, 64):
            add("n3_3tk+1_s%d_all" % s, "f64", members_3tk1(tile, tk), tile, s, kind=("none", "scale", "zero")[s % 3])
    # search depth: 257 tiny members of two chunks each, a single-chunk one every 16th
    tiny = [GC._mm((2, 15, 17)[i % 3], (15, 2, 16)[i % 3], 2 if i % 16 == 5 else tk + 1, GC.LAYOUTS[i % 5]) for i in range(257)]
    add("n257_tiny_s2", "f64", tiny, 16, 2, kind="scale")
    # converting operands, Bool, the other ops, other f (runtime-compiled, and interpreted under jit = 0)
    tki = GC.tk_of("i32_i64")
    # (rows whose f is a program compile a kernel per body and tile: one tile each keeps them at a few seconds)
    rows.append(Row("i32_i64/t16/n3_3tk+1_s2", "i32_i64", CC.TYPES["i32_i64"], members_3tk1(16, tki), "scale", 16, 2))
    tkb = GC.tk_of("bool")
    bool_specs = [_small(0), _ragged(16, (2 * tkb + 3,)), _batch(16, tkb + 1), _small(3)]
    rows.append(Row("bool/t16/n4_or_and_s3", "bool", GC.BOOL3, bool_specs, "none", 16, 3, f="and", op="|"))
    rows.append(Row("bool/t16/n4_and_and_s2", "bool", GC.BOOL3, bool_specs, "zero", 16, 2, f="and", op="&"))
    for op in ("max", "min", "*"):
        for tn, tile in (("f32", 16), ("f64", 32), ("i64", 16)):
            tk = GC.tk_of(tn)
            red = (5, 3) if op == "*" else (2 * tk + 1,)   # (the product's values are powers of two: few of them, one chunk per q)
            # (the unsplit member's K = 17 is that of contract_cases' op rows: long enough that no output's max / min is a zero of either sign)
            specs = [_ragged(tile, red), ((17, 5, 3 if op == "*" else 17), MM, ("col", "col", "col"), None), _whole(tile, red, ("col", "col", "col"))]
            rows.append(Row("%s/t%d/n3_%s_s3" % (tn, tile, op), tn, TYPES[tn], specs, ("none", "scale", "const")[n % 3], tile, 3, op=op))
            n += 1
    for tn, tile, kind in (("f32", 16, "none"), ("c64", 32, "scale")):
        tk = GC.tk_of(tn)
        specs = [_small(1), _ragged(tile, (2 * tk + 1,)), _batch(tile, 3 * tk + 1), _small(0)]
        rows.append(Row("%s/t%d/n4_dist_s3" % (tn, tile), tn, TYPES[tn], specs, kind, tile, 3, f="dist"))
    rows.append(Row("f64/t16/n4_asym_s2", "f64", TYPES["f64"], [_small(1), _ragged(16, (2 * GC.tk_of("f64") + 1,)), _whole(16, (GC.tk_of("f64") + 1, 3), ("col", "col", "col")), _small(0)],
                    "scale", 16, 2, f="asym"))
    return rows


def row(name):
    return {r.name: r for r in table()}[name]
