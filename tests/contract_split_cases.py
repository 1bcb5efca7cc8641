"""Case table of the CONTRACT family's split form (tests/test_contract_split_host.py, tests/test_gpu_contract_split.py).

Every row is a Case of tests/contract_cases.py (windowed operands in poisoned parents, integer-valued data on which every
accumulation order is exact, the destination's whole parent compared byte for byte) planned under contract = 2 with a FORCED tile
("contract_tile") and a FORCED number of slices ("contract_split" = S >= 2).  The reduced extents come from the tile numbers
describe() reports (TK), so each row is the smallest shape at which its mechanism can go wrong:

  K = 2 TK, S = 2         one whole chunk per slice; whole tiles on aligned parents: the vector loads, k0 > 0 at a slice start
  K = 3 TK + 1, S = 2     cps = 2: unequal slices, the last chunk of the last slice is one row
  K = 3 TK + 1, S = 4, 64 one chunk per slice; a forced S above the chunks clamps to 4
  K = 5 TK, S = 3         cps = 2, 3 slices, the last one short
  (TK + 1, 3), S = 2, 3   two reduced dims: 2 chunks per q, 6 in all: S = 2 starts its second slice inside a q (kc != 0), S = 3 at q boundaries

Nothing here imports torch."""
import contract_cases as CC

TILES = (16, 32, 64)


class split_options:
    """with split_options(tile, S): contract = 2, the tile and the slices forced; restored on exit."""

    def __init__(self, tile, S, contract=2):
        self.opts = [CC.option("contract", contract), CC.option("contract_tile", tile), CC.option("contract_split", S)]

    def __enter__(self):
        for o in self.opts:
            o.__enter__()

    def __exit__(self, *a):
        for o in reversed(self.opts):
            o.__exit__(*a)


class SplitCase(CC.Case):
    """A Case with its forced tile and slices; the expected result is Case.expected."""

    def __init__(self, name, dims, axes, dts, tile, S, **kw):
        CC.Case.__init__(self, name, dims, axes, dts, CC.CONTRACT, **kw)
        self.tile, self.S = tile, S

    def options(self):
        return split_options(self.tile, self.S)

    def describe(self, ops=None, initop="zero"):
        with self.options():
            p = self.plan(ops if ops is not None else self.build(), initop)
            d = p.describe()
            p.close()
        return d


def slices(desc):
    """(kparts, cps, scratch) of a describe() string; (1, 0, 0) for an unsplit plan."""
    if "kparts=" not in desc:
        return 1, 0, 0
    return int(CC.field(desc, "kparts")), int(CC.field(desc, "cps")), int(CC.field(desc, "scratch"))


def _kept(tile, whole=False):
    return ((64, 64) if whole else (65, 63)) if tile == 16 else CC.TILE_SHAPES[tile][1 if whole else 0]


def _axes(tile, nred=1):
    if tile == 16:
        return CC.MM if nred == 1 else ((0, 1), (0, 2, 3), (1, 2, 3))
    return CC.BATCH if nred == 1 else ((0, 1, 2), (0, 2, 3, 4), (1, 2, 3, 4))


_TABLE = []


def table():
    if _TABLE:
        return _TABLE
    rows = _TABLE

    def add(name, tile, S, red, tn, whole=False, **kw):
        dts = kw.pop("dts", None) or CC.TYPES[tn]
        rows.append(SplitCase("%s/t%d/%s" % (tn, tile, name), _kept(tile, whole) + tuple(red), _axes(tile, len(red)), dts, tile, S, **kw))

    for tile in TILES:
        for tn in CC.TYPES:
            tk = CC.tile_numbers(tn, tile)[2]
            big = "big" if tn == "i32_i64" else "small"
            cx = tn in ("c32", "c64")
            add("2tk_s2_vec", tile, 2, (2 * tk,), tn, whole=True, layouts=("whole", "whole", "whole_trans"), values=big)
            add("2tk_s2_vec_kfast", tile, 2, (2 * tk,), tn, whole=True, layouts=("whole", "whole_trans", "whole"), values=big)
            add("2tk_s2", tile, 2, (2 * tk,), tn, layouts=("col", "trans", "col"), values=big)
            add("3tk+1_s2", tile, 2, (3 * tk + 1,), tn, layouts=("step", "rev", "col"), values=big,
                conjs=(True, False, True) if cx else None)
            add("3tk+1_s4", tile, 4, (3 * tk + 1,), tn, layouts=("trans", "col", "trans"), values=big)
            add("3tk+1_s64", tile, 64, (3 * tk + 1,), tn, layouts=("col", "col", "rev"), values=big,
                conjs=(False, True, False) if cx else None)
            add("5tk_s3", tile, 3, (5 * tk,), tn, layouts=("rev", "step", "trans"), values=big)
            add("5tk_s3_vec", tile, 3, (5 * tk,), tn, whole=True, layouts=("whole", "whole_trans", "whole_trans"), values=big)
            add("two_s2", tile, 2, (tk + 1, 3), tn, values=big)
            add("two_s3", tile, 3, (tk + 1, 3), tn, layouts=("trans", "col", "col"), values=big, conjs=(False, True, True) if cx else None)
    # further rows: every other op, other f, on the smallest tile (the op switch and f are the tile body's, whatever the tile)
    tk32, tk64 = CC.tile_numbers("f32", 16)[2], CC.tile_numbers("f64", 16)[2]
    # (the product's values are powers of two: few of them, over two reduced dims -- one chunk per outer reduced index, three in all)
    for op in ("max", "min", "*"):
        add(op, 16, 3, (5, 3) if op == "*" else (2 * tk32 + 1,), "f32", op=op)
        add(op, 16, 3, (5, 3) if op == "*" else (2 * tk64 + 1,), "f64", op=op, layouts=("col", "trans", "col"))
        add(op, 16, 3, (5, 3) if op == "*" else (2 * tk64 + 1,), "i64", op=op)
    tkb = CC.tile_numbers("i64", 16)[2]
    add("or_and", 16, 3, (2 * tkb + 3,), "bool", dts=(CC.BOOL,) * 3, f="and", op="|")
    add("and_and", 16, 3, (2 * tkb + 3,), "bool", dts=(CC.BOOL,) * 3, f="and", op="&")
    for tile in TILES:
        add("dist", tile, 3, (2 * CC.tile_numbers("f32", tile)[2] + 1,), "f32", f="dist", layouts=("col", "trans", "col"))
        add("asym", tile, 2, (2 * CC.tile_numbers("f64", tile)[2] + 1,), "f64", f="asym", layouts=("col", "trans", "col"))
    add("dist", 16, 2, (2 * CC.tile_numbers("c64", 16)[2] + 1,), "c64", f="dist")
    add("dist", 16, 2, (2 * tkb + 1,), "i64", f="dist")
    return rows


def by_name():
    return {c.name: c for c in table()}
