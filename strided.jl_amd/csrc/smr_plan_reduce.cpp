// smr_plan_reduce.cpp -- planners of FAM_REDUCE_ALL / FAM_REDUCE_PART, and what one execution of such a plan launches (reduce_launch)
#include "smr_plan.h"

namespace smr {

void plan_reduce_all(const Canon& c, ReducePlan& rp) {
    const i64 per_block = REDUCE_ALL_PER_BLOCK;
    i64 nb = (c.total + per_block - 1) / per_block;
    nb = std::max<i64>(1, std::min<i64>(nb, std::max<i64>(1, options().reduce_blocks)));
    rp.nparts = (int)nb;
    if (nb > 1) rp.scratch_bytes = (size_t)nb * dtype_size(c.ct);
}

// What the three forms of REDUCE_PART plan from.  The reduced space is the inner reduced dim NK (extent L0) x the outer index
// q in [0, Q): red = L0 * Q elements per output; es bytes per element of the compute class, vmax elements per 16-byte vector.
struct PartShape {
    i64 red, L0, Q;
    int es, vmax;
};

// COL: a workgroup = TX lanes along kept dim 0 (vmax elements each) x TY rows of the
// reduced space; LDS tree over the rows
static void plan_part_col(const Canon& c, const PartShape& s, ReducePlan& rp) {
    const Options& o = options();
    const i64 red = s.red, L0 = s.L0, K0 = c.dims[0];
    const int vmax = s.vmax, es = s.es;
    rp.kind = 2;
    int txlog = std::min(8, ceil_log2((K0 + vmax - 1) / vmax));
    // rows of the reduced space per workgroup: fewer when the reduction is short (sum over a trailing dim of 7:
    // every lane then walks its 7 rows itself instead of 8 lanes sharing them through LDS)
    txlog = std::min<int>(txlog, std::max<int>((int)o.reduce_col_txlog, 8 - ceil_log2(std::max<i64>(1, red / 8))));
    // too few workgroups along the kept dims: narrower row segments (down to 128 bytes) give 2-4x as many and more
    // rows to each -- when that makes the split unnecessary it saves the partials and the second launch
    // (sum(A; dims=2) of 512x384x64 f32: 16.0 -> 12.4 us, 256^3: 18.4 -> 14.7 us, tools/reduce_sweep.py)
    auto kb_at = [&](int t) { return ((K0 + (((i64)vmax) << t) - 1) / (((i64)vmax) << t)) * (c.nout / K0); };
    const int narrowed_from = txlog;
    if (o.reduce_col_narrow && kb_at(txlog) < o.reduce_part_wgs) {
        int fill = -1;  // the widest segment that still puts a workgroup on every CU (round 6)
        const int t0 = txlog;
        for (int t = txlog - 1; t >= 3 && (((i64)vmax << t) * es >= 128); --t) {
            if ((red >> (8 - t)) < 8) break;  // fewer than 8 rows of the reduced space per lane row
            if (fill < 0 && kb_at(t) >= 256) fill = t;
            if (kb_at(t) >= o.reduce_part_wgs) {
                txlog = t;
                break;
            }
        }
        // no width reaches the target, but one fills the device without a split: the second launch of a split costs more
        // than a thinner first one (sum(A; dims=(3,4)) of (100,90,80,7) Float32: 9000 outputs, 560 rows each: 71 workgroups cut
        // 7 ways + a second pass 8.9 us, 282 workgroups of 8 lanes x 32 rows in one launch: see profiles/r06_sum_cases.txt)
        if (txlog == t0 && fill >= 0 && o.reduce_col_narrow >= 1 && kb_at(t0) < 256) txlog = fill;
    }
    rp.txlog = txlog;
    rp.narrowed = narrowed_from > txlog ? 1 : 0;
    const int tylog = 8 - txlog;
    rp.g0log = std::min(tylog, ceil_log2(L0));
    rp.g1log = tylog - rp.g0log;
    i64 kb = kb_at(txlog);  // workgroups along the kept dims
    i64 rows_per_wg = (i64)1 << tylog, y0 = (i64)1 << rp.g0log, y1 = (i64)1 << rp.g1log;
    // exact lane map (round 6): a row of 100 Float32 is 25 vectors -- 32 lanes leave 22 % of the workgroup idle, 25 lanes x 10
    // rows leave 2 % (and 10 rows = 4000 contiguous bytes per step).  Taken when it fills at least 3 % more lanes; the
    // row may be cut into up to four even segments.  Valid for the vector width assumed here (the launch checks alignment).
    rp.col_tx = 0;
    if (o.reduce_col_exact) {
        bool vdiv = vmax > 1 && K0 % vmax == 0;
        for (int k = 1; k < c.M && vdiv; ++k)
            if (c.strides[k][0] == 1)
                for (int d = 1; d < c.N; ++d)
                    if (c.strides[k][d] % vmax) vdiv = false;
        const i64 vv = vdiv ? vmax : 1;
        const i64 n0v = (K0 + vv - 1) / vv, per2 = vv << txlog, nk2 = (K0 + per2 - 1) / per2;
        double best = (double)K0 / (double)(nk2 * per2);
        i64 btx = 0;
        // (cutting the row into more segments just to put a workgroup on every CU and avoid the split loses: rows of 100 as
        // 4 x 7 lanes x 36 rows, sum over dims (2,4) of (100,90,80,7) Float32 11.4 us against 9.2 with the split)
        for (i64 sg = 1; sg <= 4; ++sg) {
            const i64 tx = (n0v + sg - 1) / sg;
            if (tx > 256 || tx * vv * es < 64 || (tx & (tx - 1)) == 0) continue;
            const i64 ty = 256 / tx;
            if (red < 8 * ty) continue;  // short reductions keep the few-rows rule above
            const double util = (double)n0v / (double)(sg * tx) * (double)(tx * ty) / 256.0;
            if (util > best + 0.03) {
                best = util;
                btx = tx;
                if (util >= 0.9) break;  // the fewest segments that fill the workgroup: longer contiguous pieces per row
            }
        }
        if (btx) {
            rp.col_tx = (int)btx;
            rp.col_v = (int)vv;
            rows_per_wg = 256 / btx;
            // rows along the inner reduced dim: the largest divisor of the row count that it can fill
            y0 = 1;
            for (i64 dv = 1; dv <= rows_per_wg; ++dv)
                if (rows_per_wg % dv == 0 && dv <= std::max<i64>(1, L0)) y0 = dv;
            y1 = rows_per_wg / y0;
            rp.col_y0 = (int)y0;
            rp.col_y1 = (int)y1;
            kb = ((n0v + btx - 1) / btx) * (c.nout / K0);
        }
    }
    i64 split = 1;
    // half the ROW form's target: every workgroup leaves TX*V partials per chunk, and the sweep has 512 ahead of 1024-4096
    const i64 target = std::max<i64>(1, o.reduce_part_wgs / 2);
    if (kb < target && red >= rows_per_wg * 16) split = std::max<i64>(1, std::min<i64>(target / kb, red / (rows_per_wg * 8)));
    split = std::min<i64>(split, 4096);
    // cut the outer reduced index first, the inner reduced dim with what is left (a short Q -- a trailing
    // dim of 7 -- used to forbid any cut but 2 along L0: 160 workgroups for 19 MiB)
    rp.qsplit = (int)even_cut(split, s.Q / y1);
    rp.xsplit = (int)std::max<i64>(1, std::min<i64>(split / rp.qsplit, L0 / (4 * y0)));
    rp.nparts = rp.xsplit * rp.qsplit;
    rp.tr = (int)rows_per_wg;
}

// ROW: G consecutive lanes per output, vector loads along the inner reduced dim
static void plan_part_row(const Canon& c, const PartShape& s, ReducePlan& rp) {
    const Options& o = options();
    const i64 red = s.red, L0 = s.L0, Q = s.Q;
    const int vmax = s.vmax;
    rp.kind = 1;
    int glog = 8;
    // (no floor on the lanes per output -- rounds 1-3 had 16: sum(A; dims=1) of a 3 x N array then ran on 1 lane in 16
    // and took 200 us for 33 MB (now 15.4), of 100 x 50400 f32 7.6 us (now 4.75 with 4 lanes of 6 vectors each), of
    // 32 x 200000 21.5 (now 5.6); tools/reduce_sweep.py, profiles/r03_reduce_sweep.txt)
    const int gfloor = o.reduce_row_floor >= 0 ? (int)o.reduce_row_floor : 0;
    while (glog > gfloor && red < ((i64)vmax << glog) * 4) --glog;
    // a very short inner dim with kept dim 0 right behind it in memory (sum over the channels AND the rows of a
    // 3 x W x H image): lanes along the outputs read neighbouring segments; lanes along the outer reduced index -- what
    // the rule above picks when the whole reduction is long -- would each fetch 12 bytes from a line of their own
    bool dense0 = o.reduce_row_dense && c.NK >= 1 && Q > 1 && c.dims[0] >= 256 && L0 * s.es <= 64;
    for (int k = 1; k < c.M && dense0; ++k)
        if (c.strides[k][c.NK] == 1 && c.strides[k][0] != L0) dense0 = false;
    if (dense0) {
        glog = 8;
        while (glog > 0 && L0 < ((i64)vmax << glog) * 4) --glog;
    }
    rp.g0log = std::min(glog, ceil_log2((L0 + vmax - 1) / vmax));
    rp.g1log = glog - rp.g0log;
    const i64 groups = (c.nout + (256 >> glog) - 1) / (256 >> glog);
    i64 split = 1;
    if (groups < o.reduce_part_wgs && red >= ((i64)vmax << glog) * 16) split = std::max<i64>(1, std::min<i64>(o.reduce_part_wgs / groups, red / (((i64)vmax << glog) * 8)));
    split = std::min<i64>(split, 4096);
    rp.qsplit = (int)even_cut(split, Q >> rp.g1log);
    rp.xsplit = (int)std::max<i64>(1, std::min<i64>(split / rp.qsplit, L0 / (((i64)vmax * 4) << rp.g0log)));
    rp.nparts = rp.xsplit * rp.qsplit;
    rp.tr = 1 << glog;
}

// general form: lanes cooperating per output: more when few outputs / long reductions
int reduce_part_general_lanes(const Canon& c, i64 red) {
    int tr = 1;
    // the inputs' fastest-varying dim is a reduced one -> lanes along it coalesce
    bool red_fast = false;
    for (int k = 1; k < c.M; ++k)
        for (int i = c.NK; i < c.N; ++i)
            if (std::llabs(c.strides[k][i]) == 1) red_fast = true;
    if (red_fast || c.nout < 256 * 256) {
        while (tr < 256 && tr * 2 <= red && (tr < 64 || c.nout * tr < 256 * 1024)) tr <<= 1;
    }
    if (red_fast && tr < 16 && red >= 16) tr = 16;
    return tr;
}

static void plan_part_general(const Canon& c, const PartShape& s, ReducePlan& rp) {
    const i64 red = s.red;
    rp.kind = 0;
    const int tr = reduce_part_general_lanes(c, red);
    rp.tr = tr;
    // few destination elements, long reductions: cut the reduced range so that ~2048
    // workgroups are in flight, partials folded by a second launch (also keeps the
    // serial per-lane accumulation short, which is what bounds the rounding error)
    const i64 groups = (c.nout + (256 / tr) - 1) / (256 / tr);
    i64 split = 1;
    if (groups < 1024 && red >= (i64)tr * 256) {
        split = std::min<i64>(2048 / std::max<i64>(1, groups), red / ((i64)tr * 64));
        split = std::max<i64>(1, std::min<i64>(split, 4096));
    }
    rp.nparts = (int)split;
}

void plan_reduce_part(const Canon& c, ReducePlan& rp) {
    PartShape s;
    s.es = dtype_size(c.ct);
    s.vmax = std::max(1, 16 / s.es);
    s.red = c.total / std::max<i64>(1, c.nout);
    // no reduced dim at all (an accumulating map, dest[I] = op(dest[I], f(...)), over up to MAXN kept
    // dims): nothing to index at position NK -- the general form handles it
    const bool nored = c.NK >= c.N;
    s.L0 = nored ? 1 : c.dims[c.NK];  // inner reduced dim
    s.Q = s.red / s.L0;               // outer reduced index (dims NK+1..)
    // which vectorisable form applies?
    bool row = !nored && inputs_run_along(c, c.NK);
    bool col = !nored && c.strides[0][0] == 1 && inputs_run_along(c, 0);
    const i64 force = options().reduce_part_kind;
    if (force >= 0) {  // tuning / testing override
        row = row && force == 1;
        col = col && force == 2;
    }
    if (col) plan_part_col(c, s, rp);
    else if (row) plan_part_row(c, s, rp);
    else plan_part_general(c, s, rp);
    if (rp.nparts > 1) rp.scratch_bytes = (size_t)c.nout * (size_t)rp.nparts * s.es;  // chunk partials
}

// operand k's element-offset base (as make_optab computes it) is 16-byte aligned
static bool aligned16(const Canon& c, void* const* bases, int k) {
    const uintptr_t b = (uintptr_t)(bases ? bases[c.orig[k]] : c.base[k]) + (uintptr_t)(c.offsets[k] * (i64)c.esize[k]);
    return b % 16 == 0;
}

bool reduce_all_vector(const Canon& c, void* const* bases) {
    const int es = dtype_size(c.ct);
    const int vmax = es >= 16 ? 1 : 16 / es;
    // one fused dim, every input unit stride / broadcast, 16-B aligned
    bool vec = !c.mixed && vmax > 1 && c.N == 1 && (c.total % vmax == 0) && c.total >= REDUCE_ALL_PER_BLOCK;
    for (int k = 1; k < c.M && vec; ++k) {
        if (c.strides[k][0] == 0) continue;
        if (c.strides[k][0] != 1) vec = false;
        if (!aligned16(c, bases, k)) vec = false;
    }
    return vec;
}

RedLaunch reduce_launch(const Plan& plan, void* const* bases, bool have_scratch) {
    const Canon& c = plan.c;
    RedLaunch r;
    const int es = dtype_size(c.ct);
    const i64 rs = options().reduce_single;
    if (plan.family == FAM_REDUCE_ALL) {
        int blocks = plan.red.nparts;
        if (blocks > 1 && !have_scratch) blocks = 1;
        r.nparts = blocks;
        // up to 64 partials are folded inside the launch (1 MiB: 4.9 -> 4.1 us; tools/reduce_all_sweep.py) -- the arrivals of ONE
        // counter serialise, so larger reductions keep the second launch (8 MiB with 256 workgroups: 6.6 vs 5.4 us)
        const bool single = blocks > 1 && rs > 0 && blocks <= std::max<i64>(rs, REDUCE_FOLD_MAX);
        r.fold = blocks == 1 ? RED_FOLD_EPILOGUE : (single ? RED_FOLD_IN_LAUNCH : RED_FOLD_SECOND_LAUNCH);
        r.vec = reduce_all_vector(c, bases) ? 16 / es : 1;
        return r;
    }
    if (plan.family != FAM_REDUCE_PART) return r;
    const int nsplit = (plan.red.nparts > 1 && have_scratch) ? plan.red.nparts : 1;
    r.nparts = nsplit;
    const int vmax = (c.mixed || es >= 16) ? 1 : 16 / es;
    if (plan.red.kind == 0) {
        const int ob = 256 / plan.red.tr;
        r.groups = (c.nout + ob - 1) / ob;
    } else {
        // vector width: the vector axis must divide, every vector-loaded operand must be aligned
        const int vax = plan.red.kind == 1 ? c.NK : 0;  // axis the vectors run along
        bool vec = vmax > 1 && (c.dims[vax] % vmax == 0);
        for (int k = 1; k < c.M && vec; ++k) {
            if (c.strides[k][vax] != 1) continue;
            if (!aligned16(c, bases, k)) vec = false;
            for (int d = 0; d < c.N; ++d)
                if (d != vax && (c.strides[k][d] % vmax)) vec = false;
        }
        r.vec = vec ? vmax : 1;
        if (plan.red.kind == 1) {
            const int ob = 256 >> (plan.red.g0log + plan.red.g1log);
            r.groups = (c.nout + ob - 1) / ob;
        } else {
            r.ctx = 1 << plan.red.txlog;
            r.cty = 256 >> plan.red.txlog;
            r.cy0 = 1 << plan.red.g0log;
            r.cy1 = 1 << plan.red.g1log;
            if (plan.red.col_tx > 0 && plan.red.col_v == r.vec) {  // exact lane map (plan_part_col), planned for this vector width
                r.ctx = plan.red.col_tx;
                r.cty = 256 / r.ctx;
                r.cy0 = plan.red.col_y0;
                r.cy1 = plan.red.col_y1;
            }
            const i64 per = (i64)r.vec * r.ctx;
            r.groups = ((c.dims[0] + per - 1) / per) * (c.nout / c.dims[0]);
        }
    }
    const bool single = nsplit > 1 && nsplit <= rs && r.groups <= RED_COUNTERS;
    r.fold = nsplit == 1 ? RED_FOLD_EPILOGUE : (single ? RED_FOLD_IN_LAUNCH : RED_FOLD_SECOND_LAUNCH);
    return r;
}

}  // namespace smr
