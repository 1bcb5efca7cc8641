// smr_plan.cpp -- host-side planner of libstrided_hip.so.
//
// GPU analogue of the reference's planning chain
//   _mapreduce_fuse!  (src/mapreduce.jl:98-117)   -> canonicalise(): drop/sort/flip/fuse/dedupe
//                                                    (smr_canon.cpp, with the f-program checks)
//   _mapreduce_order! (src/mapreduce.jl:119-139)  -> canonical dim order (destination-stride
//                                                    sorted) + kernel-family classification
//   _mapreduce_block!/_computeblocks (:142-180, :452-500)
//                                                 -> plan_tiles(): LDS tile shape instead of
//                                                    L1 cache blocks (smr_plan_tiled.cpp)
// The CPU heuristics (importance digits, 32 KiB blocks, 64 B lines) are NOT transliterated:
// on CDNA4 the quantities that matter are the unit-stride axis of every operand (coalescing),
// the LDS budget and the number of workgroups.  The faithful restatement of the CPU planner
// lives in oracle/ as test infrastructure.
// Here: family selection (make_plan), STREAM, describe(); the other families' planners are in smr_plan_<family>.cpp.
#include <cstdarg>
#include <cstdio>

#include "smr_plan.h"

namespace smr {

// ---- helpers shared by the family planners -----------------------------------------------------------
// bytes per element as the kernels move them: the operands' own for a bit copy, else the compute class's
int elem_bytes(const Canon& c) { return c.bitcopy ? c.esize[0] : dtype_size(c.ct); }

// ceil(log2(v)); 0 for v <= 1
int ceil_log2(i64 v) {
    int l = 0;
    while (((i64)1 << l) < v) ++l;
    return l;
}

// number of chunks an index range of `n` is cut into when about `want` are asked for: all of n when that is
// within 2x (a trailing dim of 7 cut 6 ways would leave chunks of 2,2,2,1 and two idle workgroups), else a
// count that leaves no chunk empty
i64 even_cut(i64 want, i64 n) {
    if (n <= 1 || want <= 1) return 1;
    if (n <= 2 * want) return n;
    const i64 per = (n + want - 1) / want;
    return (n + per - 1) / per;
}

// is every operand k >= k0 (0: the destination too, 1: the inputs) unit-stride or broadcast along dim d?
bool unit_or_bcast(const Canon& c, int d, int k0) {
    for (int k = k0; k < c.M; ++k)
        if (c.strides[k][d] != 1 && c.strides[k][d] != 0) return false;
    return true;
}

// ... every input, and at least one of them unit-stride: vector loads can run along dim d
bool inputs_run_along(const Canon& c, int d) {
    bool any = false;
    for (int k = 1; k < c.M; ++k) any = any || c.strides[k][d] == 1;
    return any && unit_or_bcast(c, d, 1);
}

// ---- STREAM -----------------------------------------------------------------------------------------
// Admission: every operand is unit-stride or broadcast along dim 0 -- and, unless the family is forced, rows long enough to
// keep a workgroup busy.
static bool stream_fits(const Canon& c, bool forced) {
    if (!unit_or_bcast(c, 0, 0)) return false;
    if (forced || c.N < 2) return true;
    // short rows pack (256 >> txlog) entries of dim 1 into a workgroup; when dim 1 is short too (a permutation
    // of a 4x4x4x... tensor) most lanes idle -- 8 of 256 for rows of 4 Float64 x 4 -- and the per-element
    // decode of the GENERIC family wins (measured 4^8 Float64: 9.9 us -> tools/perf_sanity.py)
    const i64 vmax = std::max<i64>(1, 16 / elem_bytes(c));
    const i64 n0v = (c.dims[0] % vmax == 0) ? c.dims[0] / vmax : c.dims[0];
    if (n0v > 128) return true;
    const i64 used = n0v * std::min<i64>(c.dims[1], (i64)256 >> ceil_log2(n0v));
    return used * 4 >= 256;
}

static void plan_stream(const Canon& c, StreamPlan& sp) {
    const int es = elem_bytes(c);
    const int vmax = (c.mixed || es >= 16) ? 1 : 16 / es;
    const bool unit = unit_or_bcast(c, 0, 0);  // (false: the strided form, element accesses)
    // vector width: 16 B per lane when every unit-stride operand stays 16-B aligned
    int v = unit ? vmax : 1;
    while (v > 1) {
        bool ok = c.dims[0] % v == 0;
        for (int k = 0; k < c.M && ok; ++k) {
            if (c.strides[k][0] == 0) continue;
            if (((uintptr_t)c.base[k] + (uintptr_t)(c.offsets[k] * c.esize[k])) % (size_t)(v * es)) ok = false;
            for (int i = 1; i < c.N && ok; ++i)
                if (c.strides[k][i] % v) ok = false;
        }
        if (ok) break;
        v >>= 1;
    }
    sp.vec = v;
    sp.vec_ua = false;
    // Round 5: rows that are not whole aligned vectors (odd lengths, odd row strides, views starting inside a vector) still move
    // as 16-byte vectors -- at element alignment, plus one partial vector per row (smr_k_stream.hip: UVec) -- when the elements
    // are 4 or 8 bytes and a row holds at least four vectors.
    // (short rows with a long tail lose: rows of 63 Float32 = 15 vectors + 3 single elements 24.9 -> 27.1 us; rows of 17
    // Float64 = 8 vectors + 1 element gain 9 %: a tail of one element, or at least 32 vectors per row.  tools/stream_ua_ab.py,
    // profiles/r05_stream_ua_ab.txt: (257,129,65) (0,2,1) 12.3 -> 9.5 us, (999,1001) axpy 4.7 -> 3.1 us, (1001,999,5) f32 10.9 -> 8.0)
    if (options().stream_ua && v < vmax && unit && es >= 4 && c.dims[0] >= 4 * vmax && (c.dims[0] % vmax <= 1 || c.dims[0] >= 32 * vmax)) {
        sp.vec = vmax;
        sp.vec_ua = true;
    }
}

// ---- family selection -------------------------------------------------------------------------------
// make_plan only selects: canonicalise, decide the family, call that family's planner (plan_flatb / plan_flat / plan_flat2,
// plan_tiles, plan_orbit, plan_stream, plan_reduce_all / plan_reduce_part, plan_contract; GENERIC has nothing to plan), describe.
int make_plan(const smr_problem* p, Plan& plan) {
    int rc = canonicalise(p, plan.c);
    if (rc) return rc;
    const Canon& c = plan.c;
    const Options& o = options();
    int fam = FAM_GENERIC;
    plan.flat2.on = false;
    plan.flatb.on = false;
    // FLAT: the one-sided form first -- unless its line side is under 8 elements long, where the two-sided form's bigger tiles win
    // (ComplexF64 (6,64,64,64,5) reversed 94 -> 40 us, (4,300,300,3) 16.5 -> 7.6; with 24-element lines the one-sided form's
    // vector accesses are 1.5x ahead; profiles/r03_flat2_ab.txt).  flat2 = 2: the two-sided form wherever it applies (experiments)
    // force_family = FAM_FLAT (tests, experiments) tries the FLAT planners like the default does and leaves the rest of the decision alone
    bool flat_ok = c.redop == SMR_RED_NONE && (o.force_family == 0 || o.force_family == FAM_FLAT);
    // plan_orbit builds the orbit list: run it once per plan, whoever asks first
    int orbit_state = -1;
    auto orbit_ok = [&]() {
        if (orbit_state < 0) orbit_state = plan_orbit(c, plan.orbit) ? 1 : 0;
        return orbit_state == 1;
    };
    // several inputs that are permuted views of ONE buffer: the orbit kernel reads the buffer once, the n-ary FLAT forms would read it per view
    if (flat_ok && c.M > 2 && o.force_family == 0 && orbit_ok()) flat_ok = false;
    if (flat_ok && plan_flatb(c, plan.flatb)) {
        plan.family = FAM_FLAT;
        describe(plan);
        return SMR_OK;
    }
    const bool one = flat_ok && plan_flat(c, plan.flat);
    const bool two_first = flat_ok && (o.flat2 >= 2 || !one || (!plan.flat.fuse && !plan.flat.lshare && c.dims[plan.flat.q] < 8));
    if (two_first && plan_flat2(c, plan.flat2)) {
        fam = FAM_FLAT;
    } else if (one) {
        fam = FAM_FLAT;
    } else if (c.redop == SMR_RED_NONE) {
        const bool forced = o.force_family == FAM_STREAM, stream = stream_fits(c, forced);
        bool transposed = false;  // (short_dim0_transposition: such inputs are staged like transposed ones)
        for (int k = 1; k < c.M; ++k) transposed = transposed || short_dim0_transposition(c, k, elem_bytes(c));
        if (stream && !forced && transposed && plan_tiles(c, plan.tile)) {
            fam = FAM_TILED;
        } else if (stream) {
            fam = FAM_STREAM;
        } else if (o.force_family != FAM_TILED && o.force_family != FAM_GENERIC && orbit_ok()) {
            fam = FAM_ORBIT;
        } else if (plan_tiles(c, plan.tile)) {
            fam = FAM_TILED;
        } else if (c.dims[0] >= 64) {
            // strided along dim 0 (A[1:2:end, :], a destination that is itself a strided view):
            // still one row segment per workgroup with the outer dims decoded once per
            // workgroup; element-wise (non-vector) accesses with the operand's own stride
            fam = FAM_STREAM;
        }
    } else {
        fam = (c.NK == 0) ? FAM_REDUCE_ALL : FAM_REDUCE_PART;
        // a complete reduction whose dims do not fuse into one run (a sub-box, a permuted sub-box):
        // the ROW form with a single destination element walks it without a per-element index
        // decomposition (measured on a 1000x1000x256 box of a 1024x1024x256 array: 0.59 -> 5 TB/s)
        if (fam == FAM_REDUCE_ALL && c.N > 1 && inputs_run_along(c, 0)) fam = FAM_REDUCE_PART;
        // two inputs that vary along different kept dims (the generic __mul! box): LDS- and register-tiled (option "contract")
        if (fam == FAM_REDUCE_PART && o.force_family == 0 && plan_contract(c, plan.contract)) fam = FAM_CONTRACT;
    }
    if (o.force_family == FAM_GENERIC && c.redop == SMR_RED_NONE) fam = FAM_GENERIC;
    if (o.force_family == FAM_TILED && c.redop == SMR_RED_NONE && fam != FAM_TILED && plan_tiles(c, plan.tile)) fam = FAM_TILED;
    plan.family = fam;
    if (fam == FAM_STREAM) plan_stream(c, plan.stream);
    if (fam == FAM_REDUCE_ALL) plan_reduce_all(c, plan.red);
    if (fam == FAM_REDUCE_PART) plan_reduce_part(c, plan.red);
    describe(plan);
    return SMR_OK;
}

// appends the formatted text to s, whatever its length: formatted once for the length, once into s
static void appendf(std::string& s, const char* fmt, ...) {
    va_list ap, ap2;
    va_start(ap, fmt);
    va_copy(ap2, ap);
    const size_t at = s.size(), n = (size_t)std::max(0, std::vsnprintf(nullptr, 0, fmt, ap));
    s.resize(at + n + 1);
    std::vsnprintf(&s[at], n + 1, fmt, ap2);
    s.resize(at + n);
    va_end(ap);
    va_end(ap2);
}

void describe(Plan& plan) {
    const Canon& c = plan.c;
    static const char* fam[] = {"auto", "generic", "stream", "tiled", "reduce_all", "reduce_part", "orbit", "flat", "contract"};
    static const char* fk[] = {"prog", "ident", "add2", "add3", "add4", "scale", "sym", "axpy", "axpby", "abs2", "mul2", "expr5"};
    static const char* ct[] = {"f32", "f64", "c32", "c64"};
    std::string s;
    appendf(s, "family=%s ct=%s%s f=%s N=%d M=%d dims=", fam[plan.family], c.ct == SMR_I64 ? "i64" : ct[c.ct & 3],
            c.bitcopy ? "(bitcopy)" : (c.mixed ? "(mixed)" : ""), fk[c.fkind], c.N, c.M);
    for (int i = 0; i < c.N; ++i) appendf(s, "%s%lld", i ? "x" : "", (long long)c.dims[i]);
    if (plan.family == FAM_TILED) {
        appendf(s, " tile=");
        for (int j = 0; j < plan.tile.nt; ++j)
            appendf(s, "%sd%d:%d", j ? "," : "", plan.tile.tdim[j], 1 << plan.tile.tlog[j]);
        appendf(s, " staged=%d lds=%zu grid=%lld threads=%d", plan.tile.nstaged, plan.tile.lds_bytes, (long long)plan.tile.grid, plan.tile.threads);
        if (!plan.tile.ord.empty()) appendf(s, " order=orbits:%d", plan.tile.ord_groups);
        if (plan.tile.tilelog == 10 || plan.tile.tilelog == 12) {  // as launched with the bases the plan was made with
            const TiledVariant v = tiled_variant(plan, nullptr, elem_bytes(c), c.mixed && !c.bitcopy);
            appendf(s, " vec=%d%s mode=%d%s%s", v.V, v.ua ? "(element-aligned)" : "", v.mode, v.wide ? " wide" : "",
                    v.pgrid ? " pipe" : "");
        }
    } else if (plan.family == FAM_ORBIT) {
        const OrbitPlan& ob = plan.orbit;
        appendf(s, " tile=");
        bool first = true;
        for (int d = 0; d < c.N; ++d)
            if (ob.lg[d] > 0) {
                appendf(s, "%sd%d:%d", first ? "" : ",", d, 1 << ob.lg[d]);
                first = false;
            }
        appendf(s, " group=%d orbits=%d lds=%zu grid=%zu", ob.ng, ob.norbits, ob.lds_bytes, ob.wmap.size());
        if (ob.pair_ok) appendf(s, " pair_grid=%zu", ob.pmap.size() / 2);
    } else if (plan.family == FAM_FLAT && plan.flatb.on) {
        appendf(s, " batched block=%d(d0..d%d) blocks_per_wg=%d", plan.flatb.P, plan.flatb.g - 1, plan.flatb.K);
    } else if (plan.family == FAM_FLAT && plan.flat2.on) {
        const Flat2Plan& f2 = plan.flat2;
        appendf(s, " two-sided dest_run=%dx%d(d%d) input_run=%dx%d(d%d)%s", f2.R[0], f2.TP[0], f2.p[0], f2.R[1], f2.TP[1], f2.p[1],
                f2.shared ? " shared-dim" : "");
    } else if (plan.family == FAM_FLAT) {
        const FlatPlan& fp = plan.flat;
        appendf(s, " flat_side=%s run=%dx%d(d%d)%s line=d%d:%d", fp.dir == 0 ? "dest" : "input", fp.R, 1 << fp.tplog, fp.p,
                fp.fuse ? "+line" : (fp.lshare ? " shared-lead" : ""), fp.q, 1 << fp.tqlog);
    } else if (plan.family == FAM_STREAM) {
        appendf(s, " vec=%d%s", plan.stream.vec, plan.stream.vec_ua ? "(element-aligned+tail)" : "");
    } else if (plan.family == FAM_REDUCE_ALL) {
        appendf(s, " blocks=%d", plan.red.nparts);
    } else if (plan.family == FAM_REDUCE_PART) {
        static const char* kinds[] = {"general", "row", "col"};
        appendf(s, " nout=%lld form=%s lanes_per_out=%d split=%d", (long long)c.nout, kinds[plan.red.kind], plan.red.tr, plan.red.nparts);
        if (plan.red.kind == 2 && plan.red.col_tx) appendf(s, " lanes=%dx%d", plan.red.col_tx, 256 / plan.red.col_tx);
    }
    if (plan.family == FAM_CONTRACT) {  // vec: as launched with the bases the plan was made with
        const ContractPlan& cp = plan.contract;
        appendf(s, " tile=d%d:%dxd%d:%d k=%d grid=%lld lds=%zu vec=%d", cp.di, cp.ti, cp.dj, cp.tj, cp.tk, (long long)cp.grid, cp.lds_bytes, contract_vec(plan, nullptr));
        // the split form ("split=" is REDUCE_PART's token: tests tell the families apart by it)
        if (cp.kparts > 1) appendf(s, " kparts=%d cps=%lld fold=second-launch scratch=%zu", cp.kparts, (long long)cp.cps, cp.scratch_bytes);
    }
    if (plan.family == FAM_REDUCE_ALL || plan.family == FAM_REDUCE_PART) {
        // as launched with the bases the plan was made with (the partials buffer is allocated on the first execution)
        static const char* folds[] = {"epilogue", "in-launch", "second-launch"};
        const RedLaunch r = reduce_launch(plan, nullptr, true);
        appendf(s, " vec=%d fold=%s", r.vec, folds[r.fold]);
        // ROW / COL: how a split reduction is cut (xsplit along the inner reduced dim x qsplit along the outer reduced index; the tokens must not
        // contain "split=", which tests match); COL: lanes along kept dim 0 as launched
        if (plan.family == FAM_REDUCE_PART && plan.red.kind != 0) {
            appendf(s, " xcut=%d qcut=%d", r.nparts > 1 ? plan.red.xsplit : 1, r.nparts > 1 ? plan.red.qsplit : 1);
            // (narrowed): the launched lanes along kept dim 0 are the segment plan_part_col narrowed -- not said when an exact lane map replaces it
            if (plan.red.kind == 2) appendf(s, " tx=%d%s", r.ctx, (plan.red.narrowed && r.ctx == (1 << plan.red.txlog)) ? "(narrowed)" : "");
        }
    }
    if (c.int_wraps) appendf(s, " int_wraps=%d", c.int_wraps);
    appendf(s, " algbytes=%lld", (long long)c.algbytes);
    plan.desc = std::move(s);
}

}  // namespace smr
