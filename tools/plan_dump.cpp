// plan_dump.cpp -- prints, for a fixed generated corpus of problems, the plan the host-side planner makes: one line per problem and
// option set with the problem's id, describe()'s string and a 64-bit FNV-1a digest over every field and work list the chosen family's
// planner produced.  Needs no GPU and not the library: it is compiled with the planner itself.  Two trees plan alike exactly when
// their outputs are equal, so a planner edit is A/B-ed by building this file against both and running `diff`:
//   cd strided.jl_amd/csrc && hipcc -O2 -std=c++17 --offload-arch=gfx950 -x hip ../../tools/plan_dump.cpp smr_plan*.cpp smr_canon.cpp -o /tmp/plan_dump
// The planner's index arithmetic under AddressSanitizer + UBSan (a plain executable, CPU only; no report = clean):
//   cd strided.jl_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip \
//       ../../tools/plan_dump.cpp smr_plan*.cpp smr_canon.cpp -fsanitize=address,undefined -o /tmp/plan_dump_asan
// To count which builder made a TILED work list, every such problem is planned twice more with one planner switch set (list_with).
// It exits with status 1 when too few problems reach one of the work-list builders or input variants (`need`): a comparison of nothing passes.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../strided.jl_amd/csrc/smr_internal.h"

namespace smr {
int set_error(int code, const std::string&) { return code; }
int cu_count() { return 256; }
}  // namespace smr
using namespace smr;

struct Fnv {
    uint64_t h = 14695981039346656037ull;
    void bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    }
    template <class T> void v(T x) { bytes(&x, sizeof x); }
    template <class T> void arr(const T* a, int n) { for (int i = 0; i < n; ++i) v(a[i]); }
    template <class T> void vec(const std::vector<T>& a) { v(a.size()); arr(a.data(), (int)a.size()); }
};

static uint64_t digest(const Plan& plan) {
    const Canon& c = plan.c;
    Fnv f;
    f.v(plan.family);
    if (plan.family == FAM_TILED) {
        const TilePlan& t = plan.tile;
        f.v(t.nt); f.v(t.tilelog); f.v(t.nstaged); f.v(t.threads); f.v(t.grid); f.v(t.lds_bytes); f.v(t.ord_groups);
        f.v((int)t.no_persist); f.v((int)t.origins32);
        f.arr(t.tdim, t.nt); f.arr(t.tlog, t.nt); f.arr(t.staged, c.M); f.arr(t.ntiles, c.N); f.arr(t.gorder, MAXN);
        for (int k = 0; k < c.M; ++k) f.arr(t.order[k], t.nt);
        f.vec(t.ord);
        const TiledVariant tv = tiled_variant(plan, nullptr, c.bitcopy ? c.esize[0] : dtype_size(c.ct), c.mixed && !c.bitcopy);
        f.v(tv.V); f.v((int)tv.ua); f.v(tv.mode); f.v((int)tv.wide); f.v(tv.thrlog); f.v(tv.pgrid);
    } else if (plan.family == FAM_ORBIT) {
        const OrbitPlan& o = plan.orbit;
        f.v(o.ng); f.v(o.k0); f.v(o.tilelog); f.v(o.vec); f.v(o.ntiles_total); f.v(o.norbits); f.v(o.nslots); f.v((int)o.pair_ok); f.v(o.lds_bytes);
        for (int a = 0; a < o.ng; ++a) { f.arr(o.gdim[a], MAXN); f.arr(o.slot[a], c.M); }
        for (int k = 1; k < c.M; ++k) f.arr(o.pdim[k], c.N);
        f.arr(o.lg, MAXN); f.arr(o.ntiles, MAXN);
        f.vec(o.list); f.vec(o.wtile); f.vec(o.wmap); f.vec(o.ptile); f.vec(o.pmap);
    } else if (plan.family == FAM_FLAT && plan.flatb.on) {
        f.v(plan.flatb.g); f.v(plan.flatb.P); f.v(plan.flatb.K); f.arr(plan.flatb.srcoff, plan.flatb.P);
    } else if (plan.family == FAM_FLAT && plan.flat2.on) {
        const Flat2Plan& p = plan.flat2;
        f.v(p.kt); f.v((int)p.shared); f.arr(p.R, 2); f.arr(p.TP, 2); f.arr(p.p, 2);
        for (int s = 0; s < 2; ++s) { f.arr(p.ingroup[s], MAXN); f.arr(p.roff[s], p.R[s]); }
    } else if (plan.family == FAM_FLAT) {
        const FlatPlan& p = plan.flat;
        f.v(p.dir); f.v(p.R); f.v(p.tplog); f.v(p.tqlog); f.v(p.p); f.v(p.q); f.v(p.kt); f.v((int)p.lshare); f.v((int)p.fuse);
        f.arr(p.ingroup, MAXN); f.arr(p.roff, p.R);
    } else if (plan.family == FAM_STREAM) {
        f.v(plan.stream.vec); f.v((int)plan.stream.vec_ua);
    } else if (plan.family == FAM_REDUCE_ALL || plan.family == FAM_REDUCE_PART) {
        const ReducePlan& r = plan.red;
        f.v(r.nparts); f.v(r.scratch_bytes); f.v(r.tr); f.v(r.kind); f.v(r.g0log); f.v(r.g1log); f.v(r.txlog); f.v(r.col_tx); f.v(r.col_v);
        f.v(r.col_y0); f.v(r.col_y1); f.v(r.xsplit); f.v(r.qsplit); f.v(r.narrowed);
        const RedLaunch l = reduce_launch(plan, nullptr, true);
        f.v(l.vec); f.v(l.fold); f.v(l.nparts); f.v(l.groups); f.v(l.ctx); f.v(l.cty); f.v(l.cy0); f.v(l.cy1);
    } else if (plan.family == FAM_CONTRACT) {
        const ContractPlan& k = plan.contract;
        f.v(k.di); f.v(k.dj); f.v(k.rb); f.v(k.ti); f.v(k.tj); f.v(k.tk); f.v(k.nti); f.v(k.ntj); f.v(k.nrest); f.v(k.grid); f.v(k.lds_bytes);
        f.v(contract_vec(plan, nullptr));
    }
    return f.h;
}

// ---- the corpus ------------------------------------------------------------------------------------------------------------------
typedef std::vector<int> Perm;                        // input dim d is the parent's dim perm[d]
enum Var { ONE, DISTINCT, OFF1, PADDED, REVERSED, STEPPED };  // ONE, OFF1, PADDED: every input views one buffer; the last two change the last input
static const char* var_name[] = {"one", "distinct", "off1", "padded", "reversed", "stepped"};
static const char* dt_name[] = {"f32", "f64", "c32", "c64"};
static char* const DEST = (char*)0x7e0000000000ull;
static char* const SRC = (char*)0x7f0000000000ull;

static void add_input(smr_problem& p, int k, const Perm& perm, Var var, int dtype, bool last) {
    i64 pd[MAXN], ps[MAXN], acc = (var == STEPPED && last) ? 2 : 1;
    for (int d = 0; d < p.N; ++d) pd[perm[d]] = p.dims[d];
    for (int e = 0; e < p.N; ++e) {
        ps[e] = acc;
        acc *= pd[e] + (var == PADDED ? 1 : 0);
    }
    smr_operand& o = p.ops[k];
    o.base = (var == ONE || var == OFF1 || var == PADDED) ? SRC : SRC + ((i64)k << 36);
    o.offset = var == OFF1 ? 1 : 0;
    o.dtype = dtype;
    o.conj = 0;
    for (int d = 0; d < p.N; ++d) o.strides[d] = ps[perm[d]];
    if (var == REVERSED && last) {
        o.offset = (p.dims[0] - 1) * o.strides[0];
        o.strides[0] = -o.strides[0];
    }
}

// destination contiguous over the dims that `keep` marks (stride 0 elsewhere: a sum over those), inputs = `views` of the given variant
static smr_problem problem(const std::vector<i64>& dims, int dtype, const std::vector<Perm>& views, Var var, unsigned keep, bool sum) {
    static const uint8_t add[] = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_ADD, 0, SMR_OP_ARG, 3, SMR_OP_ADD, 0, SMR_OP_ARG, 4, SMR_OP_ADD, 0};
    smr_problem p;
    std::memset(&p, 0, sizeof p);
    p.N = (int)dims.size();
    p.M = 1 + (int)views.size();
    i64 acc = 1;
    for (int d = 0; d < p.N; ++d) {
        p.dims[d] = dims[d];
        p.ops[0].strides[d] = (keep >> d & 1) ? acc : 0;
        if (keep >> d & 1) acc *= dims[d];
    }
    p.ops[0].base = DEST;
    p.ops[0].dtype = dtype;
    for (size_t k = 0; k < views.size(); ++k) add_input(p, 1 + (int)k, views[k], var, dtype, k + 1 == views.size());
    if (views.size() > 1) {
        p.fprog = add;
        p.fprog_len = 2 * (int)views.size() - 1;
    }
    p.redop = sum ? SMR_RED_ADD : SMR_RED_NONE;
    return p;
}

static Perm rotation(int N, int j) {
    Perm p(N);
    for (int d = 0; d < N; ++d) p[d] = (d + j) % N;
    return p;
}
static std::vector<Perm> rotations_and_transpositions(int N) {
    std::vector<Perm> pl;
    for (int j = 1; j < N; ++j) pl.push_back(rotation(N, j));
    for (int a = 0; a < N && N > 2; ++a)  // (N = 2: the transposition is the rotation)
        for (int b = a + 1; b < N; ++b) {
            pl.push_back(rotation(N, 0));
            std::swap(pl.back()[a], pl.back()[b]);
        }
    return pl;
}

// the option sets every problem is planned with; each is restored to the default before the next
struct OptSet { const char* name; i64 Options::*field; i64 value; };
static const OptSet optsets[] = {{"default", nullptr, 0},           {"orbit=0", &Options::orbit, 0},           {"orbit_pack=0", &Options::orbit_pack, 0},
                                 {"orbit_pair=0", &Options::orbit_pair, 0}, {"tile_order=0", &Options::tile_order, 0}, {"tile_block=-2", &Options::tile_block, -2}};
// how many (problem, option set) lines reached each work-list builder and each input variant, and the least the corpus must give each
enum { C_PAIR, C_PACKED, C_TILED_ORBIT, C_BLOCK_XCD, C_BLOCK_RR, C_COUNT };
static const char* cname[] = {"orbit_pair", "orbit_packed", "tiled_orbit_order", "tiled_block_per_xcd", "tiled_block_round_robin"};
static long counts[C_COUNT], var_lines[6], fam_lines[9], lines;
constexpr long need = 40;

// the TILED work list of the problem when one more option is set (empty: no list, or another family)
static std::vector<uint32_t> list_with(const smr_problem& p, i64 Options::*field, i64 value) {
    const Options saved = options();
    options().*field = value;
    Plan plan;
    const bool tiled = make_plan(&p, plan) == 0 && plan.family == FAM_TILED;
    options() = saved;
    return tiled ? plan.tile.ord : std::vector<uint32_t>();
}

static void plan_all(const std::string& id, const smr_problem& p, int var = ONE) {
    for (const OptSet& os : optsets) {
        const Options saved = options();
        if (os.field) options().*os.field = os.value;
        Plan plan;
        const int rc = make_plan(&p, plan);
        if (rc) std::printf("%s opt=%s rc=%d\n", id.c_str(), os.name, rc);
        else std::printf("%s opt=%s | %s | %016llx\n", id.c_str(), os.name, plan.desc.c_str(), (unsigned long long)digest(plan));
        ++lines;
        ++var_lines[var];
        const OrbitPlan& o = plan.orbit;
        const TilePlan& t = plan.tile;
        if (!rc) ++fam_lines[plan.family];
        if (!rc && plan.family == FAM_ORBIT) {
            size_t busy = 0;
            for (size_t w = 0; w < o.wmap.size(); ++w) busy += o.wtile[w * o.nslots] != 0xffffffffu;
            counts[C_PAIR] += o.pair_ok;
            counts[C_PACKED] += busy < (size_t)o.norbits;  // orbits that share a workgroup
        } else if (!rc && plan.family == FAM_TILED && !t.ord.empty()) {
            // which builder made the list is read off the planner's own switches: a list that "tile_order" = 0 changes is the orbit order;
            // a block-ordered list equals the one forced into a run per XCD, or it is the round-robin one
            if (t.ord != list_with(p, &Options::tile_order, 0)) ++counts[C_TILED_ORBIT];
            else ++counts[t.ord == list_with(p, &Options::tile_block_xcd, 1) ? C_BLOCK_XCD : C_BLOCK_RR];
        }
        options() = saved;
    }
}

static std::string ident(const std::vector<i64>& dims, int dtype, const std::vector<Perm>& views, const char* what) {
    std::string s = dt_name[dtype];
    for (size_t d = 0; d < dims.size(); ++d) s += (d ? "x" : " ") + std::to_string(dims[d]);
    s += " in=";
    for (size_t k = 0; k < views.size(); ++k) {
        if (k) s += ",";
        for (int e : views[k]) s += (char)('0' + e);
    }
    return s + " " + what;
}

int main() {
    const int dtypes[] = {SMR_F32, SMR_F64, SMR_C64};
    const i64 ext[] = {3, 7, 8, 24, 32, 40, 48, 64, 100};
    // mixed shapes: equal extents in the places the rotations and transpositions exchange, and extents that differ
    const std::vector<std::vector<i64>> mixed = {{100, 7}, {3, 64}, {48, 40}, {24, 100}, {8, 32, 8}, {64, 7, 64}, {40, 40, 3}, {24, 48, 24},
                                                 {32, 32, 8, 8}, {8, 32, 8, 32}, {24, 24, 7, 7}, {3, 40, 40, 3}, {48, 8, 48, 8}};
    for (int N = 2; N <= 4; ++N) {
        std::vector<std::vector<i64>> shapes;
        for (i64 e : ext)
            if (N < 4 || e <= 64) shapes.push_back(std::vector<i64>((size_t)N, e));  // (total <= 2^24)
        for (const auto& m : mixed)
            if ((int)m.size() == N) shapes.push_back(m);
        const std::vector<Perm> pl = rotations_and_transpositions(N);
        const Perm id = rotation(N, 0);
        const size_t n = pl.size();
        std::vector<std::vector<Perm>> sets;  // 1-4 inputs; with and without the identity view
        for (const Perm& p : pl) sets.push_back({p});
        for (const Perm& p : pl) sets.push_back({id, p});
        for (size_t i = 0; i < n && n > 1; ++i) sets.push_back({pl[i], pl[(i + 1) % n]});
        for (size_t i = 0; i < n && n > 1; ++i) sets.push_back({id, pl[i], pl[(i + 1) % n]});
        for (size_t i = 0; i + 2 < n; i += 3) sets.push_back({id, pl[i], pl[i + 1], pl[i + 2]});
        for (const auto& dims : shapes)
            for (int dt : dtypes) {
                for (size_t si = 0; si < sets.size(); ++si)
                    for (int var = ONE; var <= STEPPED; ++var) {
                        if (sets[si].size() == 1 && var == DISTINCT) continue;  // (the same problem as ONE)
                        if (var >= OFF1 && (si + var) % 4) continue;            // one of the four windowed variants per set, in turn
                        plan_all(ident(dims, dt, sets[si], var_name[var]), problem(dims, dt, sets[si], (Var)var, ~0u, false), var);
                    }
                // sums over the leading dim, the trailing dim and all dims, of the array and of a rotated view
                for (unsigned keep : {~1u, ~(1u << (N - 1)), 0u})
                    for (const Perm& v : {id, pl[0]})
                        plan_all(ident(dims, dt, {v}, keep == 0 ? "sum all" : (keep == ~1u ? "sum leading" : "sum trailing")), problem(dims, dt, {v}, ONE, keep, true));
            }
    }
    // the 4-way sum with its four rotations in every input order (whichever input is the identity view; the slot maps differ): ORBIT on
    // 4^4 cubes at 24^4 and 32^4 (the PAIR form for 8-byte elements), on 8^4 cubes at 40^4
    for (i64 e : {24, 32, 40})
        for (int dt : dtypes) {
            int ix[4] = {0, 1, 2, 3};
            do {
                const std::vector<Perm> views = {rotation(4, ix[0]), rotation(4, ix[1]), rotation(4, ix[2]), rotation(4, ix[3])};
                plan_all(ident({e, e, e, e}, dt, views, "one"), problem({e, e, e, e}, dt, views, ONE, ~0u, false));
            } while (std::next_permutation(ix, ix + 4));
        }
    // unary transposes with short leading dims that are no powers of two, batched small blocks, two short sides: the FLAT forms
    const std::vector<std::vector<i64>> flats = {{3, 256, 200}, {5, 300, 300, 7}, {6, 64, 64, 5}, {7, 100, 90}, {9, 11, 300, 30}, {17, 33, 65, 31},
                                                 {257, 129, 65}, {3, 1000, 700}, {100, 90, 80}, {6, 64, 64, 64}};
    for (const auto& dims : flats)
        for (int dt : dtypes) {
            const int N = (int)dims.size();
            std::vector<Perm> pl = rotations_and_transpositions(N);
            Perm rev(N);
            for (int d = 0; d < N; ++d) rev[d] = N - 1 - d;
            pl.push_back(rev);
            for (const Perm& p : pl) plan_all(ident(dims, dt, {p}, "one"), problem(dims, dt, {p}, ONE, ~0u, false));
        }
    // large boxes that cross the size rules of plan_tiles (and, four distinct arrays, the Infinity-Cache rule of the block order)
    const std::vector<std::vector<i64>> large = {{96, 96, 96, 96}, {128, 128, 128, 128}, {4000, 4000}, {8192, 8192}};
    for (const auto& dims : large)
        for (int dt : dtypes) {
            const int N = (int)dims.size();
            std::vector<Perm> all{rotation(N, 0)};
            for (int j = 1; j < N; ++j) all.push_back(rotation(N, j));
            for (size_t m = 2; m <= all.size(); ++m)
                for (int var : {ONE, DISTINCT}) {
                    const std::vector<Perm> views(all.begin(), all.begin() + m);
                    plan_all(ident(dims, dt, views, var_name[var]), problem(dims, dt, views, (Var)var, ~0u, false), var);
                }
            plan_all(ident(dims, dt, {all[1]}, "one"), problem(dims, dt, {all[1]}, ONE, ~0u, false));
        }
    // reductions of the contraction shape (the generic __mul! box: C (m, n), A (m, k), B (k, n), column-major): the only lines the
    // CONTRACT family may move
    for (const auto& mnk : std::vector<std::vector<i64>>{{256, 256, 256}, {512, 512, 512}, {1024, 1024, 1024}, {4096, 64, 64}, {64, 64, 4096}, {100, 90, 80},
                                                           {1000, 1000, 16}, {2048, 32, 256}, {2048, 2048, 64}, {33, 34, 9}, {1000, 1000, 8}, {512, 512, 15}})
        for (int dt : dtypes) {
            smr_problem p = problem(mnk, dt, {rotation(3, 0), rotation(3, 0)}, DISTINCT, 3u, true);
            const i64 m = mnk[0], n = mnk[1], k = mnk[2];
            const i64 sa[3] = {1, 0, m}, sb[3] = {0, k, 1};
            for (int d = 0; d < 3; ++d) {
                p.ops[1].strides[d] = sa[d];
                p.ops[2].strides[d] = sb[d];
            }
            static const uint8_t mul[] = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_MUL, 0};
            p.fprog = mul;
            p.fprog_len = 3;
            (void)n;
            plan_all(ident(mnk, dt, {}, "contraction"), p, DISTINCT);
        }
    static const char* fam[] = {"auto", "generic", "stream", "tiled", "reduce_all", "reduce_part", "orbit", "flat", "contract"};
    std::fprintf(stderr, "%ld lines:", lines);
    for (int f = 1; f < 9; ++f) std::fprintf(stderr, " %s=%ld", fam[f], fam_lines[f]);
    std::fprintf(stderr, "\n");
    int rc = 0;
    auto report = [&](const char* what, long n) {
        std::fprintf(stderr, "  %s: %ld%s\n", what, n, n < need ? "  -- TOO FEW: the corpus no longer covers this" : "");
        if (n < need) rc = 1;
    };
    for (int i = 0; i < C_COUNT; ++i) report(cname[i], counts[i]);
    for (int v = ONE; v <= STEPPED; ++v) report(var_name[v], var_lines[v]);
    return rc;
}
