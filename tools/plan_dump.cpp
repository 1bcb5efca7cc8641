// plan_dump.cpp -- prints, for a fixed generated corpus of problems, the plan the host-side planner makes: one line per problem and
// option set with the problem's id, describe()'s string and a 64-bit FNV-1a digest over every field and work list the chosen family's
// planner produced.  Needs no GPU and not the library: it is compiled with the planner itself.  Two trees plan alike exactly when
// their outputs are equal, so a planner edit is A/B-ed by building this file against both and running `diff`:
//   cd strided.jl_amd/csrc && hipcc -O2 -std=c++17 --offload-arch=gfx950 -x hip ../../tools/plan_dump.cpp smr_plan*.cpp smr_canon.cpp -o /tmp/plan_dump
// The planner's index arithmetic under AddressSanitizer + UBSan (a plain executable, CPU only; no report = clean):
//   cd strided.jl_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip \
//       ../../tools/plan_dump.cpp smr_plan*.cpp smr_canon.cpp -fsanitize=address,undefined -o /tmp/plan_dump_asan
// To count which builder made a TILED work list, every such problem is planned twice more with one planner switch set (list_with).
// The last section plans a fixed corpus of GROUPS through plan_group (smr_plan_group.cpp): one line per group, "group <id>", with
// describe()'s string and a digest over the kind, the raw bytes of the device tables (member descriptors, first_wg, scalar rows),
// W, varc, rb, rank, jit, algbytes and the rd / wr footprint -- or, for a group the planner refuses, its status and message.  The
// corpus restates the recipes and the refusals of tests/group_cases.py, group_scalar_cases.py, group_contract_cases.py and the group
// host tests over fake addresses.  (smr_group_create's own argument checks -- null, count, unknown flag -- are not the planner's.)
// Before the groups, a section "split <id> ..." plans the generic product box with "contract_split" / "contract_tile" set: both outcomes
// of the rule, every tile, forced slices, slices clamped to the chunks, a forced tile refused (`sneed`).  The sections before it plan
// with both options at their defaults.
// Behind the groups, a section "gsplit <id> ..." plans contraction groups under option "group_contract_split": the group rule's outcomes
// (split, a forced tile, a mixed group, groups left alone), forced slices on both tiles, slices clamped to the chunks, and the option at 0.
// Last, a section "gscalars <id> ..." plans contraction groups under SMR_GROUP_CONTRACT_SCALARS (f = x * y * alpha): equal constants (shared),
// a row per member, and a row per member with split members; its digest also covers the table of constants.
// Behind every TILED and ORBIT plan line come the launch arguments the family's pure builder makes for it (smr_plan_tiled_args.cpp,
// smr_plan_orbit_args.cpp): "args <id> opt=<set> | <form> | <digest>" over the builder's status, the argument struct's bytes (pointers
// null) and its tables -- TILED: the variant tiled_variant() names, struct and lane rows; ORBIT: "variant" lines with orbit_variant()'s
// answer for a runtime-compiled functor (native_nin = -1) and for a native one of M - 1 inputs, the one-orbit form's struct and origin
// rows, and the PAIR form's struct and work list where the native functor gets it.  Every form a launcher can reach must be digested
// (`form_need`): TILED narrow with V = 1 (modes 0, 1, 2, 7) and V = VMAX (modes 0, 1, 2, 7, 9) and wide (V = 1; modes 0, 1, 2, 7);
// ORBIT with 2 and 4 slots, with and without the identity view first, the PAIR form, and element-wise accesses (V = 1 where VMAX > 1:
// reached by the "off1" variants, whose views begin one element into the buffer).  The present corpus reaches all of them.
// Two combinations of the list (V in {1, VMAX}) x (narrow, wide) x (modes 0, 1, 2, 7, 9) are absent from `form_need` because no plan
// can have them: tiled_variant() picks V > 1 only when the offsets are narrow (`!v.wide`), so there is no wide V > 1 form, and mode 9 is
// mode 1 plus partial VECTORS, picked only when V > 1, so there is no mode 9 with V = 1 (narrow or wide).
// It exits with status 1 when too few problems reach one of the work-list builders or input variants (`need`), when a group kind, body,
// tile, scalar form or refusal is not reached (`gneed`), when a form of the argument builders is not reached (`form_need`), or when a group is refused or accepted against its recipe: a comparison of
// nothing passes.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../strided.jl_amd/csrc/smr_group.h"
#include "../strided.jl_amd/csrc/smr_orbit_args.h"
#include "../strided.jl_amd/csrc/smr_tiled_args.h"

static std::string last_error;  // what a refused group prints
namespace smr {
int set_error(int code, const std::string& msg) {
    last_error = msg;
    return code;
}
int cu_count() { return 256; }
}  // namespace smr
extern "C" const char* smr_last_error(void) { return last_error.c_str(); }
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
        if (k.kparts > 1) { f.v(k.kparts); f.v(k.cps); f.v(k.scratch_bytes); }  // (an unsplit plan's digest is the one from before the split form)
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

// ---- the launch arguments of TILED and ORBIT (the pure builders) -------------------------------------------------------------------
static std::map<std::string, long> form_counts;
static const char* const form_need[] = {"tiled narrow V=1 mode=0", "tiled narrow V=1 mode=1", "tiled narrow V=1 mode=2", "tiled narrow V=1 mode=7",
                                        "tiled narrow V>1 mode=0", "tiled narrow V>1 mode=1", "tiled narrow V>1 mode=2", "tiled narrow V>1 mode=7",
                                        "tiled narrow V>1 mode=9", "tiled wide V=1 mode=0",   "tiled wide V=1 mode=1",   "tiled wide V=1 mode=2",
                                        "tiled wide V=1 mode=7",   "orbit ng=2",              "orbit ng=4",              "orbit own0=0",
                                        "orbit own0=1",            "orbit pair",              "orbit V=1"};
constexpr long form_min = 8;

template <class A, class R>
static uint64_t digest_args(int rc, const A& a, const std::vector<R>& rows) {
    Fnv f;
    f.v(rc);
    f.bytes(&a, sizeof a);
    f.v(rows.size());
    f.bytes(rows.data(), rows.size() * sizeof(R));
    return f.h;
}
template <bool WIDE>
static void tiled_args_line(const std::string& head, const Plan& plan, int esize, const TiledVariant& tv) {
    TiledBuild<WIDE> b;
    const int rc = build_tiled_args<WIDE>(plan, esize, tv, b);
    const std::string form = std::string("tiled ") + (WIDE ? "wide" : "narrow") + (tv.V > 1 ? " V>1" : " V=1") + " mode=" + std::to_string(tv.mode);
    std::printf("%s | %s V=%d rc=%d | %016llx\n", head.c_str(), form.c_str(), tv.V, rc, (unsigned long long)digest_args(rc, b.a, b.rows));
    if (!rc) ++form_counts[form];
}
static void args_lines(const std::string& head, const Plan& plan) {
    const Canon& c = plan.c;
    if (plan.family == FAM_TILED) {
        const int esize = c.bitcopy ? c.esize[0] : dtype_size(c.ct);
        const TiledVariant tv = tiled_variant(plan, nullptr, esize, c.mixed && !c.bitcopy);
        if (tv.wide) tiled_args_line<true>(head, plan, esize, tv);
        else tiled_args_line<false>(head, plan, esize, tv);
    } else if (plan.family == FAM_ORBIT) {
        const int esize = dtype_size(c.ct);
        for (int nin : {-1, c.M - 1}) {
            OrbitVariant v;
            const int vrc = orbit_variant(plan, nullptr, esize, nin, v);
            if (vrc) {
                std::printf("%s | variant nin=%d rc=%d | %s\n", head.c_str(), nin, vrc, last_error.c_str());
                continue;
            }
            std::printf("%s | variant nin=%d V=%d nrep=%d ng=%d own0=%d pipe=%d pair=%d\n", head.c_str(), nin, v.V, v.nrep, v.ng, (int)v.own0, (int)v.pipe, (int)v.pair);
            if (nin >= 0 && !v.pair) continue;  // the one-orbit form again
            OrbitBuild b;
            const int rc = v.pair ? build_pair_args(plan, esize, b) : build_orbit_args(plan, esize, v, b);
            std::printf("%s | orbit %s rc=%d | %016llx\n", head.c_str(), v.pair ? "pair" : "one", rc, (unsigned long long)digest_args(rc, b.a, b.rows));
            if (rc) continue;
            if (v.pair) {
                ++form_counts["orbit pair"];
            } else {
                ++form_counts[v.ng == 2 ? "orbit ng=2" : "orbit ng=4"];
                ++form_counts[v.own0 ? "orbit own0=1" : "orbit own0=0"];
                if (v.V == 1 && esize < 16) ++form_counts["orbit V=1"];
            }
        }
    }
}

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
        if (!rc) args_lines("args " + id + " opt=" + os.name, plan);
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

// ---- groups (smr_plan_group.cpp: plan_group) -----------------------------------------------------------------------------------------
// The recipes of tests/group_cases.py, tests/group_scalar_cases.py and tests/group_contract_cases.py and the refusals of the group
// host tests, restated over fake addresses: operand k of member `slot` has a 16 MiB region of its own unless a recipe shares one.
static uint64_t digest(const GroupPlan& g) {
    Fnv f;
    f.v((int)g.kind);
    f.v(g.map.members.size()); f.bytes(g.map.members.data(), g.map.members.size() * sizeof(GroupMemberD));
    f.v(g.contract.members.size()); f.bytes(g.contract.members.data(), g.contract.members.size() * sizeof(GroupContractMemberD));
    f.vec(g.first_wg); f.vec(g.map.consts);
    f.v(g.map.W); f.v((int)g.map.varc); f.v(g.contract.rb); f.vec(g.rank); f.v((int)g.jit); f.v(g.algbytes);
    for (const auto* spans : {&g.rd, &g.wr}) {
        f.v(spans->size());
        for (const auto& r : *spans) { f.v(r.first); f.v(r.second); }
    }
    return f.h;
}

enum { G_MAP, G_CONTRACT, G_LINEAR, G_TRANSPOSING, G_TILE16, G_TILE32, G_RULE16, G_RULE32, G_SCALARS_MEMBER, G_SCALARS_SHARED, G_REFUSED, G_COUNT };
static const char* gname[] = {"group_map", "group_contract", "group_body_linear", "group_body_transposing", "group_tile_16", "group_tile_32",
                              "group_rule_picks_16", "group_rule_picks_32", "group_scalars_member", "group_scalars_shared", "group_refusals"};
static const long gneed[G_COUNT] = {20, 10, 20, 8, 4, 4, 2, 2, 5, 3, 34};  // (refusals: every one the corpus lists)
static long gcounts[G_COUNT], glines, gwrong;

static char* gaddr(int slot, int k) { return (char*)0x7c0000000000ull + ((i64)slot << 28) + ((i64)k << 24); }
static const double* consts_of(std::initializer_list<double> re_im) {
    static std::vector<std::vector<double>> pool;  // (kept for the run: problems point into it)
    pool.emplace_back(re_im);
    return pool.back().data();
}
typedef std::vector<uint8_t> Prog;
static const Prog P_IDENT = {}, P_ADD2 = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_ADD, 0}, P_SCALE = {SMR_OP_ARG, 1, SMR_OP_CONST, 0, SMR_OP_MUL, 0},
                  P_PLUSC = {SMR_OP_ARG, 1, SMR_OP_CONST, 0, SMR_OP_ADD, 0}, P_MUL = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_MUL, 0},
                  P_AXPBY = {SMR_OP_CONST, 0, SMR_OP_ARG, 1, SMR_OP_MUL, 0, SMR_OP_CONST, 1, SMR_OP_ARG, 2, SMR_OP_MUL, 0, SMR_OP_ADD, 0},
                  P_AXPBY_MERGED = {SMR_OP_CONST, 0, SMR_OP_ARG, 1, SMR_OP_MUL, 0, SMR_OP_CONST, 0, SMR_OP_ARG, 2, SMR_OP_MUL, 0, SMR_OP_ADD, 0},
                  P_AXPY = {SMR_OP_CONST, 0, SMR_OP_ARG, 1, SMR_OP_MUL, 0, SMR_OP_ARG, 2, SMR_OP_ADD, 0},
                  P_PROG = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_MUL, 0, SMR_OP_ARG, 1, SMR_OP_CONST, 0, SMR_OP_DIV, 0, SMR_OP_SUB, 0},
                  P_MATH = {SMR_OP_ARG, 1, SMR_OP_TAN, 0, SMR_OP_ARG, 2, SMR_OP_ADD, 0}, P_MULC = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_MUL, 0, SMR_OP_CONST, 0, SMR_OP_MUL, 0},
                  P_DIST = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_SUB, 0, SMR_OP_ABS, 0};
static void set_f(smr_problem& p, const Prog& prog, std::initializer_list<double> re_im = {}) {
    p.fprog = prog.empty() ? nullptr : prog.data();
    p.fprog_len = (int)prog.size() / 2;
    p.nconsts = (int)re_im.size() / 2;
    p.fconsts = re_im.size() ? consts_of(re_im) : nullptr;
}
// a map member: column-major destination of `dims`, input k the view `views[k]` of a column-major parent (add_input)
static smr_problem gmap(int slot, const std::vector<i64>& dims, const std::vector<Perm>& views, const Prog& prog = P_IDENT,
                        std::initializer_list<double> re_im = {}, int dtype = SMR_F64, int in_dtype = -1) {
    smr_problem p = problem(dims, dtype, views, DISTINCT, ~0u, false);
    p.ops[0].base = gaddr(slot, 0);
    for (int k = 1; k < p.M; ++k) {
        p.ops[k].base = gaddr(slot, k);
        if (in_dtype >= 0) p.ops[k].dtype = in_dtype;
    }
    set_f(p, prog, re_im);
    return p;
}
static smr_problem gcopy(int slot, const std::vector<i64>& dims, int dtype = SMR_F64) { return gmap(slot, dims, {rotation((int)dims.size(), 0)}, P_IDENT, {}, dtype); }
static smr_problem gtrans(int slot, i64 m, i64 n, const Prog& prog = P_IDENT, std::initializer_list<double> re_im = {}) { return gmap(slot, {m, n}, {{1, 0}}, prog, re_im); }
// a contraction member over box (m, n, [batch], k, [k2]): the destination varies along m, n and batch, input 1 along all but n, input 2
// along all but m; `kfirst` bit k: that input's parent is laid out reduced dims first; `pad` extends every parent dim by that much
static smr_problem gmul(int slot, const std::vector<i64>& dims, int nkept, int dtype = SMR_F64, unsigned kfirst = 0, int pad = 0, int initop = SMR_INIT_ZERO, double beta = 0) {
    smr_problem p;
    std::memset(&p, 0, sizeof p);
    p.N = (int)dims.size();
    p.M = 3;
    for (int d = 0; d < p.N; ++d) p.dims[d] = dims[d];
    for (int o = 0; o < 3; ++o) {
        i64 acc = 1;
        for (int pass = 0; pass < 2; ++pass)
            for (int d = 0; d < p.N; ++d) {
                const bool varies = o == 0 ? d < nkept : (o == 1 ? d != 1 : d != 0);
                const bool first = (o > 0 && (kfirst >> o & 1)) ? d >= nkept : d < nkept;
                if (varies && first == (pass == 0)) {
                    p.ops[o].strides[d] = acc;
                    acc *= dims[d] + pad;
                }
            }
        p.ops[o].base = gaddr(slot, o);
        p.ops[o].dtype = dtype;
    }
    set_f(p, P_MUL);
    p.redop = SMR_RED_ADD;
    p.initop = initop;
    p.initarg[0] = beta;
    return p;
}
static smr_problem gmm(int slot, i64 m, i64 n, i64 k, int dtype = SMR_F64, unsigned kfirst = 0, int pad = 0, int initop = SMR_INIT_ZERO, double beta = 0) {
    return gmul(slot, {m, n, k}, 2, dtype, kfirst, pad, initop, beta);
}

// plans one group and prints its line; `refused`: the recipe is one the library refuses (the line then holds status and message)
static void plan_one_group(const std::string& id, const std::vector<smr_problem>& ms, uint32_t flags = 0, bool refused = false, i64 tile = 0) {
    const i64 saved = group_contract_tile();
    group_contract_tile() = tile;
    GroupPlan g;
    const int rc = plan_group(ms.data(), (int)ms.size(), flags, g);
    group_contract_tile() = saved;
    ++glines;
    if ((rc != 0) != refused) ++gwrong;
    if (rc) {
        std::printf("group %s | rc=%d | %s\n", id.c_str(), rc, last_error.c_str());
        ++gcounts[G_REFUSED];
        return;
    }
    std::printf("group %s | %s | %016llx\n", id.c_str(), g.desc.c_str(), (unsigned long long)digest(g));
    if (g.kind == GROUP_CONTRACT) {
        ++gcounts[G_CONTRACT];
        ++gcounts[g.contract.rb == 2 ? G_TILE32 : G_TILE16];
        if (!tile) ++gcounts[g.contract.rb == 2 ? G_RULE32 : G_RULE16];
    } else {
        ++gcounts[G_MAP];
        gcounts[G_LINEAR] += g.map.nlinear > 0;
        gcounts[G_TRANSPOSING] += g.map.ntrans > 0;
        if (flags & SMR_GROUP_MEMBER_SCALARS) ++gcounts[g.map.varc ? G_SCALARS_MEMBER : G_SCALARS_SHARED];
    }
}

// Split contraction groups (option "group_contract_split"): "gsplit <id> | describe() | digest", the digest also over the tables of the
// split form (per member S, cps, tiles and the partials' offset; the fold launch's prefix sums) and the scratch size.  Rows of their
// own behind the group corpus: with the option at 0 every line above is the one of a tree without the option.
static void plan_split_group(const std::string& id, const std::vector<smr_problem>& ms, i64 split, i64 tile = 0) {
    const i64 saved_tile = group_contract_tile(), saved_split = group_contract_split();
    group_contract_tile() = tile;
    group_contract_split() = split;
    GroupPlan g;
    const int rc = plan_group(ms.data(), (int)ms.size(), 0, g);
    group_contract_tile() = saved_tile;
    group_contract_split() = saved_split;
    if (rc) {
        std::printf("gsplit %s | rc=%d | %s\n", id.c_str(), rc, last_error.c_str());
        return;
    }
    Fnv f;
    f.v(digest(g));
    f.v(g.contract.split.size()); f.bytes(g.contract.split.data(), g.contract.split.size() * sizeof(GroupSplitD));
    f.vec(g.contract.fold_first); f.v(g.contract.nsplit); f.v(g.contract.max_s); f.v(g.contract.scratch_bytes);
    std::printf("gsplit %s | %s | %016llx\n", id.c_str(), g.desc.c_str(), (unsigned long long)f.h);
}

static void split_group_corpus() {
    typedef std::vector<smr_problem> Ms;
    Ms longs, mixed, small, full;
    for (int i = 0; i < 16; ++i) longs.push_back(gmm(i, 32, 32, 4096));
    for (int i = 0; i < 10; ++i) mixed.push_back(gmm(i, 32, 32, 32));
    for (int i = 10; i < 12; ++i) mixed.push_back(gmm(i, 32, 32, 16384));
    mixed.push_back(gmul(12, {33, 31, 3, 65, 3}, 3));   // ragged tiles, a batch dim, two reduced dims
    for (int i = 0; i < 300; ++i) small.push_back(gmm(i, 32, 32, 32));
    for (int i = 0; i < 64; ++i) full.push_back(gmm(i, 64, 64, 4096, SMR_F32));
    plan_split_group("rule/16x(32,32,4096)", longs, 1);                 // the rule splits: 32 x 32 tiles, 32 slices each
    plan_split_group("rule/16x(32,32,4096)/t16", longs, 1, 16);        // ... a forced tile stays
    plan_split_group("rule/mixed", mixed, 1);                           // only the long members are split
    plan_split_group("rule/300x(32,32,32)", small, 1);                  // left alone: 256 workgroups and more
    plan_split_group("rule/64x(64,64,4096)f32", full, 1);               // left alone: 256 workgroups and more
    plan_split_group("forced3/mixed/t16", mixed, 3, 16);
    plan_split_group("forced64/mixed/t32", mixed, 64, 32);
    plan_split_group("forced1000/16x(32,32,4096)", longs, 1000);        // clamped to the chunks
    plan_split_group("off/mixed", mixed, 0);                            // the unsplit plan
}

// Contraction groups with per-member constants of f (SMR_GROUP_CONTRACT_SCALARS): "gscalars <id> | describe() | digest", the digest also
// over the table of constants (W, varc, whether the mul! form runs natively, every row) and, for a split group, the split form's tables.
// Rows of their own behind the other corpora: every line above is the one of a tree without the flag.
static void plan_scalars_group(const std::string& id, const std::vector<smr_problem>& ms, i64 split = 0, i64 tile = 0) {
    const i64 saved_tile = group_contract_tile(), saved_split = group_contract_split();
    group_contract_tile() = tile;
    group_contract_split() = split;
    GroupPlan g;
    const int rc = plan_group(ms.data(), (int)ms.size(), SMR_GROUP_CONTRACT_SCALARS, g);
    group_contract_tile() = saved_tile;
    group_contract_split() = saved_split;
    if (rc) {
        std::printf("gscalars %s | rc=%d | %s\n", id.c_str(), rc, last_error.c_str());
        return;
    }
    Fnv f;
    f.v(digest(g));
    f.v(g.contract.W); f.v((int)g.contract.varc); f.v((int)g.contract.mul2scale); f.vec(g.contract.consts);
    f.v(g.contract.split.size()); f.bytes(g.contract.split.data(), g.contract.split.size() * sizeof(GroupSplitD));
    f.vec(g.contract.fold_first); f.v(g.contract.nsplit); f.v(g.contract.max_s); f.v(g.contract.scratch_bytes);
    std::printf("gscalars %s | %s | %016llx\n", id.c_str(), g.desc.c_str(), (unsigned long long)f.h);
}

static void scalars_group_corpus() {
    typedef std::vector<smr_problem> Ms;
    auto alpha = [](smr_problem p, double re) {
        set_f(p, P_MULC, {re, 0});
        return p;
    };
    Ms shared, member, split;
    for (int i = 0; i < 12; ++i) shared.push_back(alpha(gmm(i, 20 + i, 24, 9), 2.0));
    for (int i = 0; i < 12; ++i) member.push_back(alpha(gmm(i, 20 + i, 24, 9), 0.5 * (i + 2)));
    for (int i = 0; i < 10; ++i) split.push_back(alpha(gmm(i, 32, 32, 32), 3.0 - i));
    for (int i = 10; i < 12; ++i) split.push_back(alpha(gmm(i, 32, 32, 16384), -0.25 * i));
    plan_scalars_group("shared", shared);               // equal constants: the unflagged plan, scalars=shared
    plan_scalars_group("member", member);               // a row per member, f=mul2scale
    plan_scalars_group("member+split", split, 3, 16);   // ... and the long members cut into slices
}

static void group_corpus() {
    const uint32_t IND = SMR_GROUP_INDEPENDENT, OWN = SMR_GROUP_MEMBER_SCALARS;
    typedef std::vector<smr_problem> Ms;
    // the layout test's shapes: both bodies in one group, 1024 / 1025 elements on either side of a chunk, rank 8
    const std::vector<std::vector<i64>> shapes = {{1}, {5, 7}, {31, 33}, {33, 31}, {64, 1, 3}, {4, 4, 4, 4, 4, 4, 4, 4}, {1024}, {1025}, {40, 40, 3}};
    auto layout_members = [&](const Prog& prog, bool own) {
        Ms ms;
        for (size_t i = 0; i < shapes.size(); ++i) {
            const int N = (int)shapes[i].size();
            Perm v(N);
            std::vector<i64> dims(N);
            for (int d = 0; d < N; ++d) v[d] = i % 2 ? N - 1 - d : d;
            for (int d = 0; d < N; ++d) dims[d] = shapes[i][v[d]];
            ms.push_back(prog.empty() ? gmap((int)i, dims, {v}) : gmap((int)i, dims, {v}, prog, {own ? 1 + (double)i / 8 : 2.5, 0}));
        }
        return ms;
    };
    for (uint32_t flags : {0u, IND}) plan_one_group("layout ident flags=" + std::to_string(flags), layout_members(P_IDENT, false), flags);
    plan_one_group("layout scale", layout_members(P_SCALE, false));
    plan_one_group("layout scale own=shared", layout_members(P_SCALE, false), OWN);
    plan_one_group("layout scale own=member", layout_members(P_SCALE, true), OWN);
    // GROUP_TMIN: 15 and 16 along dim 0 and along the staged input's unit-stride dim q, each alone and all in one group
    Ms tmin;
    for (i64 e : {15, 16})
        for (int side = 0; side < 2; ++side) {
            tmin.push_back(side ? gtrans((int)tmin.size(), 40, e) : gtrans((int)tmin.size(), e, 40));
            plan_one_group("tmin " + std::to_string(e) + (side ? " along q" : " along dim 0"), {tmin.back()});
        }
    plan_one_group("tmin all", tmin);
    for (int dt : {SMR_F32, SMR_F64, SMR_C32, SMR_C64}) {  // per type: one member per body, two and three inputs, outer dims around the plane
        const std::string t = dt_name[dt];
        plan_one_group("bodies " + t, {gmap(0, {33, 31}, {{0, 1}}, P_IDENT, {}, dt), gmap(1, {31, 33}, {{1, 0}}, P_IDENT, {}, dt), gmap(2, {20, 24, 28}, {{1, 2, 0}}, P_IDENT, {}, dt),
                                      gmap(3, {17, 3, 40}, {{2, 1, 0}}, P_IDENT, {}, dt), gmap(4, {1, 1}, {{0, 1}}, P_IDENT, {}, dt)});
        plan_one_group("add2 " + t, {gmap(0, {40, 33}, {{0, 1}, {1, 0}}, P_ADD2, {}, dt), gmap(1, {17, 5}, {{0, 1}, {1, 0}}, P_ADD2, {}, dt), gmap(2, {3, 3, 3}, {{0, 1, 2}, {2, 1, 0}}, P_ADD2, {}, dt),
                                    gmap(3, {24, 28, 20}, {{1, 2, 0}, {2, 0, 1}}, P_ADD2, {}, dt)});
        plan_one_group("prog " + t, {gmap(0, {17, 5}, {{0, 1}, {1, 0}}, P_PROG, {3, 0}, dt), gmap(1, {40, 33}, {{0, 1}, {1, 0}}, P_PROG, {3, 0}, dt), gmap(2, {3, 3, 3}, {{0, 1, 2}, {2, 1, 0}}, P_PROG, {3, 0}, dt)}, IND);
    }
    // a bitcopy group (every integer width), a mixed group (Float32 inputs, Float64 destination) and an integer group (Int64 sums)
    for (int dt : {SMR_I8, SMR_I16, SMR_I32, SMR_U64}) plan_one_group("bitcopy dtype=" + std::to_string(dt), {gcopy(0, {6, 5}, dt), gmap(1, {31, 33}, {{1, 0}}, P_IDENT, {}, dt), gcopy(2, {1025}, dt)});
    plan_one_group("mixed", {gmap(0, {6, 5}, {{0, 1}}, P_IDENT, {}, SMR_F64, SMR_F32), gmap(1, {33, 40}, {{1, 0}}, P_IDENT, {}, SMR_F64, SMR_F32), gmap(2, {12}, {{0}}, P_IDENT, {}, SMR_F64, SMR_F32)});
    plan_one_group("mixed scale own", {gmap(0, {4, 4}, {{0, 1}}, P_SCALE, {0.1, 0}, SMR_F32), gmap(1, {4, 4}, {{0, 1}}, P_SCALE, {1.1, 0}, SMR_F32)}, OWN);
    plan_one_group("integer add2", {gmap(0, {6, 5}, {{0, 1}, {1, 0}}, P_ADD2, {}, SMR_I64), gmap(1, {40, 33}, {{0, 1}, {1, 0}}, P_ADD2, {}, SMR_I64)});
    plan_one_group("integer scale own", {gmap(0, {4, 4}, {{0, 1}}, P_SCALE, {3, 0}, SMR_I32), gmap(1, {4, 4}, {{0, 1}}, P_SCALE, {5, 0}, SMR_I32)}, OWN);
    // scalar rows: differing, bit-equal, -0.0 against 0.0 (differing), an f without constants; Canon::fc rows and ProgD::consts rows
    auto scaled = [&](std::initializer_list<double> cs) {
        Ms ms;
        for (double v : cs) ms.push_back(gmap((int)ms.size(), {4, 4}, {{0, 1}}, P_SCALE, {v, 0}));
        return ms;
    };
    plan_one_group("scalars differ", scaled({1, 1.125, 1.25}), OWN);
    plan_one_group("scalars differ independent", scaled({1, 1.125, 1.25}), OWN | IND);
    plan_one_group("scalars equal", scaled({2.5, 2.5, 2.5}), OWN);
    plan_one_group("scalars equal, no flag", scaled({2.5, 2.5, 2.5}));
    plan_one_group("scalars 0.0 and -0.0", scaled({0.0, -0.0}), OWN);
    plan_one_group("scalars of an f without constants", {gcopy(0, {4, 4}), gcopy(1, {4, 4})}, OWN);
    for (const Prog* f : {&P_AXPBY, &P_AXPY, &P_PROG}) {
        Ms ms;
        for (int i = 0; i < 3; ++i) ms.push_back(gmap(i, {33, 40}, {{0, 1}, {1, 0}}, *f, {1 + i / 8.0, 0, 2 - i / 16.0, 0}));
        if (f != &P_AXPBY)
            for (auto& m : ms) m.nconsts = 1;
        plan_one_group(std::string("scalars rows of ") + (f == &P_AXPBY ? "axpby" : (f == &P_AXPY ? "axpy" : "prog")), ms, OWN);
    }
    plan_one_group("scalars complex", {gmap(0, {4, 4}, {{0, 1}}, P_SCALE, {2, 1}, SMR_C64), gmap(1, {4, 4}, {{0, 1}}, P_SCALE, {2, -1}, SMR_C64)}, OWN);
    // SMR_GROUP_INDEPENDENT: even and odd columns of one parent into even and odd columns of another; shared inputs, an in-place member
    auto interleaved = [&](bool contraction) {
        Ms ms;
        for (int j = 0; j < 2; ++j) {
            smr_problem p = contraction ? gmm(j, 16, 8, 5) : gcopy(j, {8, 4});
            for (int k = 0; k < (contraction ? 1 : 2); ++k) {
                p.ops[k].base = gaddr(0, k);
                p.ops[k].offset = j * p.dims[0];
                p.ops[k].strides[1] = 2 * p.dims[0];
            }
            ms.push_back(p);
        }
        return ms;
    };
    plan_one_group("interleaved maps", interleaved(false), 0, true);
    plan_one_group("interleaved maps independent", interleaved(false), IND);
    plan_one_group("interleaved contractions", interleaved(true), 0, true);
    plan_one_group("interleaved contractions independent", interleaved(true), IND);
    {
        smr_problem ab = gcopy(0, {4, 4}), bc = gcopy(1, {4, 4}), ac = gcopy(1, {4, 4}), dd = gcopy(2, {4, 4});
        bc.ops[1].base = ab.ops[0].base;  // reads what member 0 writes
        ac.ops[1].base = ab.ops[1].base;  // shares member 0's input
        dd.ops[1].base = dd.ops[0].base;  // in place
        plan_one_group("chain", {ab, bc}, 0, true);
        plan_one_group("shared input, in place", {ab, ac, dd});
    }
    // refusals of map groups
    {
        smr_problem red = problem({8, 8}, SMR_F64, {{0, 1}}, DISTINCT, 0u, true), bad = gcopy(1, {6, 5});
        bad.dims[0] = 0;
        plan_one_group("refused: a reduction in a map group", {gcopy(0, {6, 5}), red}, 0, true);
        plan_one_group("refused: dtype", {gcopy(0, {6, 5}), gcopy(1, {6, 5}), gcopy(2, {6, 5}, SMR_F32)}, 0, true);
        plan_one_group("refused: another constant", scaled({2, 3}), 0, true);
        plan_one_group("refused: another program", {scaled({2})[0], gmap(1, {4, 4}, {{0, 1}}, P_PLUSC, {2, 0})}, 0, true);
        plan_one_group("refused: a malformed member", {gcopy(0, {6, 5}), bad}, 0, true);
        plan_one_group("refused: another number of operands", {gcopy(0, {6, 5}), gmap(1, {6, 5}, {{0, 1}, {1, 0}}, P_ADD2)}, 0, true);
        plan_one_group("refused: converting and not", {gcopy(0, {6, 5}), gmap(1, {6, 5}, {{0, 1}}, P_IDENT, {}, SMR_F64, SMR_F32)}, 0, true);
        smr_problem cj = gcopy(1, {6, 5}, SMR_C64);
        cj.ops[1].conj = 1;
        plan_one_group("refused: dtype of a bit copy", {gcopy(0, {6, 5}, SMR_I32), gcopy(1, {6, 5}, SMR_U32)}, 0, true);
        plan_one_group("refused: conj flag", {gcopy(0, {6, 5}, SMR_C64), cj}, 0, true);
        plan_one_group("refused own: another program", {scaled({2})[0], gmap(1, {4, 4}, {{0, 1}}, P_PLUSC, {2, 0})}, OWN, true);
        plan_one_group("refused own: another program in member 2", {scaled({2})[0], gmap(1, {4, 4}, {{0, 1}}, P_SCALE, {5, 0}), gmap(2, {4, 4}, {{0, 1}}, P_PLUSC, {2, 0})}, OWN, true);
        plan_one_group("refused own: a complex scalar among real ones", {scaled({2})[0], gmap(1, {4, 4}, {{0, 1}}, P_SCALE, {2, 1})}, OWN, true);
        plan_one_group("refused own: leaves the integer class", {gmap(0, {4, 4}, {{0, 1}}, P_SCALE, {3, 0}, SMR_I32), gmap(1, {4, 4}, {{0, 1}}, P_SCALE, {2.5, 0}, SMR_I32)}, OWN, true);
        smr_problem merged = gmap(1, {4, 4}, {{0, 1}, {1, 0}}, P_AXPBY_MERGED, {2, 0});
        plan_one_group("refused own: equal constants merged", {gmap(0, {4, 4}, {{0, 1}, {1, 0}}, P_AXPBY, {2, 0, 3, 0}), merged}, OWN, true);
        const Options saved = options();
        options().jit = 0;
        plan_one_group("refused: a math opcode without runtime compilation", {gmap(0, {6, 5}, {{0, 1}, {1, 0}}, P_MATH)}, 0, true);
        options() = saved;
        plan_one_group("refused: box elements", {gcopy(0, {6, 5}), gcopy(1, {65536, 32768})}, 0, true);
        Ms many;  // 46340^2 elements are 2097066 workgroups: the sum crosses 2^31 - 1 at member 1024
        for (int i = 0; i < 1100; ++i) many.push_back(gcopy(0, {46340, 46340}));
        plan_one_group("refused: workgroups", many, IND, true);
    }
    // contraction groups: the rule's tile (16 x 16 under a workgroup per CU or under half-full 32 x 32 tiles, else 32 x 32), both forced
    // tiles, ragged and whole tiles, padded parents (no vector loads), k-major inputs, a batch dim, two reduced dims, beta per member
    auto blocks = [&](int count, i64 m, i64 n, i64 k, int dt = SMR_F64) {
        Ms ms;
        for (int i = 0; i < count; ++i) ms.push_back(gmm(i % 2048, m, n, k, dt));
        return ms;
    };
    for (i64 tile : {0, 16, 32}) {
        const std::string t = " tile=" + std::to_string(tile);
        plan_one_group("contract 255 x 32^3" + t, blocks(255, 32, 32, 32), 0, false, tile);
        plan_one_group("contract 256 x 32^3" + t, blocks(256, 32, 32, 32), 0, false, tile);
        plan_one_group("contract 300 x 17x17x8" + t, blocks(300, 17, 17, 8), 0, false, tile);
        plan_one_group("contract 300 x 24x24x8" + t, blocks(300, 24, 24, 8), 0, false, tile);
        for (int dt : {SMR_F32, SMR_F64, SMR_C32, SMR_C64, SMR_I64}) {
            const i64 tk = contract_tk(dtype_size(dt), 1);
            Ms ms = {gmm(0, 15, 2, 2, dt), gmul(1, {48, 48, 3, 2}, 3, dt, 2u), gmm(2, 32, 32, tk, dt), gmm(3, 32, 32, 2 * tk, dt, 6u), gmm(4, 32, 32, 2 * tk + 1, dt, 2u),
                     gmm(5, 32, 32, tk + 1, dt, 0, 1), gmm(6, 33, 17, 2 * tk + 1, dt, 4u, 1), gmul(7, {17, 33, 3, tk + 1}, 3, dt, 2u), gmul(8, {33, 15, tk + 1, 2}, 2, dt),
                     gmm(9, 17, 31, 5, dt, 6u), gmm(10, 31, 17, 5, dt), gmm(11, 2, 15, tk, dt, 2u)};
            for (size_t i = 0; i < ms.size(); ++i) {
                ms[i].initop = SMR_INIT_SCALE;
                ms[i].initarg[0] = 2 + (double)(i % 3);
            }
            plan_one_group("contract paths dtype=" + std::to_string(dt) + t, ms, 0, false, tile);
            plan_one_group("contract one dtype=" + std::to_string(dt) + t, {gmm(0, 15, 16, tk + 1, dt, 4u)}, 0, false, tile);
        }
    }
    {
        Ms dist = blocks(3, 20, 24, 9), mn = blocks(3, 20, 24, 9), cst = blocks(2, 20, 24, 9);
        for (auto& m : dist) set_f(m, P_DIST);
        for (auto& m : mn) { m.redop = SMR_RED_MIN; m.initop = SMR_INIT_NONE; }
        for (size_t i = 0; i < cst.size(); ++i) { cst[i].initop = SMR_INIT_CONST; cst[i].initarg[0] = 2 + (double)i; }
        plan_one_group("contract another f", dist);
        plan_one_group("contract min", mn);
        plan_one_group("contract const beta", cst);
        plan_one_group("contract two shapes", {gmm(0, 20, 24, 9, SMR_F32), gmm(1, 33, 17, 5, SMR_F32)});
        Ms mixed = blocks(2, 20, 24, 9, SMR_F32);
        for (auto& m : mixed) m.ops[0].dtype = SMR_F64;
        plan_one_group("contract converting", mixed);
        const Options saved = options();
        options().max_lds_bytes = 20000;
        plan_one_group("contract 32 forced, 20000 bytes of LDS", blocks(255, 32, 32, 32), 0, false, 32);
        options().max_lds_bytes = 1000;
        plan_one_group("refused: max_lds_bytes", blocks(2, 32, 32, 32), 0, true);
        options() = saved;
    }
    // refusals of contraction groups
    {
        const smr_problem ok = gmm(0, 20, 24, 9), ok1 = gmm(1, 20, 24, 9), plain = problem({8, 8}, SMR_F64, {{0, 1}}, DISTINCT, 0u, true);
        smr_problem mx = gmm(2, 20, 24, 9), sc = gmm(0, 20, 24, 9, SMR_F64, 0, 0, SMR_INIT_SCALE, 2), c2 = ok, c3 = ok1, onbuf = gmm(1, 8, 4, 4);
        mx.redop = SMR_RED_MAX;
        set_f(c2, P_MULC, {2, 0});
        set_f(c3, P_MULC, {3, 0});
        onbuf.ops[1].base = onbuf.ops[0].base;  // C[:, 0:4] = C[:, 4:8] * B
        onbuf.ops[1].offset = 32;
        plan_one_group("refused: a map in a contraction group", {ok, ok1, gcopy(2, {6, 5})}, 0, true);
        plan_one_group("refused: member 0 is another reduction", {plain}, 0, true);
        plan_one_group("refused: member 1 is another reduction", {ok, plain}, 0, true);
        plan_one_group("refused: m = 1", {ok, gmm(1, 1, 24, 9)}, 0, true);
        plan_one_group("refused: another op", {ok, ok1, mx}, 0, true);
        plan_one_group("refused: another kind of initop", {sc, ok1}, 0, true);
        plan_one_group("refused: another alpha", {c2, c3}, 0, true);
        plan_one_group("refused: dtype of a contraction", {ok, gmm(1, 20, 24, 9, SMR_F32)}, 0, true);
        plan_one_group("refused: an input on the destination's buffer", {ok, onbuf}, 0, true);
        plan_one_group("refused: member scalars of a contraction group", {ok, ok1}, OWN, true);
        plan_one_group("refused: a contraction in a map group", {gcopy(0, {6, 5}), ok1}, 0, true);
        plan_one_group("refused: box elements of a contraction", {ok, gmm(1, 32768, 32768, 2)}, 0, true);
        Ms many;  // 2^21 tiles of 16 x 16 each: the sum crosses 2^31 - 1 at member 1023
        for (int i = 0; i < 1100; ++i) many.push_back(gmm(0, 32768, 16384, 2));
        plan_one_group("refused: workgroups of a contraction group", many, IND, true, 16);
    }
}

// ---- the split form of CONTRACT ("contract_split", "contract_tile") -------------------------------------------------------------------
// The generic product box (m, n, k[, k2]) planned with the two options set: "split <id> contract=<c> split=<s> tile=<t>".  Both outcomes
// of the rule (split; left alone: one chunk, enough workgroups already, the partials too large for the inputs), every tile by the rule
// and forced, forced slices, slices clamped to the chunks, a forced tile beyond the LDS budget (refused: REDUCE_PART).
enum { S_RULE_SPLIT, S_RULE_LEFT, S_TILE16, S_TILE32, S_TILE64, S_FORCED, S_CLAMPED, S_REFUSED, S_TWO_REDUCED, S_COUNT };
static const char* sname[] = {"split_by_rule", "rule_leaves_alone", "split_tile_16", "split_tile_32", "split_tile_64", "split_forced", "split_clamped", "split_tile_refused", "split_two_reduced_dims"};
static const long sneed[S_COUNT] = {6, 6, 6, 6, 6, 12, 6, 3, 12};
static long scounts[S_COUNT];

static smr_problem mul_box(const std::vector<i64>& dims, int dt) {
    // C (m, n), A (m, k[, k2]) column-major, B (n, k[, k2]) with k fastest; with two reduced dims the parents are padded by one
    // along k, so that the two do not fuse into one (Q > 1: slices that start inside and between outer reduced indices)
    const int N = (int)dims.size();
    smr_problem p = problem(dims, dt, {rotation(N, 0), rotation(N, 0)}, DISTINCT, 3u, true);
    i64 sa = dims[0], sb = 1;
    for (int d = 0; d < N; ++d) p.ops[1].strides[d] = p.ops[2].strides[d] = 0;
    p.ops[1].strides[0] = 1;
    for (int d = 2; d < N; ++d) {
        p.ops[1].strides[d] = sa;
        sa *= dims[d] + (N > 3 && d == 2 ? 1 : 0);
        p.ops[2].strides[d] = sb;
        sb *= dims[d] + (N > 3 && d == 2 ? 1 : 0);
    }
    p.ops[2].strides[1] = sb;
    static const uint8_t mul[] = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_MUL, 0};
    p.fprog = mul;
    p.fprog_len = 3;
    return p;
}

static void split_line(const std::string& id, const smr_problem& p, i64 contract, i64 split, i64 tile, i64 lds = 65536) {
    const Options saved = options();
    options().contract = contract;
    options().contract_split = split;
    options().contract_tile = tile;
    options().max_lds_bytes = lds;
    Plan plan;
    const int rc = make_plan(&p, plan);
    options() = saved;
    if (rc) {
        std::printf("split %s contract=%lld split=%lld tile=%lld rc=%d\n", id.c_str(), (long long)contract, (long long)split, (long long)tile, rc);
        return;
    }
    std::printf("split %s contract=%lld split=%lld tile=%lld | %s | %016llx\n", id.c_str(), (long long)contract, (long long)split, (long long)tile, plan.desc.c_str(),
                (unsigned long long)digest(plan));
    const ContractPlan& k = plan.contract;
    const bool is_split = plan.family == FAM_CONTRACT && k.kparts > 1;
    if (split == 1) ++scounts[is_split ? S_RULE_SPLIT : S_RULE_LEFT];
    if (is_split) ++scounts[k.rb == 1 ? S_TILE16 : (k.rb == 2 ? S_TILE32 : S_TILE64)];
    if (split >= 2 && is_split) ++scounts[k.kparts == split ? S_FORCED : S_CLAMPED];
    if (tile && lds < 65536 && plan.family != FAM_CONTRACT) ++scounts[S_REFUSED];
    if (is_split && plan.c.N - plan.c.NK > 1) ++scounts[S_TWO_REDUCED];  // (the reduced dims did not fuse: Q > 1)
}

static void split_corpus() {
    const std::vector<std::vector<i64>> boxes = {{64, 64, 4096},   {64, 64, 65536}, {32, 32, 1048576}, {128, 128, 16384}, {256, 256, 4096}, {16, 512, 32768},
                                                 {100, 90, 80},    {1024, 1024, 1024}, {64, 64, 512, 64}, {40, 40, 40},   {128, 128, 64},   {512, 512, 512},
                                                 {256, 256, 256},  {65, 63, 193},   {33, 33, 97, 3},   {2048, 2048, 64}};
    for (const auto& dims : boxes)
        for (int dt : {SMR_F32, SMR_F64, SMR_C64}) {
            const smr_problem p = mul_box(dims, dt);
            const std::string id = ident(dims, dt, {}, "product");
            for (i64 contract : {1, 2}) split_line(id, p, contract, 1, 0);           // the rule
            for (i64 tile : {16, 32, 64}) split_line(id, p, 2, 1, tile);              // the rule on a forced tile
            for (i64 s : {2, 3, 8, 64, 100000})                                       // forced slices (clamped to the chunks, or refused: too large)
                for (i64 tile : {0, 16, 32, 64}) split_line(id, p, 2, s, tile);
            split_line(id, p, 2, 4, 64, 8192);                                        // the forced tile does not fit: REDUCE_PART
        }
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
    split_corpus();
    group_corpus();
    split_group_corpus();
    scalars_group_corpus();
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
    for (const char* form : form_need) {
        const long n = form_counts[form];
        std::fprintf(stderr, "  args %s: %ld%s\n", form, n, n < form_min ? "  -- TOO FEW: the corpus no longer reaches this form of the argument builders" : "");
        if (n < form_min) rc = 1;
    }
    std::fprintf(stderr, "%ld group lines, %ld accepted or refused against the recipe's word\n", glines, gwrong);
    if (gwrong) rc = 1;
    for (int i = 0; i < S_COUNT; ++i) {
        std::fprintf(stderr, "  %s: %ld%s\n", sname[i], scounts[i], scounts[i] < sneed[i] ? "  -- TOO FEW: the split corpus no longer covers this" : "");
        if (scounts[i] < sneed[i]) rc = 1;
    }
    for (int i = 0; i < G_COUNT; ++i) {
        std::fprintf(stderr, "  %s: %ld%s\n", gname[i], gcounts[i], gcounts[i] < gneed[i] ? "  -- TOO FEW: the group corpus no longer covers this" : "");
        if (gcounts[i] < gneed[i]) rc = 1;
    }
    return rc;
}
