// smr_k_gcontract.hip -- contraction groups: K small independent outer-product reductions (the generic __mul! box; one f, one op,
// the same operand types; rank, extents, strides, pointers and beta of their own) in ONE launch of 256-lane workgroups.
//
// Every member is tiled like a single call of FAM_CONTRACT (smr_k_contract.hip) with ONE tile size for the whole launch, 16 x 16
// or 32 x 32 (RB = 1 or 2; the group planner, smr_plan_group.cpp, picks it); a member's workgroups are its nti * ntj * rest tiles and
// the grid is their sum.  A workgroup finds its member by the binary search it shares with the map groups (smr_group.h:
// group_member_of) over the prefix sums first_wg[] with its index in the group, blockIdx.x + wg0 -- a launch may be one contiguous block range of the group, which is
// how a recorded sequence cuts it -- decodes its index inside the member into (tile along di, tile along dj, rest) and runs the
// family's tile body (smr_contract.h: contract_impl) in one of its three copies: bounds-free for whole tiles, with 16-byte global
// loads where the member's own `vec` allows, clamped for ragged tiles.  The sum has the copy with the operator fixed.
//
// The member's descriptor (smr_group.h: GroupContractMemberD) stays in the device table and is read in place through the
// constant address space: the tile body indexes strides[k][NK], dims[di], ... with run-time indices, all wave-uniform, so each is
// a scalar load.  The body is a template over the geometry's type for that reason.
//
// ACCUMULATION ORDER: the single call's.  One lane owns each output, starting from the neutral element, q ascending and inside it k
// ascending, the init-ed old destination combined last -- whatever the tile.  A member's result is bit-identical to the single
// call's on that member alone.  No partials, no scratch, one launch.
//
// SPLIT FORM (option "group_contract_split", off by default; smr_plan_group.cpp: contract_group_rule): a few members with small open
// legs and a very long reduced range.  Member i's chunk walk is cut into S_i slices of cps_i chunks by the single call's arithmetic
// (smr_contract.h: contract_slices) and the member has tiles_i * S_i workgroups in the main launch, the slice the slow digit as in
// contract_split_body.  A workgroup of a split member (S_i >= 2) runs the tile body over its slice from the neutral element and
// stores its register block -- compute-class values, no conversion, no conj, no initop; ragged tiles store all their lanes -- to the
// group's partials at part_off_i + (tile * S_i + slice) * RB^2 * 256; a workgroup of an unsplit member (S_i == 1) runs the body above
// and finishes its outputs in this launch.  The branch is on the member: wave-uniform.  k_group_contract_fold, the grouped form of
// k_contract_fold, then runs RB^2 workgroups per tile of the split members only (a second prefix table, searched by the same
// group_member_of), one lane per output: P_0 .. P_{S-1} folded in slice order, the result through the epilogue with the member's beta.
// ACCUMULATION ORDER of a split member: the split single call's, dest = op(initop(old), op(... op(P_0, P_1) ..., P_{S-1})) -- bit-
// identical to the single call on that member under contract = 2, contract_tile = the group's tile, contract_split = S_i.
// Compiled once per compute type (-DSMR_CT=n), and a second time with -DSMR_GCONTRACT_SPLIT: the split form's two kernels and their
// entry point in objects of their own, so that k_group_contract's code objects are those of the library before the split form
// (kernels added to a translation unit change the register allocation of the ones it held: profiles/contract_split.txt).
//
// PER-MEMBER CONSTANTS OF f (SMR_GROUP_CONTRACT_SCALARS, GroupContractPlan::varc): an alpha per block.  A third table holds one row of
// W doubles per member (ProgD::consts of the member's own canonicalisation); group_contract_varc_body / group_contract_split_varc_body
// are the two bodies above plus one step: right after the member search the workgroup rebuilds f's constants from the row of its
// MEMBER (set_consts, smr_device.h; wave-uniform index, constant address space: scalar loads) -- every tile and every slice of a
// member reads the same row -- before any data load.  The fold launch does not call f and is the split form's kernel, as it is
// (instantiated in these objects a second time).  Natively
// compiled: the mul! form x * y * alpha (FMul2Scale); every other f with constants, and every mixed group, is a program whose
// runtime-compiled text depends on f's structure only.  A third pass, -DSMR_GCONTRACT_VARC, compiles these kernels and their entry
// points into objects of their own, for the reason given above.
#include "smr_contract.h"
#include "smr_group.h"

#ifndef SMR_CT
#error "compile with -DSMR_CT=0..3 or 7"
#endif

namespace smr {

struct GroupContractArgs {
    const GroupContractMemberD* members;
    const uint32_t* first_wg;  // count + 1 prefix sums
    int32_t count;
    uint32_t wg0;              // first workgroup of this launch within the group (0: the launch is the whole group)
    int32_t redop, pad;
    int32_t dtype[3];
    int32_t conj[3];
};

template <class T, class F, bool MIXED, int RB>
SMR_DEV void group_contract_body(const GroupContractArgs a, F f) {
    typedef CGeom<T, RB> G;
    __shared__ __attribute__((aligned(16))) T lds[2 * 2 * G::TK * G::LD];
    static_assert(sizeof(T) * 2 * 2 * G::TK * G::LD == contract_lds(G::ES, RB), "the planner's LDS figure is the kernel's");
    // the member of this workgroup, by its index in the group (smr_group.h: group_member_of)
    const uint32_t b = blockIdx.x + a.wg0;
    GroupWordC* const first_wg = (GroupWordC*)a.first_wg;
    const int lo = group_member_of(first_wg, a.count, b);
    GroupContractMemberC& m = ((GroupContractMemberC*)a.members)[lo];
    // (not group_contract_optab below: this body is left textually as it was, so that k_group_contract's code objects stay the ones
    // of the library before the split form)
    OpTab t;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
        t.base[k] = nullptr;
        t.dtype[k] = 0;
        t.conj[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.base[k] = m.base[k];
        t.dtype[k] = a.dtype[k];
        t.conj[k] = a.conj[k];
    }
    contract_by_op<T, F, MIXED, RB, false>(m, t, a.redop, f, lds, (i64)(b - first_wg[lo]), 0, m.Q * m.nkc, (T*)nullptr);
}

// the split form's arguments: the unsplit ones first (wg0 keeps its kernarg offset), the tables of the split form, the partials
struct GroupContractSplitArgs {
    GroupContractArgs g;
    const GroupSplitD* split;      // count entries
    const uint32_t* fold_first;    // count + 1 prefix sums of the fold launch's workgroups
    void* partials;
};

// the operand table of member `m` in registers
SMR_DEV OpTab group_contract_optab(GroupContractMemberC& m, const GroupContractArgs& a) {
    OpTab t;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
        t.base[k] = nullptr;
        t.dtype[k] = 0;
        t.conj[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.base[k] = m.base[k];
        t.dtype[k] = a.dtype[k];
        t.conj[k] = a.conj[k];
    }
    return t;
}

// The split form's main launch: workgroup w of member i is (tile = w % tiles_i, slice = w / tiles_i) when S_i >= 2, tile w otherwise.
template <class T, class F, bool MIXED, int RB>
SMR_DEV void group_contract_split_body(const GroupContractSplitArgs a, F f) {
    typedef CGeom<T, RB> G;
    __shared__ __attribute__((aligned(16))) T lds[2 * 2 * G::TK * G::LD];
    const uint32_t b = blockIdx.x + a.g.wg0;
    GroupWordC* const first_wg = (GroupWordC*)a.g.first_wg;
    const int lo = group_member_of(first_wg, a.g.count, b);
    GroupContractMemberC& m = ((GroupContractMemberC*)a.g.members)[lo];
    GroupSplitC& sp = ((GroupSplitC*)a.split)[lo];
    const OpTab t = group_contract_optab(m, a.g);
    const i64 w = (i64)(b - first_wg[lo]), nchunks = m.Q * m.nkc;
    const i64 S = (i64)sp.S;
    if (S < 2) {  // (wave-uniform: sp is the member's)
        contract_by_op<T, F, MIXED, RB, false>(m, t, a.g.redop, f, lds, w, 0, nchunks, (T*)nullptr);
        return;
    }
    const i64 tiles = (i64)sp.tiles, sl = w / tiles, tile = w - sl * tiles;
    const i64 t_lo = sl * sp.cps, t_hi = t_lo + sp.cps < nchunks ? t_lo + sp.cps : nchunks;
    T* sink = (T*)a.partials + sp.part_off + (tile * S + sl) * (i64)(RB * RB * 256);
    contract_by_op<T, F, MIXED, RB, true>(m, t, a.g.redop, f, lds, tile, t_lo, t_hi, sink);
}

// per-member constants: the argument block behind the existing fields (wg0 keeps its kernarg offset), and the two bodies
struct GroupConstsArgs {
    int32_t W, pad;        // doubles per row of `consts`
    const double* consts;  // count rows of f's constants, one per member
};
struct GroupContractVarcArgs {
    GroupContractArgs g;
    GroupConstsArgs k;
};
struct GroupContractSplitVarcArgs {
    GroupContractSplitArgs s;
    GroupConstsArgs k;
};

template <class T, class F, bool MIXED, int RB>
SMR_DEV void group_contract_varc_body(const GroupContractVarcArgs a, F f) {
    typedef CGeom<T, RB> G;
    __shared__ __attribute__((aligned(16))) T lds[2 * 2 * G::TK * G::LD];
    const uint32_t b = blockIdx.x + a.g.wg0;
    GroupWordC* const first_wg = (GroupWordC*)a.g.first_wg;
    const int lo = group_member_of(first_wg, a.g.count, b);
    f.set_consts((GroupConstC*)a.k.consts + (i64)lo * a.k.W);  // the member's row: not the workgroup's, not the slice's
    GroupContractMemberC& m = ((GroupContractMemberC*)a.g.members)[lo];
    const OpTab t = group_contract_optab(m, a.g);
    contract_by_op<T, F, MIXED, RB, false>(m, t, a.g.redop, f, lds, (i64)(b - first_wg[lo]), 0, m.Q * m.nkc, (T*)nullptr);
}

template <class T, class F, bool MIXED, int RB>
SMR_DEV void group_contract_split_varc_body(const GroupContractSplitVarcArgs a, F f) {
    typedef CGeom<T, RB> G;
    __shared__ __attribute__((aligned(16))) T lds[2 * 2 * G::TK * G::LD];
    const uint32_t b = blockIdx.x + a.s.g.wg0;
    GroupWordC* const first_wg = (GroupWordC*)a.s.g.first_wg;
    const int lo = group_member_of(first_wg, a.s.g.count, b);
    f.set_consts((GroupConstC*)a.k.consts + (i64)lo * a.k.W);  // the member's row: not the workgroup's, not the slice's
    GroupContractMemberC& m = ((GroupContractMemberC*)a.s.g.members)[lo];
    GroupSplitC& sp = ((GroupSplitC*)a.s.split)[lo];
    const OpTab t = group_contract_optab(m, a.s.g);
    const i64 w = (i64)(b - first_wg[lo]), nchunks = m.Q * m.nkc;
    const i64 S = (i64)sp.S;
    if (S < 2) {  // (wave-uniform: sp is the member's)
        contract_by_op<T, F, MIXED, RB, false>(m, t, a.s.g.redop, f, lds, w, 0, nchunks, (T*)nullptr);
        return;
    }
    const i64 tiles = (i64)sp.tiles, sl = w / tiles, tile = w - sl * tiles;
    const i64 t_lo = sl * sp.cps, t_hi = t_lo + sp.cps < nchunks ? t_lo + sp.cps : nchunks;
    T* sink = (T*)a.s.partials + sp.part_off + (tile * S + sl) * (i64)(RB * RB * 256);
    contract_by_op<T, F, MIXED, RB, true>(m, t, a.s.g.redop, f, lds, tile, t_lo, t_hi, sink);
}

#ifndef SMR_JIT
#if defined(SMR_GCONTRACT_SPLIT) || defined(SMR_GCONTRACT_VARC)
// The split form's second launch, the grouped form of k_contract_fold: workgroup w of split member i is (register = w % RB^2, tile =
// w / RB^2); one lane per (tile, register, lane) of the main launch folds that output's S_i partials in slice order, acc = P_0; acc =
// op(acc, P_s) for s = 1 .. S_i - 1, and puts the result through the epilogue with the member's own beta; lanes past the end of a
// ragged tile drop theirs.  It does not call f.  Eight partials are loaded (index clamped, never guarded) before the first is used.
template <class T, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_group_contract_fold(GroupContractSplitArgs a) {
    typedef CGeom<T, RB> G;
    const uint32_t b0 = blockIdx.x;
    GroupWordC* const fold_first = (GroupWordC*)a.fold_first;
    const int lo = group_member_of(fold_first, a.g.count, b0);
    GroupContractMemberC& g = ((GroupContractMemberC*)a.g.members)[lo];
    GroupSplitC& sp = ((GroupSplitC*)a.split)[lo];
    const OpTab t = group_contract_optab(g, a.g);
    i64 b = (i64)(b0 - fold_first[lo]);
    const int reg = (int)(b % (RB * RB));
    b /= RB * RB;
    const int kparts = (int)sp.S;
    const T* p = (const T*)a.partials + sp.part_off + b * kparts * (i64)(RB * RB * 256) + reg * 256 + (int)threadIdx.x;
    const i64 bi = b % g.nti;
    b /= g.nti;
    const i64 bj = b % g.ntj;
    b /= g.ntj;
    i64 off0 = 0;
#pragma nounroll
    for (int n = 0; n < g.nrd; ++n) {
        const int d = g.rdim[n];
        const i64 x = b / g.dims[d], cd = b - x * g.dims[d];
        b = x;
        off0 += cd * g.strides[0][d];
    }
    const int li = (int)threadIdx.x & (CONTRACT_LANES - 1), lj = (int)threadIdx.x >> 4;
    const i64 i = bi * G::TILE + G::idx(li, reg / RB), j = bj * G::TILE + G::idx(lj, reg % RB);
    if (i >= g.dims[g.di] || j >= g.dims[g.dj]) return;
    constexpr i64 SL = RB * RB * 256;  // elements between the slices of one tile
    const int last = kparts - 1;
    T acc = p[0];
    for (int s0 = 1; s0 <= last; s0 += 8) {
        T x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = p[(i64)(s0 + e < last ? s0 + e : last) * SL];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const T v = red_apply<T>(a.g.redop, acc, x[e]);
            if (s0 + e <= last) acc = v;
        }
    }
    contract_epilogue<T, MIXED>(g, t, off0 + i * g.strides[0][g.di] + j * g.strides[0][g.dj], acc);
}
#endif

#if defined(SMR_GCONTRACT_VARC)
template <class T, class F, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_group_contract_varc(GroupContractVarcArgs a, F f) {
    group_contract_varc_body<T, F, MIXED, RB>(a, f);
}

template <class T, class F, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_group_contract_split_varc(GroupContractSplitVarcArgs a, F f) {
    group_contract_split_varc_body<T, F, MIXED, RB>(a, f);
}

// the unsplit arguments of a planned group (what go_gc / go_gcs fill), and its table of constants
static void fill_gc(const GroupPlan& g, GroupContractArgs& a) {
    const Canon& c = g.c;
    std::memset(&a, 0, sizeof a);
    a.members = (const GroupContractMemberD*)g.d_members;
    a.first_wg = (const uint32_t*)g.d_first;
    a.count = (int32_t)g.contract.members.size();
    a.wg0 = 0;
    a.redop = c.redop;
    for (int k = 0; k < 3; ++k) {
        a.dtype[k] = c.dtype[k];
        a.conj[k] = c.conj[k];
    }
}
static int fill_consts(const GroupPlan& g, GroupConstsArgs& k) {
    const GroupContractPlan& cp = g.contract;
    // (a dry run compiles without a device: no tables yet, and nothing is launched)
    if (!cp.varc || cp.W < 1 || (!jit_dry_run() && !cp.d_consts)) return set_error(SMR_EINVAL, "contraction group: per-member constants planned without their table");
    k.W = cp.W;
    k.pad = 0;
    k.consts = (const double*)cp.d_consts;
    return SMR_OK;
}

template <class T, class F, bool MIXED, int RB>
static int launch_gcv(const Canon& c, const GroupContractVarcArgs& a, unsigned grid, hipStream_t s, F f) {
    // sliceable like k_group_contract: wg0 has the kernarg offset it has there, and the row is found from the member
    mark_sliceable(1, (unsigned)(offsetof(GroupContractVarcArgs, g) + offsetof(GroupContractArgs, wg0)), 0);
    if constexpr (is_jit<F>::value)  // the kernel argument kc holds member 0's constants and goes unused; the text depends on f's structure only
        return launch_jit<T>(c, s, "gcontract", "smr::GroupContractVarcArgs", "group_contract_varc_body", "", grid, 256, 0, a, MIXED, RB);
    else
        return launch_native(nullptr, 0, "k_group_contract_varc", [&] { SMR_LAUNCH((k_group_contract_varc<T, F, MIXED, RB>), dim3(grid), dim3(256), 0, s, a, f); });
}

template <class T, class F, bool MIXED>
static int go_gcv(const GroupPlan& g, hipStream_t s, F f) {
    GroupContractVarcArgs a;
    fill_gc(g, a.g);
    if (int rc = fill_consts(g, a.k)) return rc;
    const unsigned grid = g.first_wg.back();
    if (g.contract.rb == 2) return launch_gcv<T, F, MIXED, 2>(g.c, a, grid, s, f);
    if (g.contract.rb == 1) return launch_gcv<T, F, MIXED, 1>(g.c, a, grid, s, f);
    return set_error(SMR_EINVAL, "contraction group: no kernel for this tile");
}

template <>
int launch_group_contract_varc_ct<SMR_CT>(const GroupPlan& g, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = g.c;
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go_gcv<T, decltype(f), true>(g, s, f); });
    // natively compiled: the mul! form x * y * alpha (the planner recognised it); every other f is runtime-compiled or interpreted
    if (g.contract.mul2scale) return go_gcv<T, FMul2Scale<T>, false>(g, s, FMul2Scale<T>{});
    return with_prog<T>(c, [&](auto f) { return go_gcv<T, decltype(f), false>(g, s, f); });
}

// the two launches of the split form: the members' (tile, slice) workgroups with their rows, then the split form's fold as it is
template <class T, class F, bool MIXED, int RB>
static int launch_gcsv(const GroupPlan& g, const GroupContractSplitVarcArgs& a, hipStream_t s, F f) {
    const unsigned grid = g.first_wg.back();
    mark_sliceable(1, (unsigned)(offsetof(GroupContractSplitVarcArgs, s) + offsetof(GroupContractSplitArgs, g) + offsetof(GroupContractArgs, wg0)), 0);
    int rc;
    if constexpr (is_jit<F>::value)
        rc = launch_jit<T>(g.c, s, "gcontract", "smr::GroupContractSplitVarcArgs", "group_contract_split_varc_body", "", grid, 256, 0, a, MIXED, RB);
    else
        rc = launch_native(nullptr, 0, "k_group_contract_split_varc", [&] { SMR_LAUNCH((k_group_contract_split_varc<T, F, MIXED, RB>), dim3(grid), dim3(256), 0, s, a, f); });
    if (rc || jit_no_launch()) return rc;
    SMR_LAUNCH((k_group_contract_fold<T, MIXED, RB>), dim3(g.contract.fold_first.back()), dim3(256), 0, s, a.s);
    return check_launch("k_group_contract_fold");
}

template <class T, class F, bool MIXED>
static int go_gcsv(const GroupPlan& g, hipStream_t s, F f) {
    const GroupContractPlan& cp = g.contract;
    if (!jit_dry_run() && (!g.d_members || !g.d_first || !cp.d_split || !cp.d_fold_first || !cp.d_partials))
        return set_error(SMR_EINVAL, "split contraction group without its tables or its partials buffer");
    GroupContractSplitVarcArgs a;
    std::memset(&a, 0, sizeof a);
    fill_gc(g, a.s.g);
    a.s.split = (const GroupSplitD*)cp.d_split;
    a.s.fold_first = (const uint32_t*)cp.d_fold_first;
    a.s.partials = cp.d_partials;
    if (int rc = fill_consts(g, a.k)) return rc;
    if (cp.rb == 2) return launch_gcsv<T, F, MIXED, 2>(g, a, s, f);
    if (cp.rb == 1) return launch_gcsv<T, F, MIXED, 1>(g, a, s, f);
    return set_error(SMR_EINVAL, "contraction group: no kernel for this tile");
}

template <>
int launch_group_contract_split_varc_ct<SMR_CT>(const GroupPlan& g, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = g.c;
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go_gcsv<T, decltype(f), true>(g, s, f); });
    if (g.contract.mul2scale) return go_gcsv<T, FMul2Scale<T>, false>(g, s, FMul2Scale<T>{});
    return with_prog<T>(c, [&](auto f) { return go_gcsv<T, decltype(f), false>(g, s, f); });
}
#elif !defined(SMR_GCONTRACT_SPLIT)
template <class T, class F, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_group_contract(GroupContractArgs a, F f) {
    group_contract_body<T, F, MIXED, RB>(a, f);
}

template <class T, class F, bool MIXED, int RB>
static int launch_gc(const Canon& c, const GroupContractArgs& a, unsigned grid, hipStream_t s, F f) {
    // the members are independent and a workgroup serves one member: any contiguous block range can be launched on its own.  `a` is
    // the first kernel parameter of k_group_contract and of the runtime-compiled entry alike, so wg0 has one kernarg offset in both
    mark_sliceable(1, (unsigned)offsetof(GroupContractArgs, wg0), 0);
    if constexpr (is_jit<F>::value)
        return launch_jit<T>(c, s, "gcontract", "smr::GroupContractArgs", "group_contract_body", "", grid, 256, 0, a, MIXED, RB);
    else
        return launch_native(nullptr, 0, "k_group_contract", [&] { SMR_LAUNCH((k_group_contract<T, F, MIXED, RB>), dim3(grid), dim3(256), 0, s, a, f); });
}

template <class T, class F, bool MIXED>
static int go_gc(const GroupPlan& g, hipStream_t s, F f) {
    const Canon& c = g.c;
    GroupContractArgs a;
    std::memset(&a, 0, sizeof a);
    a.members = (const GroupContractMemberD*)g.d_members;
    a.first_wg = (const uint32_t*)g.d_first;
    a.count = (int32_t)g.contract.members.size();
    a.wg0 = 0;
    a.redop = c.redop;
    for (int k = 0; k < 3; ++k) {
        a.dtype[k] = c.dtype[k];
        a.conj[k] = c.conj[k];
    }
    const unsigned grid = g.first_wg.back();
    if (g.contract.rb == 2) return launch_gc<T, F, MIXED, 2>(c, a, grid, s, f);
    if (g.contract.rb == 1) return launch_gc<T, F, MIXED, 1>(c, a, grid, s, f);
    return set_error(SMR_EINVAL, "contraction group: no kernel for this tile");
}

template <>
int launch_group_contract_ct<SMR_CT>(const GroupPlan& g, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = g.c;
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go_gc<T, decltype(f), true>(g, s, f); });
    // natively compiled: the product, as in the single-call kernel; every other f is runtime-compiled or interpreted
    if (c.fkind == FK_MUL2) return go_gc<T, FMul2<T>, false>(g, s, FMul2<T>{});
    return with_prog<T>(c, [&](auto f) { return go_gc<T, decltype(f), false>(g, s, f); });
}
#else  // SMR_GCONTRACT_SPLIT
template <class T, class F, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_group_contract_split(GroupContractSplitArgs a, F f) {
    group_contract_split_body<T, F, MIXED, RB>(a, f);
}

// the two launches of the split form: the members' (tile, slice) workgroups, then the fold (native: it does not call f)
template <class T, class F, bool MIXED, int RB>
static int launch_gcs(const GroupPlan& g, const GroupContractSplitArgs& a, hipStream_t s, F f) {
    const unsigned grid = g.first_wg.back(), fold = g.contract.fold_first.back();
    // a contiguous block range of the main launch is still self-contained (a workgroup writes its own outputs or its own partials):
    // a recorded sequence cuts it under "slices" and puts the fold behind all ranges on the same queue (smr_sched.cpp, step 3c)
    mark_sliceable(1, (unsigned)(offsetof(GroupContractSplitArgs, g) + offsetof(GroupContractArgs, wg0)), 0);
    int rc;
    if constexpr (is_jit<F>::value)
        rc = launch_jit<T>(g.c, s, "gcontract", "smr::GroupContractSplitArgs", "group_contract_split_body", "", grid, 256, 0, a, MIXED, RB);
    else
        rc = launch_native(nullptr, 0, "k_group_contract_split", [&] { SMR_LAUNCH((k_group_contract_split<T, F, MIXED, RB>), dim3(grid), dim3(256), 0, s, a, f); });
    if (rc || jit_no_launch()) return rc;
    SMR_LAUNCH((k_group_contract_fold<T, MIXED, RB>), dim3(fold), dim3(256), 0, s, a);
    return check_launch("k_group_contract_fold");
}

template <class T, class F, bool MIXED>
static int go_gcs(const GroupPlan& g, hipStream_t s, F f) {
    const Canon& c = g.c;
    const GroupContractPlan& cp = g.contract;
    // (a dry run compiles without a device: no tables and no partials yet, and nothing is launched)
    if (!jit_dry_run() && (!g.d_members || !g.d_first || !cp.d_split || !cp.d_fold_first || !cp.d_partials))
        return set_error(SMR_EINVAL, "split contraction group without its tables or its partials buffer");
    GroupContractSplitArgs a;
    std::memset(&a, 0, sizeof a);
    a.g.members = (const GroupContractMemberD*)g.d_members;
    a.g.first_wg = (const uint32_t*)g.d_first;
    a.g.count = (int32_t)cp.members.size();
    a.g.wg0 = 0;
    a.g.redop = c.redop;
    for (int k = 0; k < 3; ++k) {
        a.g.dtype[k] = c.dtype[k];
        a.g.conj[k] = c.conj[k];
    }
    a.split = (const GroupSplitD*)cp.d_split;
    a.fold_first = (const uint32_t*)cp.d_fold_first;
    a.partials = cp.d_partials;
    if (cp.rb == 2) return launch_gcs<T, F, MIXED, 2>(g, a, s, f);
    if (cp.rb == 1) return launch_gcs<T, F, MIXED, 1>(g, a, s, f);
    return set_error(SMR_EINVAL, "contraction group: no kernel for this tile");
}

template <>
int launch_group_contract_split_ct<SMR_CT>(const GroupPlan& g, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = g.c;
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go_gcs<T, decltype(f), true>(g, s, f); });
    if (c.fkind == FK_MUL2) return go_gcs<T, FMul2<T>, false>(g, s, FMul2<T>{});
    return with_prog<T>(c, [&](auto f) { return go_gcs<T, decltype(f), false>(g, s, f); });
}
#endif  // SMR_GCONTRACT_VARC / unsplit / SMR_GCONTRACT_SPLIT
#endif  // !SMR_JIT

}  // namespace smr
