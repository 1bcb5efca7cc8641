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
// Compiled once per compute type (-DSMR_CT=n).
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

#ifndef SMR_JIT
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
#endif  // !SMR_JIT

}  // namespace smr
