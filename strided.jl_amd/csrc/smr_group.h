// smr_group.h -- grouped launches (smr_group_*): K independent small maps, each with its own rank, dims, strides, pointers and
// offsets, run as ONE kernel launch (smr_k_group.hip) -- or K independent small contractions (smr_k_gcontract.hip).  Shared by the
// group planner (smr_plan_group.cpp), the C ABI and launch path (smr_group.cpp) and the kernels' translation units.  The top part
// -- the device tables and the member search both kernels run -- is also compiled by hiprtc (SMR_JIT).
#pragma once

#include "smr_device.h"

namespace smr {

constexpr int GROUP_U = 4;                   // linear form: elements per lane
constexpr int GROUP_CHUNK = 256 * GROUP_U;   // ... canonical indices per workgroup
constexpr int GROUP_TILE = 32;               // transposing form: tile edge (staged through GROUP_TILE x (GROUP_TILE + 1) elements of LDS)
constexpr int GROUP_TMIN = 16;               // transposing form only when both tiled dims are at least this long (a 32 x 32 tile is then >= 1/4 full)

// One member of a group as the kernel reads it (device table, one entry per member).  Everything in it is wave-uniform.
struct GroupMemberD {
    void* base[MAXM];            // operand addresses, element offsets folded in
    i64 strides[MAXM][MAXN];     // canonical strides (elements)
    i64 qstride[MAXM];           // transposing form: every operand's stride along dim q
    void* tbase;                 // transposing form: the staged input's address ...
    i64 tsp, tsq;                // ... and its strides along dim 0 and dim q (tsq = +-1)
    uint32_t dims[MAXN];         // canonical dims (a member has at most 2^31 - 1 box elements)
    uint32_t step[MAXN];         // linear form: the mixed-radix digits of 256 over `dims` (a lane's step between its elements)
    uint32_t total;              // box elements
    int32_t N;                   // canonical rank
    int32_t form;                // 0 linear, 1 transposing
    int32_t kt, q;               // transposing form: staged input (1..M-1), canonical dim along which it is unit-stride
    int32_t tdtype, tconj;       // ... its dtype / conj flag
    uint32_t ntp, ntq;           // ... tiles along dim 0 and along dim q
};

// One member of a CONTRACTION group (smr_k_gcontract.hip): the geometry a single call of FAM_CONTRACT carries in ContractArgs
// (smr_contract.h: the field names are those the shared tile body reads), and the member's operand addresses.  Everything in it
// is wave-uniform.  beta (the initop's argument) is the member's own; redop and the initop code are those of member 0.
struct GroupContractMemberD {
    void* base[3];               // destination, input 1, input 2: element offsets folded in
    int32_t N, NK, redop, initop, di, dj, vec, nrd;
    int32_t rdim[MAXN];
    int32_t mode[3];
    i64 dims[MAXN];
    i64 strides[3][MAXN];
    double beta[2];
    i64 nti, ntj, K, Q, nkc;
};

// The split form of a contraction group (option "group_contract_split"; smr_k_gcontract.hip): how member i's chunk walk is cut, one
// entry per member in a table of its own next to the member table.  S == 1: the member is not split and runs the unsplit body.
struct GroupSplitD {
    i64 part_off;                // first element of the member's partials in the group's buffer (compute-class elements)
    i64 cps;                     // chunks per slice
    uint32_t S;                  // slices
    uint32_t tiles;              // output tiles: the member's workgroups in the main launch are tiles * S, the slice the slow digit
};

// One member of a REDUCTION group (SMR_GROUP_REDUCE; smr_k_greduce.hip): a complete reduction as a single call of FAM_REDUCE_ALL
// carries it in its arguments.  Everything in it is wave-uniform.  beta (the initop's argument) is the member's own; redop and the
// initop code are those of member 0.  The member's workgroups W are first_wg[i + 1] - first_wg[i].
struct GroupReduceMemberD {
    void* base[MAXM];            // operand addresses, element offsets folded in ([0]: the one destination element)
    i64 strides[MAXM][MAXN];     // canonical strides (elements)
    i64 dims[MAXN];              // canonical dims
    i64 total;                   // box elements (at most 2^31 - 1)
    i64 part_off;                // W > 1: the member's first slot in the group's partials (compute-class elements) ...
    double beta[2];
    int32_t counter;             // ... and its arrival counter
    int32_t N;                   // canonical rank
    int32_t form;                // GROUP_FORM_REDUCE_STRIDED or GROUP_FORM_REDUCE_VECTOR
    int32_t pad;
};

// One member of a PARTIAL reduction group (SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART; smr_k_greduce_part.hip): a reduction that keeps
// dims, as a single call of FAM_REDUCE_PART's general form carries it in its arguments with the reduced range in one piece.  Dims
// [0, NK) are kept, [NK, N) reduced (NK == 0: one destination element; NK == N: no reduced dim, an accumulating map).  1 << trlog
// consecutive lanes cooperate on one destination element and a workgroup owns 256 >> trlog consecutive destination elements in
// canonical order, so the member's workgroups are ceil(nout / (256 >> trlog)).  Everything in it is wave-uniform; beta is the member's own.
struct GroupReducePartMemberD {
    void* base[MAXM];            // operand addresses, element offsets folded in
    i64 strides[MAXM][MAXN];     // canonical strides (elements; the destination's are 0 along the reduced dims)
    i64 dims[MAXN];              // canonical dims
    i64 nout, nred;              // destination elements, reduced elements per destination element (nout * nred <= 2^31 - 1)
    double beta[2];
    int32_t N, NK;               // canonical rank, kept dims
    int32_t trlog;               // log2 of the lanes per destination element (0 .. 8)
    int32_t pad;
};

// The tables are read-only for the whole launch and every index into them is wave-uniform: read through the constant address
// space they are fetched by scalar loads into scalar registers, not once per lane.
typedef const GroupMemberD __attribute__((address_space(4))) GroupMemberC;
typedef const GroupContractMemberD __attribute__((address_space(4))) GroupContractMemberC;
typedef const GroupSplitD __attribute__((address_space(4))) GroupSplitC;
typedef const GroupReduceMemberD __attribute__((address_space(4))) GroupReduceMemberC;
typedef const GroupReducePartMemberD __attribute__((address_space(4))) GroupReducePartMemberC;
typedef const uint32_t __attribute__((address_space(4))) GroupWordC;
typedef const double __attribute__((address_space(4))) GroupConstC;

// The member of workgroup `b` of the group: the last one whose first workgroup is <= b (first_wg[]: count + 1 prefix sums of the
// members' workgroups; every member has at least one in the main launch.  The fold launch of a split contraction group searches
// its own prefix sums, in which unsplit members have none: equal neighbouring entries.  The loop keeps first_wg[lo] <= b <
// first_wg[hi], so it ends on the one member whose range is not empty and holds b).
SMR_DEV int group_member_of(GroupWordC* first_wg, int count, uint32_t b) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first_wg[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// what smr_group_layout reports per member: the body a map member runs (GroupMemberD::form), that it is a contraction, or the body
// a member of a reduction group runs (GroupReduceMemberD::form), or that it is a member of a partial reduction group
enum GroupForm { GROUP_FORM_LINEAR = 0, GROUP_FORM_TRANSPOSING = 1, GROUP_FORM_CONTRACT = 2, GROUP_FORM_REDUCE_STRIDED = 3, GROUP_FORM_REDUCE_VECTOR = 4, GROUP_FORM_REDUCE_PART = 5 };

#ifndef SMR_JIT
// every recognised functor has a natively compiled group kernel (a single call's functor code); any other f is a program, as in GENERIC
constexpr unsigned GROUP_FMASK = 0xffffffffu;

// a reduction group runs natively the functors a single complete reduction does (smr_k_reduce.hip), any other f as a program
constexpr unsigned GROUP_REDUCE_FMASK = (1u << FK_IDENT) | (1u << FK_ABS2) | (1u << FK_MUL2);

// the kind is member 0's: a reduction opens a contraction group (every member an outer-product reduction on FAM_CONTRACT's tile body)
// -- unless SMR_GROUP_REDUCE asks for a reduction group (every member a complete reduction; with SMR_GROUP_REDUCE_PART every member
// a reduction that may keep dims)
enum GroupKind { GROUP_MAP, GROUP_CONTRACT, GROUP_REDUCE, GROUP_REDUCE_PART };

struct GroupMapPlan {  // GROUP_MAP only
    std::vector<GroupMemberD> members;
    int nlinear = 0, ntrans = 0;
    // per-member scalars (SMR_GROUP_MEMBER_SCALARS and constants that do differ): row i holds member i's W doubles, Canon::fc
    // (W = 4) for a recognised functor, ProgD::consts (W = 2 * nconst) for a program
    bool varc = false;
    int W = 0;
    std::vector<double> consts;
    mutable void* d_consts = nullptr;  // device copy of `consts`
};
struct GroupContractPlan {  // GROUP_CONTRACT only
    std::vector<GroupContractMemberD> members;
    int rb = 1;  // one tile size (16 * rb) for the whole launch
    // the split form (option "group_contract_split"): empty / 0 unless at least one member is split
    std::vector<GroupSplitD> split;        // one entry per member
    std::vector<uint32_t> fold_first;      // count + 1 prefix sums of the members' workgroups in the fold launch (rb^2 per tile of a split member)
    int nsplit = 0, max_s = 0;             // members with S >= 2, the largest S
    size_t scratch_bytes = 0;              // the group's partials: sum over split members of tiles * S * tile^2 * element size
    mutable void* d_split = nullptr;       // device copies, and the partials buffer (one per group)
    mutable void* d_fold_first = nullptr;
    mutable void* d_partials = nullptr;
    // per-member constants of f (SMR_GROUP_CONTRACT_SCALARS and constants that do differ), as in GroupMapPlan: row i holds member
    // i's W doubles, ProgD::consts (W = 2 * nconst) -- for the recognised product x * y * alpha (`mul2scale`) the pair (re, im) of alpha
    bool varc = false;
    bool mul2scale = false;                // varc, unmixed and f is the mul! form: the natively compiled FMul2Scale
    int W = 0;
    std::vector<double> consts;
    mutable void* d_consts = nullptr;      // device copy of `consts`
};

struct GroupReducePlan {  // GROUP_REDUCE only
    std::vector<GroupReduceMemberD> members;
    int nvec = 0, nstrided = 0;            // members on the vector / the strided body
    int npartials = 0;                     // members with more than one workgroup: each has a run of slots and a counter
    i64 slots = 0;                         // the group's partials, in compute-class elements (sum of W_i over those members)
    size_t scratch_bytes = 0;              // ... in bytes, the counters included
    long double max_in_bytes = 0;          // the largest member's first input (what the non-temporal-load rule looks at)
    mutable void* d_partials = nullptr;    // one buffer per group, and the counters (zeroed when allocated; a run leaves them zero)
    mutable void* d_counters = nullptr;
};

struct GroupReducePartPlan {  // GROUP_REDUCE_PART only: no partials, no counters, no scratch -- a member's reduced range is never split
    std::vector<GroupReducePartMemberD> members;
    int lanes[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // members per lanes-per-output 1 << j
};

// A planned group.  `c` is the canonical problem of member 0: its compute class, flags, dtypes and f-program are those of every member
// (the values of the program's constants too, unless `map.varc` / `contract.varc`).
struct GroupPlan {
    Canon c;
    GroupKind kind = GROUP_MAP;
    GroupMapPlan map;
    GroupContractPlan contract;
    GroupReducePlan reduce;
    GroupReducePartPlan reduce_part;
    std::vector<uint32_t> first_wg;   // count + 1 prefix sums of the members' workgroups
    std::vector<int> rank;            // canonical rank per member (smr_group_layout)
    bool jit = false;                 // f runs as a runtime-compiled functor
    i64 algbytes = 0;
    std::string desc;
    // what one execution reads (every input of every member) and writes (every destination): operand_span() ranges, sorted, with
    // overlapping and adjacent ones merged -- the footprint of a group recorded in a sequence (smr_seq_add_group)
    std::vector<std::pair<uintptr_t, uintptr_t>> rd, wr;
    // device copies of the member table and `first_wg` (and map.d_consts), uploaded by prepare / the first execution
    mutable std::mutex build_mu;
    mutable void* d_members = nullptr;
    mutable void* d_first = nullptr;

    // a host table as bytes; the member table of the group's kind
    template <class E> static std::pair<const void*, size_t> bytes_of(const std::vector<E>& v) { return {v.data(), v.size() * sizeof(E)}; }
    std::pair<const void*, size_t> member_table() const {
        if (kind == GROUP_REDUCE_PART) return bytes_of(reduce_part.members);
        return kind == GROUP_CONTRACT ? bytes_of(contract.members) : (kind == GROUP_REDUCE ? bytes_of(reduce.members) : bytes_of(map.members));
    }
    int form(size_t i) const {
        if (kind == GROUP_REDUCE_PART) return GROUP_FORM_REDUCE_PART;
        return kind == GROUP_CONTRACT ? GROUP_FORM_CONTRACT : (kind == GROUP_REDUCE ? reduce.members[i].form : map.members[i].form);
    }
};

// smr_plan_group.cpp: plans members[0..count) (count >= 1, known flags) into a fresh `g`.  Host arithmetic only, no HIP runtime call
int plan_group(const smr_problem* members, int count, uint32_t flags, GroupPlan& g);

template <int CT> int launch_group_ct(const GroupPlan&, hipStream_t);           // smr_k_group.hip
template <int CT> int launch_group_contract_ct(const GroupPlan&, hipStream_t);  // smr_k_gcontract.hip
template <int CT> int launch_group_contract_split_ct(const GroupPlan&, hipStream_t);  // smr_k_gcontract.hip compiled with -DSMR_GCONTRACT_SPLIT
template <int CT> int launch_group_contract_varc_ct(const GroupPlan&, hipStream_t);        // ... with -DSMR_GCONTRACT_VARC (contract.varc)
template <int CT> int launch_group_contract_split_varc_ct(const GroupPlan&, hipStream_t);  // ... (contract.varc and a split member)
template <int CT> int launch_group_reduce_ct(const GroupPlan&, hipStream_t);    // smr_k_greduce.hip
template <int CT> int launch_group_reduce_part_ct(const GroupPlan&, hipStream_t);  // smr_k_greduce_part.hip

int ensure_device();         // smr_api.cpp
i64& group_max_bytes();      // option "group_max_bytes" (smr_group.cpp)
i64& group_contract_tile();  // option "group_contract_tile": 0 = the planner's rule, 16 / 32 force the tile of contraction groups
i64& group_contract_split(); // option "group_contract_split": 0 = never, 1 = the group rule, N >= 2 force N slices per member (smr_plan_group.cpp)

// Bounding byte range [lo, hi) of operand k of a canonical problem: what footprint() (smr_api.cpp) and the group planner compare.
inline void operand_span(const Canon& c, int k, const void* base, uintptr_t& lo_out, uintptr_t& hi_out) {
    i64 lo = c.offsets[k], hi = c.offsets[k];
    for (int d = 0; d < c.N; ++d) {
        const i64 ext = (c.dims[d] - 1) * c.strides[k][d];
        (ext < 0 ? lo : hi) += ext;
    }
    lo_out = (uintptr_t)base + (uintptr_t)(lo * (i64)c.esize[k]);
    hi_out = (uintptr_t)base + (uintptr_t)((hi + 1) * (i64)c.esize[k]);
}
#endif  // !SMR_JIT

}  // namespace smr
