// smr_k_greduce_part.hip -- partial reduction groups (SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART): K independent reductions that may
// KEEP dims (one f, one op, one initop code, the same operand types; rank, extents, strides, pointers, beta and the kept dims of
// their own) in ONE launch of 256-lane workgroups.
//
// Member i runs the general form of a single partial reduction (smr_k_reduce.hip: reduce_part_impl) with its reduced range in one
// piece: TR_i = 1 << trlog consecutive lanes cooperate on one destination element, a workgroup owns 256 / TR_i consecutive
// destination elements in canonical order, W_i = ceil(nout_i / (256 / TR_i)) (the group planner, smr_plan_group.cpp) and the grid is
// the sum.  A workgroup finds its member by the binary search it shares with the other group kernels (smr_group.h: group_member_of)
// over the prefix sums first_wg[] with its index in the group, blockIdx.x + wg0 -- a launch may be one contiguous block range of the
// group.  The member's descriptor (smr_group.h: GroupReducePartMemberD) stays in the device table and is read in place through the
// constant address space: dims[d] and strides[k][d] are indexed by run-time loops over the dims, all wave-uniform, so each is a
// scalar load and no copy of the descriptor exists that would have to live in scratch.
//
// ACCUMULATION ORDER: that of reduce_part_impl with nsplit = 1.  Lane rl = tid & (TR - 1) of output o = (b - first_wg[i]) * (256 / TR)
// + (tid >> trlog) accumulates r = rl, rl + TR, rl + 2 TR, ... serially into one accumulator that starts at the op's neutral; TR <= 64:
// wave_reduce over TR lanes; TR > 64: wave_reduce over 64 lanes, then lane rl = 0 adds the waves' values from LDS in ascending order.
// Lane rl = 0 runs the single call's epilogue (initop with the member's own beta, redop, store, conversions) -- epilogue, wave_reduce,
// neutral and red_apply are smr_k_reduce.hip's own, which this file includes for its device functions only.  Lanes with o >= nout_i
// stay dead but take part in the barrier.  A member's result is bit-identical to smr_mapreduce on that member alone under option
// "reduce_part_kind" = 0 wherever that call reads "form=general lanes_per_out=TR_i split=1" (include/strided_hip.h).
//
// Addressing: a member has at most 2^31 - 1 box elements, so output and reduced indices are decomposed in 32 bits -- the output index
// once per lane, the reduced index per element: none for at most one reduced dim (the index times the stride), one division for two
// (extent and strides hoisted out of the loop), the loop over the dims for more.
//
// No workgroup depends on another: the launch is sliceable on wg0.  Compiled once per compute type (-DSMR_CT=n).
#define SMR_REDUCE_DEVICE_ONLY 1
#include "smr_k_reduce.hip"
#include "smr_group.h"

#ifndef SMR_CT
#error "compile with -DSMR_CT=0..3 or 7"
#endif

namespace smr {

struct GroupReducePartArgs {
    const GroupReducePartMemberD* members;
    const uint32_t* first_wg;  // count + 1 prefix sums
    int32_t count, M, redop, initop;
    uint32_t wg0;              // first workgroup of this launch within the group (0: the launch is the whole group)
    int32_t pad;
    int32_t dtype[MAXM];
    int32_t conj[MAXM];
};

// offsets of index `i` decomposed over dims [d0, d1) of member `m` added into off[] (a real loop over the dims, as in
// smr_k_reduce.hip: decompose; 32-bit: i and every dim of a member are below 2^31)
SMR_DEV void group_part_decompose(GroupReducePartMemberC& m, int M, uint32_t i, int d0, int d1, i64* off) {
    uint32_t rem = i;
#pragma nounroll
    for (int d = d0; d < d1; ++d) {
        uint32_t c;
        if (d == d1 - 1) {
            c = rem;
        } else {
            const uint32_t n = (uint32_t)m.dims[d];
            const uint32_t q = rem / n;
            c = rem - q * n;
            rem = q;
        }
#pragma unroll
        for (int k = 0; k < MAXM; ++k)
            if (k < M) off[k] += (i64)c * m.strides[k][d];
    }
}

template <class T, class F, bool MIXED, int OPC>
SMR_DEV void group_reduce_part_impl(const GroupReducePartArgs& a, F f) {
    const int redop = (OPC >= 0) ? OPC : a.redop;  // compile-time for the sum: no op switch inside the loops
    __shared__ T xbuf[256];
    // the member of this workgroup and the workgroup's index inside the member
    const uint32_t b = blockIdx.x + a.wg0;
    GroupWordC* const first_wg = (GroupWordC*)a.first_wg;
    const int lo = group_member_of(first_wg, a.count, b);
    GroupReducePartMemberC& m = ((GroupReducePartMemberC*)a.members)[lo];
    const uint32_t og = b - first_wg[lo];
    OpTab t;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
        t.base[k] = m.base[k];
        t.dtype[k] = a.dtype[k];
        t.conj[k] = a.conj[k];
    }
    const int nin = (F::NIN >= 0) ? F::NIN : a.M - 1;
    const int trlog = m.trlog, tr_ = 1 << trlog;
    const int N = m.N, NK = m.NK;
    const uint32_t nout = (uint32_t)m.nout, nred = (uint32_t)m.nred;
    const uint32_t rl = threadIdx.x & (uint32_t)(tr_ - 1);
    const uint32_t ol = threadIdx.x >> trlog;
    // (og * (256 / TR) < nout + 256 / TR: no overflow)
    const uint32_t o = og * (uint32_t)(256 >> trlog) + ol;
    const bool live = o < nout;
    i64 ooff[MAXM];
#pragma unroll
    for (int k = 0; k < MAXM; ++k) ooff[k] = 0;
    if (live) group_part_decompose(m, a.M, o, 0, NK, ooff);
    T acc = neutral<T>(redop);
    if (live) {
        const int nrd = N - NK;  // reduced dims (wave-uniform)
        if (nrd <= 2) {
            // at most two reduced dims: the inner one's extent and both strides per operand in registers
            const uint32_t L0 = nrd == 2 ? (uint32_t)m.dims[NK] : 0x7fffffffu;
            i64 s0[MAXM], s1[MAXM];
#pragma unroll
            for (int k = 0; k < MAXM; ++k) {
                s0[k] = (k < a.M && nrd >= 1) ? m.strides[k][NK] : 0;
                s1[k] = (k < a.M && nrd == 2) ? m.strides[k][NK + 1] : 0;
            }
            for (uint32_t r = rl; r < nred; r += (uint32_t)tr_) {
                uint32_t c0 = r, c1 = 0;
                if (nrd == 2) {
                    c1 = r / L0;
                    c0 = r - c1 * L0;
                }
                T in[MAXIN];
#pragma unroll
                for (int k = 0; k < MAXIN; ++k) {
                    in[k] = T{};
                    if (k < nin) in[k] = load_op<T, MIXED>(t, k + 1, ooff[k + 1] + (i64)c0 * s0[k + 1] + (i64)c1 * s1[k + 1]);
                }
                acc = red_apply<T>(redop, acc, f(in));
            }
        } else {
            for (uint32_t r = rl; r < nred; r += (uint32_t)tr_) {
                i64 off[MAXM];
#pragma unroll
                for (int k = 0; k < MAXM; ++k) off[k] = ooff[k];
                group_part_decompose(m, a.M, r, NK, N, off);
                T in[MAXIN];
#pragma unroll
                for (int k = 0; k < MAXIN; ++k) {
                    in[k] = T{};
                    if (k < nin) in[k] = load_op<T, MIXED>(t, k + 1, off[k + 1]);
                }
                acc = red_apply<T>(redop, acc, f(in));
            }
        }
    }
    if (tr_ > 1) {  // (workgroup-uniform: the member's)
        acc = wave_reduce(acc, redop, tr_ < 64 ? tr_ : 64);
        if (tr_ > 64) {  // lanes of one output span several waves
            xbuf[threadIdx.x] = acc;
            __syncthreads();
            if (rl == 0) {
                for (int j = 64; j < tr_; j += 64) acc = red_apply<T>(redop, acc, xbuf[threadIdx.x + j]);
            }
        }
    }
    if (live && rl == 0) {
        // what the single call's epilogue reads of its arguments (every field named at compile time: registers)
        RedArgs r;
        r.ops = t;
        r.redop = a.redop;
        r.initop = a.initop;
        r.beta[0] = m.beta[0];
        r.beta[1] = m.beta[1];
        epilogue<T, MIXED>(r, ooff[0], acc);
    }
}

template <class T, class F, bool MIXED>
SMR_DEV void group_reduce_part_body(const GroupReducePartArgs a, F f) {
    if (a.redop == SMR_RED_ADD)
        group_reduce_part_impl<T, F, MIXED, SMR_RED_ADD>(a, f);
    else
        group_reduce_part_impl<T, F, MIXED, -1>(a, f);
}

#ifndef SMR_JIT
template <class T, class F, bool MIXED>
__global__ void __launch_bounds__(256) k_group_reduce_part(GroupReducePartArgs a, F f) {
    group_reduce_part_body<T, F, MIXED>(a, f);
}

template <class T, class F, bool MIXED>
static int go_grp(const GroupPlan& g, hipStream_t s, F f) {
    const Canon& c = g.c;
    // (a dry run compiles without a device: no tables yet, and nothing is launched)
    if (!jit_dry_run() && (!g.d_members || !g.d_first)) return set_error(SMR_EINVAL, "partial reduction group without its tables");
    GroupReducePartArgs a;
    std::memset(&a, 0, sizeof a);
    a.members = (const GroupReducePartMemberD*)g.d_members;
    a.first_wg = (const uint32_t*)g.d_first;
    a.count = (int32_t)g.reduce_part.members.size();
    a.M = c.M;
    a.redop = c.redop;
    a.initop = c.initop;
    a.wg0 = 0;
    for (int k = 0; k < MAXM; ++k) {
        a.dtype[k] = k < c.M ? c.dtype[k] : 0;
        a.conj[k] = k < c.M ? c.conj[k] : 0;
    }
    const unsigned grid = g.first_wg.back();
    // the members are independent and a workgroup serves destination elements of its own: any contiguous block range can be launched
    // on its own.  `a` is the first kernel parameter of k_group_reduce_part and of the runtime-compiled entry alike, so wg0 has one
    // kernarg offset in both
    mark_sliceable(1, (unsigned)offsetof(GroupReducePartArgs, wg0), 0);
    if constexpr (is_jit<F>::value)
        return launch_jit<T>(c, s, "greduce_part", "smr::GroupReducePartArgs", "group_reduce_part_body", "", grid, 256, 0, a, MIXED);
    else
        return launch_native(nullptr, 0, "k_group_reduce_part", [&] { SMR_LAUNCH((k_group_reduce_part<T, F, MIXED>), dim3(grid), dim3(256), 0, s, a, f); });
}

template <>
int launch_group_reduce_part_ct<SMR_CT>(const GroupPlan& g, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = g.c;
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go_grp<T, decltype(f), true>(g, s, f); });
    // the functors a reduction group runs natively: the same code computes f in a single call
    return with_functor<T>(c, GROUP_REDUCE_FMASK, [&](auto f) { return go_grp<T, decltype(f), false>(g, s, f); });
}
#endif  // !SMR_JIT

}  // namespace smr
