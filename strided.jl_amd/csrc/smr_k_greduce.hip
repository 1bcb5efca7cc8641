// smr_k_greduce.hip -- reduction groups (SMR_GROUP_REDUCE): K independent COMPLETE reductions (one f, one op, one initop code, the
// same operand types; rank, extents, strides, pointers and beta of their own; every destination one element) in ONE launch of
// 256-lane workgroups.
//
// Member i has W_i = min(ceil(total_i / 4096), 64) workgroups (the group planner, smr_plan_group.cpp) and the grid is their sum.  A
// workgroup finds its member by the binary search it shares with the other group kernels (smr_group.h: group_member_of) over the
// prefix sums first_wg[]; its index inside the member and W_i take the places blockIdx.x and gridDim.x have in a single call.  The
// member's descriptor (smr_group.h: GroupReduceMemberD) stays in the device table and is read in place through the constant address
// space: dims[d] and strides[k][d] are indexed by the run-time loop over the dims, all wave-uniform, so each is a scalar load and
// no copy of the descriptor exists that would have to live in scratch.
//
// ACCUMULATION ORDER: that of reduce_all_impl (smr_k_reduce.hip) on a grid of W_i workgroups.  Four accumulators per lane; vector
// body (the planner's `form`, decided like the single call's): a wave reads 4 consecutive 1-KiB rows per iteration; strided body: a
// grid stride of W_i * 256 with 4 elements in flight, the rank-1 shortcut or the decomposition over the dims; then the pairwise tree
// over the four accumulators, the wave butterfly, four wave sums through LDS.  W_i == 1: lane 0 runs the epilogue (initop with the
// member's own beta, redop, store).  W_i > 1: the workgroup publishes its partial write-through into the member's run of W_i slots
// of the group's partials, arrives at the member's counter, and the workgroup that arrives last folds the slots in slot order and
// runs the epilogue -- the protocol of the single call's one-launch fold, through ITS functions (put_partial, arrive_last, fold_all,
// epilogue of smr_k_reduce.hip, which this file includes for its device functions only): they take a RedArgs, so the workgroup fills
// one with what they read -- the operand table, redop, initop, beta, the member's slots, its counter, W -- all of it fields named at
// compile time, which stay in registers; dims and strides, the only fields anything indexes at run time, are never set or read
// there.  Nobody waits or polls.  A member's result is bit-identical to smr_mapreduce on that member alone under option
// "reduce_blocks" = 64 (where that call runs family REDUCE_ALL: include/strided_hip.h).
//
// The launch is NOT sliceable: the fold needs all of a member's workgroups in one launch.
// Compiled once per compute type (-DSMR_CT=n).
#define SMR_REDUCE_DEVICE_ONLY 1
#include "smr_k_reduce.hip"
#include "smr_group.h"

#ifndef SMR_CT
#error "compile with -DSMR_CT=0..3 or 7"
#endif

namespace smr {

struct GroupReduceArgs {
    const GroupReduceMemberD* members;
    const uint32_t* first_wg;  // count + 1 prefix sums
    void* partials;            // compute-class elements: W_i consecutive slots from part_off_i for every member with W_i > 1
    unsigned* counters;        // one arrival counter per such member (zero between launches)
    int32_t count, M, redop, initop;
    int32_t ntl, pad;          // ntl: non-temporal loads in the vector body (Options::nt_load)
    int32_t dtype[MAXM];
    int32_t conj[MAXM];
};

// offsets of box element `i` of member `m` added into off[] (a real loop over the dims, as in smr_k_reduce.hip: decompose)
SMR_DEV void group_reduce_decompose(GroupReduceMemberC& m, int M, i64 i, i64* off) {
    i64 rem = i;
    const int N = m.N;
#pragma nounroll
    for (int d = 0; d < N; ++d) {
        i64 c;
        if (d == N - 1) {
            c = rem;
        } else {
            const i64 q = rem / m.dims[d];
            c = rem - q * m.dims[d];
            rem = q;
        }
#pragma unroll
        for (int k = 0; k < MAXM; ++k)
            if (k < M) off[k] += c * m.strides[k][d];
    }
}

template <class T, class F, bool MIXED, int OPC>
SMR_DEV void group_reduce_impl(const GroupReduceArgs& a, F f) {
    const int redop = (OPC >= 0) ? OPC : a.redop;  // compile-time for the sum: no op switch inside the loops
    __shared__ T wsum[4];
    // the member of this workgroup, its index inside the member and the member's workgroups
    const uint32_t b = blockIdx.x;
    GroupWordC* const first_wg = (GroupWordC*)a.first_wg;
    const int lo = group_member_of(first_wg, a.count, b);
    GroupReduceMemberC& m = ((GroupReduceMemberC*)a.members)[lo];
    const uint32_t wg = b - first_wg[lo], W = first_wg[lo + 1] - first_wg[lo];
    OpTab t;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
        t.base[k] = m.base[k];
        t.dtype[k] = a.dtype[k];
        t.conj[k] = a.conj[k];
    }
    const int nin = (F::NIN >= 0) ? F::NIN : a.M - 1;
    constexpr int ACC = 4;
    T acc[ACC];
#pragma unroll
    for (int j = 0; j < ACC; ++j) acc[j] = neutral<T>(redop);
    const i64 total = m.total;
    const i64 nthreads = (i64)W * 256;
    const i64 t0 = (i64)wg * 256 + threadIdx.x;
    constexpr int V = (MIXED || sizeof(T) >= 16) ? 1 : (int)(16 / sizeof(T));
    bool vector = false;
    if constexpr (V > 1) vector = m.form == GROUP_FORM_REDUCE_VECTOR;  // (wave-uniform: the member's)
    if constexpr (V > 1) {
        if (vector) {
            // rank 1, unit-stride (or broadcast) inputs: 16-byte loads, ACC vectors in flight; a wave reads ACC consecutive 1-KiB rows
            // (one contiguous 4-KiB piece) per iteration
            typedef RVec<T, V> VT;
            const i64 nvec = total / V;
            const i64 lane_ = threadIdx.x & 63;
            const i64 nrows = (nvec + 63) >> 6;
            auto sweep = [&](auto NTL) {
                for (i64 row = (t0 >> 6) * ACC; row < nrows; row += (nthreads >> 6) * ACC) {
                    const i64 i = row * 64 + lane_;
                    VT x[ACC][MAXIN];
#pragma unroll
                    for (int j = 0; j < ACC; ++j) {
                        const i64 ii = i + j * 64;
                        if (ii < nvec) {
#pragma unroll
                            for (int k = 0; k < MAXIN; ++k)
                                if (k < nin) {
                                    if (m.strides[k + 1][0] == 0) {
                                        const T s = load_op<T, false>(t, k + 1, 0);
#pragma unroll
                                        for (int e = 0; e < V; ++e) x[j][k].v[e] = s;
                                    } else {
                                        x[j][k] = load_vec_ct<decltype(NTL)::value, VT>((const T*)t.base[k + 1] + ii * V);
                                        if constexpr (tr<T>::cx) {
                                            if (t.conj[k + 1]) {
#pragma unroll
                                                for (int e = 0; e < V; ++e) x[j][k].v[e] = cj(x[j][k].v[e]);
                                            }
                                        }
                                    }
                                }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < ACC; ++j) {
                        const i64 ii = i + j * 64;
                        if (ii < nvec) {
#pragma unroll
                            for (int e = 0; e < V; ++e) {
                                T in[MAXIN];
#pragma unroll
                                for (int k = 0; k < MAXIN; ++k) {
                                    in[k] = T{};
                                    if (k < nin) in[k] = x[j][k].v[e];
                                }
                                acc[j] = red_apply<T>(redop, acc[j], f(in));
                            }
                        }
                    }
                }
            };
            if (a.ntl) {
                nt_block_guard();
                sweep(BoolC<true>{});
                nt_block_guard();
            } else {
                sweep(BoolC<false>{});
            }
        }
    }
    if (!vector) {
        const bool linear = m.N == 1;
        for (i64 i = t0; i < total; i += nthreads * ACC) {
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const i64 ii = i + j * nthreads;
                if (ii < total) {
                    i64 off[MAXM];
#pragma unroll
                    for (int k = 0; k < MAXM; ++k) off[k] = 0;
                    if (linear) {
#pragma unroll
                        for (int k = 1; k < MAXM; ++k)
                            if (k < a.M) off[k] = ii * m.strides[k][0];
                    } else {
                        group_reduce_decompose(m, a.M, ii, off);
                    }
                    T in[MAXIN];
#pragma unroll
                    for (int k = 0; k < MAXIN; ++k) {
                        in[k] = T{};
                        if (k < nin) in[k] = load_op<T, MIXED>(t, k + 1, off[k + 1]);
                    }
                    acc[j] = red_apply<T>(redop, acc[j], f(in));
                }
            }
        }
    }
#pragma unroll
    for (int w = ACC / 2; w > 0; w >>= 1) {  // pairwise tree over the per-lane accumulators
#pragma unroll
        for (int j = 0; j < w; ++j) acc[j] = red_apply<T>(redop, acc[j], acc[j + w]);
    }
    T v = acc[0];
    v = wave_reduce(v, redop, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wsum[wave] = v;
    __syncthreads();
    // what the single call's epilogue and fold read of their arguments (every field named at compile time: registers)
    RedArgs r;
    r.ops = t;
    r.redop = a.redop;
    r.initop = a.initop;
    r.beta[0] = m.beta[0];
    r.beta[1] = m.beta[1];
    r.partials = (T*)a.partials + m.part_off;  // (only touched when W > 1: the member then owns slots [0, W) from part_off)
    r.counters = a.counters + m.counter;       // ... and this counter
    r.nparts = (int32_t)W;
    r.single = 1;
    if (threadIdx.x == 0) {
        v = red_apply<T>(redop, red_apply<T>(redop, wsum[0], wsum[1]), red_apply<T>(redop, wsum[2], wsum[3]));
        if (W == 1)
            epilogue<T, MIXED>(r, 0, v);
        else
            put_partial<T>(r, wg, v);
    }
    if (W > 1) {  // (workgroup-uniform)
        if (!arrive_last(r, 0, (int)W)) return;
        fold_all<T, MIXED>(r, redop, wsum);
    }
}

template <class T, class F, bool MIXED>
SMR_DEV void group_reduce_body(const GroupReduceArgs a, F f) {
    if (a.redop == SMR_RED_ADD)
        group_reduce_impl<T, F, MIXED, SMR_RED_ADD>(a, f);
    else
        group_reduce_impl<T, F, MIXED, -1>(a, f);
}

#ifndef SMR_JIT
template <class T, class F, bool MIXED>
__global__ void __launch_bounds__(256) k_group_reduce(GroupReduceArgs a, F f) {
    group_reduce_body<T, F, MIXED>(a, f);
}

template <class T, class F, bool MIXED>
static int go_gr(const GroupPlan& g, hipStream_t s, F f) {
    const Canon& c = g.c;
    const GroupReducePlan& rp = g.reduce;
    // (a dry run compiles without a device: no tables yet, and nothing is launched)
    if (!jit_dry_run() && (!g.d_members || !g.d_first || (rp.npartials && (!rp.d_partials || !rp.d_counters))))
        return set_error(SMR_EINVAL, "reduction group without its tables, its partials or its counters");
    GroupReduceArgs a;
    std::memset(&a, 0, sizeof a);
    a.members = (const GroupReduceMemberD*)g.d_members;
    a.first_wg = (const uint32_t*)g.d_first;
    a.partials = rp.d_partials;
    a.counters = (unsigned*)rp.d_counters;
    a.count = (int32_t)rp.members.size();
    a.M = c.M;
    a.redop = c.redop;
    a.initop = c.initop;
    // as a single call decides it (smr_k_reduce.hip: fill_args), on the group's largest member; it does not change values
    a.ntl = (options().nt_load > 0 || (options().nt_load < 0 && rp.max_in_bytes < 2147483648.0L)) ? 1 : 0;
    for (int k = 0; k < MAXM; ++k) {
        a.dtype[k] = k < c.M ? c.dtype[k] : 0;
        a.conj[k] = k < c.M ? c.conj[k] : 0;
    }
    const unsigned grid = g.first_wg.back();
    // no mark_sliceable: a block range of this launch would leave a member's last workgroup waiting for arrivals that never come
    if constexpr (is_jit<F>::value)
        return launch_jit<T>(c, s, "greduce", "smr::GroupReduceArgs", "group_reduce_body", "", grid, 256, 0, a, MIXED);
    else
        return launch_native(nullptr, 0, "k_group_reduce", [&] { SMR_LAUNCH((k_group_reduce<T, F, MIXED>), dim3(grid), dim3(256), 0, s, a, f); });
}

template <>
int launch_group_reduce_ct<SMR_CT>(const GroupPlan& g, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = g.c;
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go_gr<T, decltype(f), true>(g, s, f); });
    // the functors a single complete reduction runs natively (smr_k_reduce.hip): the same code computes f in both
    return with_functor<T>(c, GROUP_REDUCE_FMASK, [&](auto f) { return go_gr<T, decltype(f), false>(g, s, f); });
}
#endif  // !SMR_JIT

}  // namespace smr
