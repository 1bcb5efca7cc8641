// smr_k_group.hip -- grouped launches: K small independent maps (one functor f, the same operand types; rank, dims, strides,
// pointers and offsets of their own) in ONE launch of 256-lane workgroups.  The grid is the sum of the members' workgroup counts:
// a workgroup finds its member by a binary search of the prefix sums first_wg[] (smr_group.h: group_member_of, shared with the
// contraction groups' kernel) with its index in the group (blockIdx.x + wg0: a launch may be one contiguous block range of the group,
// which is how a recorded sequence spreads one group over several hardware queues) and reads the member's descriptor (smr_group.h:
// GroupMemberD).  Both steps use wave-uniform indices only, so they stay in scalar registers.  Two bodies, chosen per member by the
// group planner (smr_plan_group.cpp):
//   linear       destination-fastest enumeration, GROUP_CHUNK consecutive canonical indices per workgroup, GROUP_U per lane
//                (256 apart: a wave's accesses are consecutive).  The index is decomposed once per lane and then stepped by the
//                mixed-radix digits of 256.  Correct for any strides; coalesced when the inputs are unit-stride or broadcast
//                along the destination's fastest dim.
//   transposing  exactly one input is unit-stride along another dim q: the (dim 0 x dim q) plane is cut into 32 x 32 tiles that
//                pass through LDS (rows padded to 33 elements: the column reads of 4-, 8- and 16-byte elements are free of bank
//                conflicts), ragged edges guarded, outer dims decomposed from the tile index, other inputs read directly.
// Loads and stores go through load_op / store_op: conj, mixed dtypes and bit copies behave as in GENERIC.
// Per-member scalars (VARC, SMR_GROUP_MEMBER_SCALARS): f's constants differ from member to member.  A third table holds one row
// of W doubles per member (Canon::fc for a recognised functor, ProgD::consts for a program); the workgroup reads its member's row
// by scalar loads like the descriptor and rebuilds the functor's constants from it (set_consts, smr_device.h) before any data
// load.  Without VARC the functor is the kernel argument as it came: one f for the whole launch.
// Compiled once per compute type (-DSMR_CT=n).
#ifndef SMR_JIT
#include <utility>
#endif

#include "smr_dispatch.h"
#include "smr_group.h"

#ifndef SMR_CT
#error "compile with -DSMR_CT=0..3 or 7"
#endif

namespace smr {

struct GroupArgs {
    const GroupMemberD* members;
    const uint32_t* first_wg;  // count + 1 prefix sums
    int32_t count, M;
    int32_t dtype[MAXM];
    int32_t conj[MAXM];
    uint32_t wg0;              // first workgroup of this launch within the group (0: the launch is the whole group)
    int32_t W;                 // VARC: doubles per row of `consts` (behind wg0, which keeps its place in the kernarg segment)
    const double* consts;      // VARC: count rows of f's constants, one per member (null otherwise)
};

template <class T, class F, bool MIXED, bool VARC = false>
SMR_DEV void group_body(const GroupArgs a, F f) {
    __shared__ T tile[GROUP_TILE * (GROUP_TILE + 1)];
    const int nin = (F::NIN >= 0) ? F::NIN : a.M - 1;
    // the member of this workgroup, by its index in the group (smr_group.h: group_member_of)
    const uint32_t b = blockIdx.x + a.wg0;
    GroupWordC* const first_wg = (GroupWordC*)a.first_wg;
    const int lo = group_member_of(first_wg, a.count, b);
    GroupMemberC& m = ((GroupMemberC*)a.members)[lo];
    const uint32_t w = b - first_wg[lo];
    if constexpr (VARC) f.set_consts((GroupConstC*)a.consts + (i64)lo * a.W);
    OpTab t;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
        t.base[k] = m.base[k];
        t.dtype[k] = a.dtype[k];
        t.conj[k] = a.conj[k];
    }
    const int N = m.N;
    if (m.form == 0) {
        const uint32_t total = m.total;
        const uint32_t i0 = w * (uint32_t)GROUP_CHUNK + threadIdx.x;
        uint32_t c[MAXN];
        {
            uint32_t rem = i0;
#pragma unroll
            for (int d = 0; d < MAXN; ++d) {
                c[d] = 0;
                if (d < N) {
                    const uint32_t dd = m.dims[d];
                    const uint32_t q = rem / dd;
                    c[d] = rem - q * dd;
                    rem = q;
                }
            }
        }
        T in[GROUP_U][MAXIN];
        i64 off0[GROUP_U];
#pragma unroll
        for (int u = 0; u < GROUP_U; ++u) {
            const bool valid = i0 + (uint32_t)(u * 256) < total;  // (total < 2^31: no wrap)
            i64 off[MAXM];
#pragma unroll
            for (int k = 0; k < MAXM; ++k) off[k] = 0;
#pragma unroll
            for (int d = 0; d < MAXN; ++d)
                if (d < N) {
#pragma unroll
                    for (int k = 0; k < MAXM; ++k)
                        if (k < a.M) off[k] += (i64)c[d] * m.strides[k][d];
                }
            off0[u] = off[0];
#pragma unroll
            for (int k = 0; k < MAXIN; ++k) {
                in[u][k] = T{};
                if (k < nin && valid) in[u][k] = load_op<T, MIXED>(t, k + 1, off[k + 1]);
            }
            // the next element of this lane: index + 256, as a mixed-radix addition (digits past `total` are never used)
            uint32_t carry = 0;
#pragma unroll
            for (int d = 0; d < MAXN; ++d)
                if (d < N) {
                    const uint32_t x = c[d] + m.step[d] + carry;
                    carry = x >= m.dims[d] ? 1u : 0u;
                    c[d] = carry ? x - m.dims[d] : x;
                }
        }
#pragma unroll
        for (int u = 0; u < GROUP_U; ++u)
            if (i0 + (uint32_t)(u * 256) < total) store_op<T, MIXED>(t, off0[u], f(in[u]));
    } else {
        // tile (tp, tq) of the plane, then the outer dims, from the member-local workgroup index (all wave-uniform)
        uint32_t r = w;
        const uint32_t tp = r % m.ntp;
        r /= m.ntp;
        const uint32_t tq = r % m.ntq;
        r /= m.ntq;
        const int qd = m.q, kt = m.kt;
        i64 ob[MAXM];
#pragma unroll
        for (int k = 0; k < MAXM; ++k) ob[k] = 0;
#pragma unroll
        for (int d = 1; d < MAXN; ++d)
            if (d < N && d != qd) {
                const uint32_t dd = m.dims[d];
                const uint32_t q = r / dd;
                const i64 cc = (i64)(r - q * dd);
                r = q;
#pragma unroll
                for (int k = 0; k < MAXM; ++k)
                    if (k < a.M) ob[k] += cc * m.strides[k][d];
            }
        const uint32_t np = m.dims[0];
        uint32_t nq = 1;
        i64 obt = 0;  // the staged input's outer offset
#pragma unroll
        for (int d = 1; d < MAXN; ++d)
            if (d == qd) nq = m.dims[d];
#pragma unroll
        for (int k = 1; k < MAXM; ++k)
            if (k == kt) obt = ob[k];
        OpTab ts;  // slot 1 = the staged input: no register array is indexed by a run-time value
        ts.base[0] = nullptr;
        ts.base[1] = m.tbase;
        ts.dtype[0] = ts.dtype[1] = m.tdtype;
        ts.conj[0] = ts.conj[1] = m.tconj;
        const uint32_t lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
        const uint32_t p0 = tp * GROUP_TILE, q0 = tq * GROUP_TILE;
        // in: lanes run along q, the staged input's unit-stride dim
#pragma unroll
        for (int rr = 0; rr < GROUP_TILE / 8; ++rr) {
            const uint32_t p = ly + 8 * rr;
            const uint32_t gp = p0 + p, gq = q0 + lx;
            if (gp < np && gq < nq) tile[p * (GROUP_TILE + 1) + lx] = load_op<T, MIXED>(ts, 1, obt + (i64)gp * m.tsp + (i64)gq * m.tsq);
        }
        __syncthreads();
        // out: lanes run along dim 0, the destination's fastest dim
#pragma unroll
        for (int rr = 0; rr < GROUP_TILE / 8; ++rr) {
            const uint32_t qq = ly + 8 * rr;
            const uint32_t gp = p0 + lx, gq = q0 + qq;
            if (gp < np && gq < nq) {
                T in[MAXIN];
#pragma unroll
                for (int k = 0; k < MAXIN; ++k) {
                    in[k] = T{};
                    if (k < nin) {
                        if (k + 1 == kt) in[k] = tile[lx * (GROUP_TILE + 1) + qq];
                        else in[k] = load_op<T, MIXED>(t, k + 1, ob[k + 1] + (i64)gp * m.strides[k + 1][0] + (i64)gq * m.qstride[k + 1]);
                    }
                }
                store_op<T, MIXED>(t, ob[0] + (i64)gp * m.strides[0][0] + (i64)gq * m.qstride[0], f(in));
            }
        }
    }
}

#ifndef SMR_JIT
template <class T, class F, bool MIXED>
__global__ void __launch_bounds__(256) k_group(GroupArgs a, F f) {
    group_body<T, F, MIXED>(a, f);
}

template <class T, class F, bool MIXED>
__global__ void __launch_bounds__(256) k_group_varc(GroupArgs a, F f) {
    group_body<T, F, MIXED, true>(a, f);
}

// does F take constants on the device (set_consts)?  Only such a functor has a VARC instantiation
template <class F, class = void> struct takes_consts { static constexpr bool value = false; };
template <class F> struct takes_consts<F, decltype(std::declval<F&>().set_consts((const double*)nullptr))> { static constexpr bool value = true; };

template <class T, class F, bool MIXED>
static int go(const GroupPlan& g, hipStream_t s, F f) {
    const Canon& c = g.c;
    GroupArgs a;
    a.members = (const GroupMemberD*)g.d_members;
    a.first_wg = (const uint32_t*)g.d_first;
    a.count = (int32_t)g.map.members.size();
    a.M = c.M;
    for (int k = 0; k < MAXM; ++k) {
        a.dtype[k] = k < c.M ? c.dtype[k] : 0;
        a.conj[k] = k < c.M ? c.conj[k] : 0;
    }
    a.wg0 = 0;
    const bool varc = g.map.varc;
    a.W = varc ? g.map.W : 0;
    a.consts = varc ? (const double*)g.map.d_consts : nullptr;
    const unsigned grid = g.first_wg.back();
    // the members are independent and a workgroup serves one member: any contiguous block range can be launched on its own.  `a` is
    // the first kernel parameter of k_group and of the runtime-compiled entry alike, so wg0 has one kernarg offset in both
    mark_sliceable(1, (unsigned)offsetof(GroupArgs, wg0), 0);
    if constexpr (is_jit<F>::value) {
        // the kernel argument kc holds member 0's constants and goes unused under VARC; the text depends on f's structure only
        if (varc) return launch_jit<T>(c, s, "group", "smr::GroupArgs", "group_body", "", grid, 256, 0, a, MIXED, true);
        return launch_jit<T>(c, s, "group", "smr::GroupArgs", "group_body", "", grid, 256, 0, a, MIXED);
    } else {
        if constexpr (takes_consts<F>::value) {
            if (varc)
                return launch_native(nullptr, 0, "k_group_varc", [&] { SMR_LAUNCH((k_group_varc<T, F, MIXED>), dim3(grid), dim3(256), 0, s, a, f); });
        } else if (varc) {
            return set_error(SMR_EINVAL, "group: per-member scalars planned for an f without constants");
        }
        return launch_native(nullptr, 0, "k_group", [&] { SMR_LAUNCH((k_group<T, F, MIXED>), dim3(grid), dim3(256), 0, s, a, f); });
    }
}

template <>
int launch_group_ct<SMR_CT>(const GroupPlan& g, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = g.c;
    if (c.bitcopy) return with_bitcopy<SMR_CT>(c, [&](auto f) { return go<typename ident_elem<decltype(f)>::type, decltype(f), false>(g, s, f); });
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go<T, decltype(f), true>(g, s, f); });
    return with_functor<T>(c, GROUP_FMASK, [&](auto f) { return go<T, decltype(f), false>(g, s, f); });
}
#endif  // !SMR_JIT

}  // namespace smr
