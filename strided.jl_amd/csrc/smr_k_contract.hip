// smr_k_contract.hip -- FAM_CONTRACT: outer-product reductions, LDS- and register-tiled
//
//     dest[i, j, rest] = op(initop(dest[i, j, rest]), op over (q, k) of f(in1[i, k, q, rest], in2[j, k, q, rest]))
//
// The box of the reference's generic __mul! (src/linalg.jl:130-162: C2 = (m, n, 1), A2 = (m, 1, k), B2 = (1, n, k)) and of every
// reduction shaped like it -- pairwise distances, min-plus products, Boolean products, contractions written as mapreducedim! over
// views.  Input 1 varies along kept dim di and not along dj, input 2 the other way round; k is the inner reduced dim NK, q the outer
// reduced index (dims NK+1.., dim NK+1 fastest), `rest` the other kept dims (decoded once per workgroup, never tiled).
//
// 256 lanes = 16 x 16.  A workgroup owns a TILE x TILE block of outputs (TILE = 16 * RB, RB = 4, 2 or 1), a lane an RB x RB block of
// accumulators in registers.  The reduced space is walked in chunks of TK along k (smr_internal.h: contract_tk): per chunk the workgroup stages the TILE x TK tile
// of each input in LDS (compute-class values: operand types are converted and conj flags applied while staging), and after the barrier
// every lane runs acc[r][s] = op(acc[r][s], f(a[r], b[s])) for the chunk's k in ascending order.  The two LDS tiles are double
// buffered: the global loads of chunk t+1 are in flight while chunk t is consumed; one barrier per chunk.
//
// ACCUMULATION ORDER (defined): every output is accumulated by ONE lane, seeded with the neutral element of `op`, over q ascending and
// inside it over k ascending; the (init-ed) old destination is combined last: dest = op(initop(old), acc).  For real floats the result
// is therefore bit-identical to the plain sequential loop.  (REDUCE_PART's COL form folds rows through an LDS tree instead.)
//
// Ragged extents: loads of lanes past the end of di / dj and of rows past the end of k are CLAMPED to a valid address, never branched
// around; their outputs are never stored and their k rows never consumed (the k loop is bounded by the true extent: f and op are
// arbitrary, no padding value is neutral).  Whole tiles run a copy of the body without the clamps along di / dj, with 16-byte global
// loads where both inputs allow them (smr_plan_contract.cpp: contract_vec).
//
// LDS layout: tile[k][t], t the tiled index, rows padded by 16 bytes.  A lane reads its RB values of a row as 16-byte (or RB-element)
// pieces that are contiguous over the 16 lanes along that dim and a broadcast over the 16 lanes along the other: conflict-free.
// One launch, no partials, no scratch: the plan runs unchanged through eager direct dispatch and recorded sequences.
//
// SPLIT FORM (option "contract_split", off by default; smr_plan_contract.cpp: contract_split_rule): few output tiles and a long reduced
// range.  The walk over the Q * nkc chunks (chunk t: q = t / nkc, rows k in [kc * TK, min((kc + 1) * TK, K)) ascending, kc = t % nkc)
// is cut into S = kparts contiguous slices of cps chunks, the last one possibly shorter, none empty.  k_contract_split runs one
// workgroup per (tile, slice): the same tile body over chunks [s * cps, min((s + 1) * cps, Q * nkc)), seeded with the neutral element,
// whose register block is stored -- compute-class values, no conversion, no conj -- to partials[tile][slice][register r * RB + s][lane];
// ragged tiles store all their lanes (the buffer holds whole tiles).  k_contract_fold then folds every output's S partials in slice
// order and applies the epilogue.  ACCUMULATION ORDER OF THE SPLIT FORM (defined):
//     dest = op(initop(old), op(... op(op(P_0, P_1), P_2) ..., P_{S-1})),
// P_s the sequential accumulation, from the neutral element, over the chunks of slice s in ascending order.  Results are run-to-run
// identical and, for real floats, bit-identical to that loop written on the host; they are NOT those of the unsplit loop, which is
// why the form is opt-in.  No atomics, no waiting on another workgroup: the second launch is the only fold form.
// The tile body itself (staging, chunk loop, epilogue) lives in smr_contract.h: the grouped kernel (smr_k_gcontract.hip) runs it too.
#include "smr_contract.h"

#ifndef SMR_CT
#error "compile with -DSMR_CT=0..3 or 7"
#endif

namespace smr {

template <class T, class F, bool MIXED, int RB>
SMR_DEV void contract_body(const ContractArgs a, F f) {
    typedef CGeom<T, RB> G;
    // one allocation for both copies of the body: [buffer][input][TK][LD]
    __shared__ __attribute__((aligned(16))) T lds[2 * 2 * G::TK * G::LD];
    static_assert(sizeof(T) * 2 * 2 * G::TK * G::LD == contract_lds(G::ES, RB), "the planner's LDS figure is the kernel's");
    contract_by_op<T, F, MIXED, RB, false>(a, a.ops, a.redop, f, lds, (i64)blockIdx.x, 0, a.Q * a.nkc, (T*)nullptr);
}

// The split form's main launch: workgroup b is (tile = b % tiles, slice = b / tiles) -- the slice is the slow digit, so consecutive
// workgroups walk the same k-slice of neighbouring tiles and find each other's input rows in L2 (not measured against the other
// order) -- and stores its register block, accumulated from the neutral element over its slice alone, to its place in the partials.
template <class T, class F, bool MIXED, int RB>
SMR_DEV void contract_split_body(const ContractSplitArgs a, F f) {
    typedef CGeom<T, RB> G;
    __shared__ __attribute__((aligned(16))) T lds[2 * 2 * G::TK * G::LD];
    const i64 b = (i64)blockIdx.x, sl = b / a.tiles, tile = b - sl * a.tiles;
    const i64 nchunks = a.c.Q * a.c.nkc, t_lo = sl * a.cps, t_hi = t_lo + a.cps < nchunks ? t_lo + a.cps : nchunks;
    T* sink = (T*)a.partials + (tile * a.kparts + sl) * (i64)(RB * RB * 256);
    contract_by_op<T, F, MIXED, RB, true>(a.c, a.c.ops, a.c.redop, f, lds, tile, t_lo, t_hi, sink);
}

#ifndef SMR_JIT
// This file is compiled twice per compute type: as it is (k_contract and the family's entry point), and with -DSMR_CONTRACT_SPLIT
// (the split form's two kernels and their entry point) -- objects of their own, so that k_contract's code objects are the ones of
// the library before the split form (kernels added to a translation unit change the register allocation of the ones it held:
// profiles/contract_split.txt).
#ifndef SMR_CONTRACT_SPLIT
template <class T, class F, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_contract(ContractArgs a, F f) {
    contract_body<T, F, MIXED, RB>(a, f);
}
#else
template <class T, class F, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_contract_split(ContractSplitArgs a, F f) {
    contract_split_body<T, F, MIXED, RB>(a, f);
}

// The split form's second launch: one lane per (tile, register, lane) of the main launch -- workgroup b is (register = b % RB^2,
// tile = b / RB^2) -- folds that output's kparts partials in slice order, acc = P_0; acc = op(acc, P_s) for s = 1 .. kparts - 1, and
// puts the result through the epilogue; lanes past the end of a ragged tile drop theirs.  It does not call f.  The reads of a wave
// are 64 consecutive values; eight partials are loaded (index clamped, never guarded) before the first of them is used, as in
// k_reduce_part_final: they were written by the launch before, and guarded loads one by one are as many serial round trips.
template <class T, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_contract_fold(ContractSplitArgs a) {
    typedef CGeom<T, RB> G;
    const ContractArgs& g = a.c;
    i64 b = (i64)blockIdx.x;
    const int reg = (int)(b % (RB * RB));
    b /= RB * RB;
    const T* p = (const T*)a.partials + b * a.kparts * (i64)(RB * RB * 256) + reg * 256 + (int)threadIdx.x;
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
    const int last = a.kparts - 1;
    T acc = p[0];
    for (int s0 = 1; s0 <= last; s0 += 8) {
        T x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = p[(i64)(s0 + e < last ? s0 + e : last) * SL];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const T t = red_apply<T>(g.redop, acc, x[e]);
            if (s0 + e <= last) acc = t;
        }
    }
    contract_epilogue<T, MIXED>(g, g.ops, off0 + i * g.strides[0][g.di] + j * g.strides[0][g.dj], acc);
}
#endif  // SMR_CONTRACT_SPLIT

#ifndef SMR_CONTRACT_SPLIT
template <class T, class F, bool MIXED, int RB>
static int launch_rb(const Canon& c, const ContractArgs& a, unsigned grid, hipStream_t s, F f) {
    if constexpr (is_jit<F>::value)
        return launch_jit<T>(c, s, "contract", "smr::ContractArgs", "contract_body", "", grid, 256, 0, a, MIXED, RB);
    else
        return launch_native(nullptr, 0, "k_contract", [&] { SMR_LAUNCH((k_contract<T, F, MIXED, RB>), dim3(grid), dim3(256), 0, s, a, f); });
}
#else
// the two launches of the split form: (tile, slice) workgroups into the plan's partials, then the fold (native: it does not call f)
template <class T, class F, bool MIXED, int RB>
static int launch_split_rb(const Plan& plan, const ContractSplitArgs& a, hipStream_t s, F f) {
    const ContractPlan& cp = plan.contract;
    const unsigned grid = (unsigned)(cp.grid * cp.kparts);
    int rc;
    if constexpr (is_jit<F>::value)
        rc = launch_jit<T>(plan.c, s, "contract", "smr::ContractSplitArgs", "contract_split_body", "", grid, 256, 0, a, MIXED, RB);
    else
        rc = launch_native(nullptr, 0, "k_contract_split", [&] { SMR_LAUNCH((k_contract_split<T, F, MIXED, RB>), dim3(grid), dim3(256), 0, s, a, f); });
    if (rc || jit_no_launch()) return rc;
    SMR_LAUNCH((k_contract_fold<T, MIXED, RB>), dim3((unsigned)(cp.grid * RB * RB)), dim3(256), 0, s, a);
    return check_launch("k_contract_fold");
}
#endif  // SMR_CONTRACT_SPLIT

template <class T, class F, bool MIXED>
static int go_contract(const Plan& plan, void* const* bases, hipStream_t s, F f) {
    const Canon& c = plan.c;
    const ContractPlan& cp = plan.contract;
    ContractArgs a;
    std::memset(&a, 0, sizeof a);
    a.ops = make_optab(c, bases);
    // the geometry both kernels of the family read (smr_contract.h); the tile is the plan's
    const i64 wgs = contract_fill(a, c, cp.di, cp.dj, contract_vec(plan, bases), cp.rb);
    if (wgs != cp.grid || a.nti != cp.nti || a.ntj != cp.ntj) return set_error(SMR_EINVAL, "contract plan does not match the kernel's tile geometry");
    if (cp.tk != contract_tk((int)sizeof(T), cp.rb) || contract_lds((int)sizeof(T), cp.rb) != cp.lds_bytes) return set_error(SMR_EINVAL, "contract plan does not match the kernel's tile geometry");
#ifdef SMR_CONTRACT_SPLIT
    {
        // (a dry run compiles without a device: no partials yet, and nothing is launched)
        if (!plan.scratch && !jit_dry_run()) return set_error(SMR_EINVAL, "split contract plan without its partials buffer");
        if ((a.Q * a.nkc + cp.cps - 1) / cp.cps != cp.kparts) return set_error(SMR_EINVAL, "contract plan does not match the kernel's tile geometry");
        ContractSplitArgs sa;
        std::memset(&sa, 0, sizeof sa);
        sa.c = a;
        sa.partials = plan.scratch;
        sa.tiles = cp.grid;
        sa.cps = cp.cps;
        sa.kparts = cp.kparts;
        if (cp.rb == 4) return launch_split_rb<T, F, MIXED, 4>(plan, sa, s, f);
        if (cp.rb == 2) return launch_split_rb<T, F, MIXED, 2>(plan, sa, s, f);
        return launch_split_rb<T, F, MIXED, 1>(plan, sa, s, f);
    }
#else
    if (cp.rb == 4) return launch_rb<T, F, MIXED, 4>(c, a, (unsigned)cp.grid, s, f);
    if (cp.rb == 2) return launch_rb<T, F, MIXED, 2>(c, a, (unsigned)cp.grid, s, f);
    return launch_rb<T, F, MIXED, 1>(c, a, (unsigned)cp.grid, s, f);
#endif
}

// (the same dispatch over f for both objects: the unsplit one hands split plans to the other)
template <>
#ifdef SMR_CONTRACT_SPLIT
int launch_contract_split_ct<SMR_CT>(const Plan& plan, void* const* bases, hipStream_t s) {
#else
int launch_contract_ct<SMR_CT>(const Plan& plan, void* const* bases, hipStream_t s) {
    if (plan.contract.kparts > 1) return launch_contract_split_ct<SMR_CT>(plan, bases, s);
#endif
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = plan.c;
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go_contract<T, decltype(f), true>(plan, bases, s, f); });
    // natively compiled: the product (with_functor would instantiate the kernel for every functor kind; this family has two inputs
    // and an RB x RB unrolled body, so only the one __mul! needs is built -- every other f is runtime-compiled or interpreted)
    if (c.fkind == FK_MUL2) return go_contract<T, FMul2<T>, false>(plan, bases, s, FMul2<T>{});
    return with_prog<T>(c, [&](auto f) { return go_contract<T, decltype(f), false>(plan, bases, s, f); });
}
#endif  // !SMR_JIT

}  // namespace smr
