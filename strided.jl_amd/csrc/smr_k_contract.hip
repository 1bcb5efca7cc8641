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
    contract_by_op<T, F, MIXED, RB>(a, a.ops, a.redop, f, lds, (i64)blockIdx.x);
}

#ifndef SMR_JIT
template <class T, class F, bool MIXED, int RB>
__global__ void __launch_bounds__(256) k_contract(ContractArgs a, F f) {
    contract_body<T, F, MIXED, RB>(a, f);
}

template <class T, class F, bool MIXED, int RB>
static int launch_rb(const Canon& c, const ContractArgs& a, unsigned grid, hipStream_t s, F f) {
    if constexpr (is_jit<F>::value)
        return launch_jit<T>(c, s, "contract", "smr::ContractArgs", "contract_body", "", grid, 256, 0, a, MIXED, RB);
    else
        return launch_native(nullptr, 0, "k_contract", [&] { SMR_LAUNCH((k_contract<T, F, MIXED, RB>), dim3(grid), dim3(256), 0, s, a, f); });
}

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
    if (cp.rb == 4) return launch_rb<T, F, MIXED, 4>(c, a, (unsigned)cp.grid, s, f);
    if (cp.rb == 2) return launch_rb<T, F, MIXED, 2>(c, a, (unsigned)cp.grid, s, f);
    return launch_rb<T, F, MIXED, 1>(c, a, (unsigned)cp.grid, s, f);
}

template <>
int launch_contract_ct<SMR_CT>(const Plan& plan, void* const* bases, hipStream_t s) {
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
