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
#include "smr_dispatch.h"
#ifndef SMR_JIT
#include <cstdlib>
#endif

#ifndef SMR_CT
#error "compile with -DSMR_CT=0..3 or 7"
#endif

namespace smr {

struct ContractArgs {
    OpTab ops;
    int32_t N, NK, redop, initop, di, dj, vec, nrd;
    int32_t rdim[MAXN];    // the kept dims other than di / dj, in the order blockIdx.x decodes them
    int32_t mode[3];       // per input: lanes of a staging pass run along 0 = the tiled dim, 1 = k
    i64 dims[MAXN];
    i64 strides[3][MAXN];
    double beta[2];
    i64 nti, ntj, K, Q, nkc;  // tiles along di / dj, extent of dim NK, outer reduced indices, chunks per q
};

template <class T, int V>
struct alignas(sizeof(T) * V >= 16 ? 16 : sizeof(T) * V) CVec {
    T v[V];
};

template <class T, int RB>
struct CGeom {
    static constexpr int ES = (int)sizeof(T);
    static constexpr int TILE = CONTRACT_LANES * RB;
    static constexpr int TK = contract_tk(ES, RB);
    static constexpr int LD = TILE + contract_pad(ES);        // LDS row (elements)
    static constexpr int VE = ES >= 16 ? 1 : 16 / ES;          // elements per 16-byte vector
    static constexpr int CE = contract_ce(ES, RB);             // elements per LDS read piece
    static constexpr int NEL = TILE * TK;                      // elements of one staged tile
    static constexpr int PER = NEL / 256;                      // ... per lane
    static constexpr int NR = PER > VE ? PER : VE;             // staging registers per lane and input
    static_assert(NEL % 256 == 0 && PER >= 1, "a staged tile is a whole number of passes");
    // tiled index of the lane's r-th value (smr_internal.h: contract_idx)
    static SMR_DEV int idx(int t, int r) { return contract_idx(ES, RB, t, r); }
};

// global loads of one input's tile of one chunk into registers
template <class T, bool MIXED, int RB, bool EDGE, bool VEC>
SMR_DEV void contract_fetch(const ContractArgs& a, int k, int dt, T* r, i64 base, i64 t0, i64 k0) {
    typedef CGeom<T, RB> G;
    const i64 st = a.strides[k][dt], sk = a.strides[k][a.NK];
    const int mode = a.mode[k];
    if constexpr (VEC) {
        typedef CVec<T, G::VE> VT;
        constexpr int NV = G::NEL / G::VE;
#pragma unroll
        for (int p = 0; p < (NV + 255) / 256; ++p) {
            const int v = p * 256 + (int)threadIdx.x;
            if (NV % 256 == 0 || v < NV) {
                i64 off;
                if (mode == 0) {
                    const int tv = v % (G::TILE / G::VE), kk = v / (G::TILE / G::VE);
                    const i64 kq = (k0 + kk < a.K) ? k0 + kk : a.K - 1;
                    off = base + (t0 + tv * G::VE) + kq * sk;
                } else {
                    const int kv = v % (G::TK / G::VE), tt = v / (G::TK / G::VE);
                    const i64 ks = (k0 + kv * G::VE < a.K) ? k0 + kv * G::VE : a.K - G::VE;  // (K is a whole number of vectors)
                    off = base + (t0 + tt) * st + ks;
                }
                VT x = *reinterpret_cast<const VT*>((const T*)a.ops.base[k] + off);
                if constexpr (tr<T>::cx) {
                    if (a.ops.conj[k]) {
#pragma unroll
                        for (int e = 0; e < G::VE; ++e) x.v[e] = cj(x.v[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < G::VE; ++e) r[p * G::VE + e] = x.v[e];
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < G::PER; ++p) {
            const int e = p * 256 + (int)threadIdx.x;
            const int tt = mode == 0 ? e % G::TILE : e / G::TK, kk = mode == 0 ? e / G::TILE : e % G::TK;
            i64 ti = t0 + tt;
            if constexpr (EDGE) ti = ti < a.dims[dt] ? ti : a.dims[dt] - 1;
            const i64 kq = (k0 + kk < a.K) ? k0 + kk : a.K - 1;
            r[p] = load_op<T, MIXED>(a.ops, k, base + ti * st + kq * sk);
        }
    }
}

// ... and from the registers into the LDS tile
template <class T, int RB, bool VEC>
SMR_DEV void contract_stash(const ContractArgs& a, int k, const T* r, T* tile) {
    typedef CGeom<T, RB> G;
    const int mode = a.mode[k];
    if constexpr (VEC) {
        typedef CVec<T, G::VE> VT;
        constexpr int NV = G::NEL / G::VE;
#pragma unroll
        for (int p = 0; p < (NV + 255) / 256; ++p) {
            const int v = p * 256 + (int)threadIdx.x;
            if (NV % 256 == 0 || v < NV) {
                if (mode == 0) {
                    const int tv = v % (G::TILE / G::VE), kk = v / (G::TILE / G::VE);
                    VT x;
#pragma unroll
                    for (int e = 0; e < G::VE; ++e) x.v[e] = r[p * G::VE + e];
                    *reinterpret_cast<VT*>(tile + kk * G::LD + tv * G::VE) = x;
                } else {
                    const int kv = v % (G::TK / G::VE), tt = v / (G::TK / G::VE);
#pragma unroll
                    for (int e = 0; e < G::VE; ++e) tile[(kv * G::VE + e) * G::LD + tt] = r[p * G::VE + e];
                }
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < G::PER; ++p) {
            const int e = p * 256 + (int)threadIdx.x;
            const int tt = mode == 0 ? e % G::TILE : e / G::TK, kk = mode == 0 ? e / G::TILE : e % G::TK;
            tile[kk * G::LD + tt] = r[p];
        }
    }
}

// offsets of outer reduced index q (dims NK+1 .. N-1, dim NK+1 fastest) of the two inputs
SMR_DEV void contract_qoff(const ContractArgs& a, i64 q, i64* qo) {
    qo[1] = qo[2] = 0;
#pragma nounroll
    for (int d = a.NK + 1; d < a.N; ++d) {
        const i64 n = a.dims[d], x = q / n, cd = q - x * n;
        q = x;
        qo[1] += cd * a.strides[1][d];
        qo[2] += cd * a.strides[2][d];
    }
}

template <class T, bool MIXED>
SMR_DEV void contract_epilogue(const ContractArgs& a, i64 off0, T acc) {
    typedef typename tr<T>::real R;
    const T beta = mk<T>(rcast<R>(a.beta[0]), rcast<R>(a.beta[1]));
    T old;
    if (a.initop == SMR_INIT_ZERO || a.initop == SMR_INIT_CONST) {
        old = init_apply<T>(a.initop, T{}, beta);  // does not depend on what the destination held: no load
    } else {
        old = load_op<T, MIXED>(a.ops, 0, off0);
        if (a.initop != SMR_INIT_NONE) old = init_apply<T>(a.initop, old, beta);
    }
    store_op<T, MIXED>(a.ops, off0, red_apply<T>(a.redop, old, acc));
}

// one workgroup's tile: origin (i0, j0), `boff` the operands' offsets of the workgroup's `rest` index
template <class T, class F, bool MIXED, int RB, int OPC, bool EDGE, bool VEC>
SMR_DEV void contract_tile(const ContractArgs& a, const F& f, T* lds, i64 i0, i64 j0, const i64* boff) {
    typedef CGeom<T, RB> G;
    const int redop = (OPC >= 0) ? OPC : a.redop;  // compile-time for the sum: no op switch inside the loops
    const int li = (int)threadIdx.x & (CONTRACT_LANES - 1), lj = (int)threadIdx.x >> 4;
    constexpr int TSZ = G::TK * G::LD;  // lds: [buffer][input][TK][LD]
    T acc[RB][RB];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int s = 0; s < RB; ++s) acc[r][s] = neutral<T>(redop);
    const i64 nchunks = a.Q * a.nkc;
    i64 qo[3] = {0, 0, 0};
    i64 q = 0, kc = 0;  // the chunk being fetched
    T ra[G::NR], rb[G::NR];
    contract_fetch<T, MIXED, RB, EDGE, VEC>(a, 1, a.di, ra, boff[1], i0, 0);
    contract_fetch<T, MIXED, RB, EDGE, VEC>(a, 2, a.dj, rb, boff[2], j0, 0);
    contract_stash<T, RB, VEC>(a, 1, ra, lds);
    contract_stash<T, RB, VEC>(a, 2, rb, lds + TSZ);
    __syncthreads();
    for (i64 t = 0; t < nchunks; ++t) {
        const int cur = (int)(t & 1);
        const i64 kbeg = kc * G::TK;
        const int kn = (int)((a.K - kbeg < G::TK) ? a.K - kbeg : G::TK);  // rows of the chunk being consumed
        const bool more = t + 1 < nchunks;
        if (more) {
            if (++kc == a.nkc) {
                kc = 0;
                ++q;
                contract_qoff(a, q, qo);
            }
            contract_fetch<T, MIXED, RB, EDGE, VEC>(a, 1, a.di, ra, boff[1] + qo[1], i0, kc * G::TK);
            contract_fetch<T, MIXED, RB, EDGE, VEC>(a, 2, a.dj, rb, boff[2] + qo[2], j0, kc * G::TK);
        }
        const T* As = lds + cur * 2 * TSZ;
        const T* Bs = As + TSZ;
        auto step = [&](int kk) {
            typedef CVec<T, G::CE> PT;
            T av[RB], bv[RB];
#pragma unroll
            for (int r = 0; r < RB; r += G::CE) {
                const PT pa = *reinterpret_cast<const PT*>(As + kk * G::LD + G::idx(li, r));
                const PT pb = *reinterpret_cast<const PT*>(Bs + kk * G::LD + G::idx(lj, r));
#pragma unroll
                for (int e = 0; e < G::CE; ++e) {
                    av[r + e] = pa.v[e];
                    bv[r + e] = pb.v[e];
                }
            }
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int s = 0; s < RB; ++s) {
                    T in[MAXIN];
#pragma unroll
                    for (int m = 0; m < MAXIN; ++m) in[m] = T{};
                    in[0] = av[r];
                    in[1] = bv[s];
                    acc[r][s] = red_apply<T>(redop, acc[r][s], f(in));
                }
        };
        // (the interpreter, NIN < 0, is not unrolled over k: RB * RB copies of it per row are code enough)
        if (F::NIN >= 0 && kn == G::TK) {
            // unrolled in blocks of at most 16 rows: the code of one block, whatever the chunk
            constexpr int UB = G::TK < 16 ? G::TK : 16;
#pragma nounroll
            for (int kb = 0; kb < G::TK; kb += UB) {
#pragma unroll
                for (int kk = 0; kk < UB; ++kk) step(kb + kk);
            }
        } else {
#pragma nounroll
            for (int kk = 0; kk < kn; ++kk) step(kk);
        }
        if (more) {
            T* nx = lds + (cur ^ 1) * 2 * TSZ;
            contract_stash<T, RB, VEC>(a, 1, ra, nx);
            contract_stash<T, RB, VEC>(a, 2, rb, nx + TSZ);
        }
        __syncthreads();
    }
    const i64 s0i = a.strides[0][a.di], s0j = a.strides[0][a.dj];
#pragma unroll
    for (int s = 0; s < RB; ++s)
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const i64 i = i0 + G::idx(li, r), j = j0 + G::idx(lj, s);
            if (!EDGE || (i < a.dims[a.di] && j < a.dims[a.dj])) contract_epilogue<T, MIXED>(a, boff[0] + i * s0i + j * s0j, acc[r][s]);
        }
}

template <class T, class F, bool MIXED, int RB, int OPC>
SMR_DEV void contract_impl(const ContractArgs& a, const F& f, T* lds) {
    typedef CGeom<T, RB> G;
    // blockIdx.x = tile along di (fastest), tile along dj, the other kept dims
    i64 b = blockIdx.x;
    const i64 bi = b % a.nti;
    b /= a.nti;
    const i64 bj = b % a.ntj;
    b /= a.ntj;
    i64 boff[3] = {0, 0, 0};
#pragma nounroll
    for (int n = 0; n < a.nrd; ++n) {
        const int d = a.rdim[n];
        const i64 x = b / a.dims[d], cd = b - x * a.dims[d];
        b = x;
#pragma unroll
        for (int k = 0; k < 3; ++k) boff[k] += cd * a.strides[k][d];
    }
    const i64 i0 = bi * G::TILE, j0 = bj * G::TILE;
    const bool whole = i0 + G::TILE <= a.dims[a.di] && j0 + G::TILE <= a.dims[a.dj];
    if (!whole) {
        contract_tile<T, F, MIXED, RB, OPC, true, false>(a, f, lds, i0, j0, boff);
        return;
    }
    if constexpr (!MIXED && G::VE > 1) {
        if (a.vec > 1) {
            contract_tile<T, F, MIXED, RB, OPC, false, true>(a, f, lds, i0, j0, boff);
            return;
        }
    }
    contract_tile<T, F, MIXED, RB, OPC, false, false>(a, f, lds, i0, j0, boff);
}

template <class T, class F, bool MIXED, int RB>
SMR_DEV void contract_body(const ContractArgs a, F f) {
    typedef CGeom<T, RB> G;
    // one allocation for both copies of the body: [buffer][input][TK][LD]
    __shared__ __attribute__((aligned(16))) T lds[2 * 2 * G::TK * G::LD];
    static_assert(sizeof(T) * 2 * 2 * G::TK * G::LD == contract_lds(G::ES, RB), "the planner's LDS figure is the kernel's");
    // the sum gets a copy of the body with the operator fixed.  (Copies for min and max as well were measured and lost: registers are
    // allocated for the whole kernel, and the NaN-aware min / max blocks pushed every path, the sum included, into scratch memory:
    // 1024^3 Float32 87 -> 165 us.)
    if (a.redop == SMR_RED_ADD)
        contract_impl<T, F, MIXED, RB, SMR_RED_ADD>(a, f, lds);
    else
        contract_impl<T, F, MIXED, RB, -1>(a, f, lds);
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
    a.N = c.N;
    a.NK = c.NK;
    a.redop = c.redop;
    a.initop = c.initop;
    a.di = cp.di;
    a.dj = cp.dj;
    a.vec = contract_vec(plan, bases);
    for (int d = 0; d < c.NK; ++d)
        if (d != cp.di && d != cp.dj) a.rdim[a.nrd++] = d;
    for (int i = 0; i < MAXN; ++i) a.dims[i] = (i < c.N) ? c.dims[i] : 1;
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < MAXN; ++i) a.strides[k][i] = (i < c.N) ? c.strides[k][i] : 0;
    // whichever of (tiled dim, k) has unit stride is the fast lane axis of the staging loads
    for (int k = 1; k < 3; ++k) {
        const int dt = k == 1 ? cp.di : cp.dj;
        a.mode[k] = (std::llabs(c.strides[k][dt]) != 1 && std::llabs(c.strides[k][c.NK]) == 1) ? 1 : 0;
        if (a.vec > 1) a.mode[k] = c.strides[k][dt] == 1 ? 0 : 1;
    }
    a.beta[0] = c.initarg[0];
    a.beta[1] = c.initarg[1];
    a.nti = cp.nti;
    a.ntj = cp.ntj;
    a.K = c.dims[c.NK];
    a.Q = c.total / c.nout / a.K;
    a.nkc = (a.K + cp.tk - 1) / cp.tk;
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
