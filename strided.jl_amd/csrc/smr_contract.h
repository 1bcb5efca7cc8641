// smr_contract.h -- the device code of FAM_CONTRACT's tile (staging, the register-blocked chunk loop, the epilogue), shared by the
// single-call kernel (smr_k_contract.hip) and the grouped one (smr_k_gcontract.hip), and the host code that fills the geometry both
// read.  Also compiled by hiprtc (SMR_JIT): the runtime compiler embeds it by name.
//
// Every function is a template over the type A of the geometry it reads: `const ContractArgs` (a kernel argument) in a single call,
// `GroupContractMemberC` -- a member's descriptor in a device table, read through the constant address space -- in a group.  The
// body indexes strides[k][NK], dims[di] and so on with run-time (wave-uniform) indices; read in place through A those are scalar
// loads, whereas a by-value copy of a descriptor in a local would send them to scratch memory.  The operand table (addresses, dtypes,
// conj flags) is passed next to it: a group builds it in registers from the member's addresses and the launch's dtypes.
#pragma once

#include "smr_dispatch.h"
#ifndef SMR_JIT
#include <cstdlib>
#endif

namespace smr {

struct ContractArgs {
    OpTab ops;
    int32_t N, NK, redop, initop, di, dj, vec, nrd;
    int32_t rdim[MAXN];    // the kept dims other than di / dj, in the order the workgroup index decodes them
    int32_t mode[3];       // per input: lanes of a staging pass run along 0 = the tiled dim, 1 = k
    i64 dims[MAXN];
    i64 strides[3][MAXN];
    double beta[2];
    i64 nti, ntj, K, Q, nkc;  // tiles along di / dj, extent of dim NK, outer reduced indices, chunks per q
};

// The split form (smr_k_contract.hip: k_contract_split / k_contract_fold): the geometry above, and how the chunk walk over (q, k)
// is cut.  Workgroup b of the main launch is (tile = b % tiles, slice = b / tiles) and walks chunks [slice * cps, min((slice + 1) *
// cps, Q * nkc)); its register block goes to partials[tile][slice][register r * RB + s][lane 0..255], compute-class values.
struct ContractSplitArgs {
    ContractArgs c;
    void* partials;
    i64 tiles, cps;
    int32_t kparts, pad_;
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
template <class T, bool MIXED, int RB, bool EDGE, bool VEC, class A>
SMR_DEV void contract_fetch(A& a, const OpTab& ops, int k, int dt, T* r, i64 base, i64 t0, i64 k0) {
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
                VT x = *reinterpret_cast<const VT*>((const T*)ops.base[k] + off);
                if constexpr (tr<T>::cx) {
                    if (ops.conj[k]) {
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
            r[p] = load_op<T, MIXED>(ops, k, base + ti * st + kq * sk);
        }
    }
}

// ... and from the registers into the LDS tile
template <class T, int RB, bool VEC, class A>
SMR_DEV void contract_stash(A& a, int k, const T* r, T* tile) {
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
template <class A>
SMR_DEV void contract_qoff(A& a, i64 q, i64* qo) {
    qo[1] = qo[2] = 0;
#pragma nounroll
    for (int d = a.NK + 1; d < a.N; ++d) {
        const i64 n = a.dims[d], x = q / n, cd = q - x * n;
        q = x;
        qo[1] += cd * a.strides[1][d];
        qo[2] += cd * a.strides[2][d];
    }
}

template <class T, bool MIXED, class A>
SMR_DEV void contract_epilogue(A& a, const OpTab& ops, i64 off0, T acc) {
    typedef typename tr<T>::real R;
    const T beta = mk<T>(rcast<R>(a.beta[0]), rcast<R>(a.beta[1]));
    T old;
    if (a.initop == SMR_INIT_ZERO || a.initop == SMR_INIT_CONST) {
        old = init_apply<T>(a.initop, T{}, beta);  // does not depend on what the destination held: no load
    } else {
        old = load_op<T, MIXED>(ops, 0, off0);
        if (a.initop != SMR_INIT_NONE) old = init_apply<T>(a.initop, old, beta);
    }
    store_op<T, MIXED>(ops, off0, red_apply<T>(a.redop, old, acc));
}

// one workgroup's tile: origin (i0, j0), `boff` the operands' offsets of the workgroup's `rest` index.  The workgroup walks chunks
// [t_lo, t_hi) of the Q * nkc chunks of the reduced space (chunk t: outer reduced index q = t / nkc, rows [kc * TK, min((kc + 1) * TK,
// K)) with kc = t % nkc); the whole range in the unsplit kernels.  SPLIT (compile time): the register block is not put through the
// epilogue but stored, as it is, to `sink` -- [register r * RB + s][lane] -- by every lane, those past a ragged tile's end included.
template <class T, class F, bool MIXED, int RB, int OPC, bool EDGE, bool VEC, bool SPLIT, class A>
SMR_DEV void contract_tile(A& a, const OpTab& ops, const F& f, T* lds, i64 i0, i64 j0, const i64* boff, i64 t_lo, i64 t_hi, T* sink) {
    typedef CGeom<T, RB> G;
    const int redop = (OPC >= 0) ? OPC : a.redop;  // compile-time for the sum: no op switch inside the loops
    const int li = (int)threadIdx.x & (CONTRACT_LANES - 1), lj = (int)threadIdx.x >> 4;
    constexpr int TSZ = G::TK * G::LD;  // lds: [buffer][input][TK][LD]
    T acc[RB][RB];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int s = 0; s < RB; ++s) acc[r][s] = neutral<T>(redop);
    // (the unsplit copies are handed 0 and Q * nkc, and take them from here: they compile to what they did before the split form)
    if constexpr (!SPLIT) {
        t_lo = 0;
        t_hi = a.Q * a.nkc;
    }
    i64 qo[3] = {0, 0, 0};
    i64 q = 0, kc = 0;  // the chunk being fetched
    if (t_lo != 0) {
        q = t_lo / a.nkc;
        kc = t_lo - q * a.nkc;
        contract_qoff(a, q, qo);
    }
    T ra[G::NR], rb[G::NR];
    contract_fetch<T, MIXED, RB, EDGE, VEC>(a, ops, 1, a.di, ra, boff[1] + qo[1], i0, kc * G::TK);
    contract_fetch<T, MIXED, RB, EDGE, VEC>(a, ops, 2, a.dj, rb, boff[2] + qo[2], j0, kc * G::TK);
    contract_stash<T, RB, VEC>(a, 1, ra, lds);
    contract_stash<T, RB, VEC>(a, 2, rb, lds + TSZ);
    __syncthreads();
    for (i64 t = t_lo; t < t_hi; ++t) {
        const int cur = (int)((t - t_lo) & 1);
        const i64 kbeg = kc * G::TK;
        const int kn = (int)((a.K - kbeg < G::TK) ? a.K - kbeg : G::TK);  // rows of the chunk being consumed
        const bool more = t + 1 < t_hi;
        if (more) {
            if (++kc == a.nkc) {
                kc = 0;
                ++q;
                contract_qoff(a, q, qo);
            }
            contract_fetch<T, MIXED, RB, EDGE, VEC>(a, ops, 1, a.di, ra, boff[1] + qo[1], i0, kc * G::TK);
            contract_fetch<T, MIXED, RB, EDGE, VEC>(a, ops, 2, a.dj, rb, boff[2] + qo[2], j0, kc * G::TK);
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
    if constexpr (SPLIT) {
        // every store instruction of a wave writes 64 consecutive values
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int s = 0; s < RB; ++s) sink[(r * RB + s) * 256 + (int)threadIdx.x] = acc[r][s];
    } else {
        const i64 s0i = a.strides[0][a.di], s0j = a.strides[0][a.dj];
#pragma unroll
        for (int s = 0; s < RB; ++s)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const i64 i = i0 + G::idx(li, r), j = j0 + G::idx(lj, s);
                if (!EDGE || (i < a.dims[a.di] && j < a.dims[a.dj])) contract_epilogue<T, MIXED>(a, ops, boff[0] + i * s0i + j * s0j, acc[r][s]);
            }
    }
}

// workgroup `b` of the problem `a`: tile along di (fastest), tile along dj, the other kept dims.  (A single call passes blockIdx.x,
// a group the workgroup's index inside its member.)
template <class T, class F, bool MIXED, int RB, int OPC, bool SPLIT, class A>
SMR_DEV void contract_impl(A& a, const OpTab& ops, const F& f, T* lds, i64 b, i64 t_lo, i64 t_hi, T* sink) {
    typedef CGeom<T, RB> G;
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
        contract_tile<T, F, MIXED, RB, OPC, true, false, SPLIT>(a, ops, f, lds, i0, j0, boff, t_lo, t_hi, sink);
        return;
    }
    if constexpr (!MIXED && G::VE > 1) {
        if (a.vec > 1) {
            contract_tile<T, F, MIXED, RB, OPC, false, true, SPLIT>(a, ops, f, lds, i0, j0, boff, t_lo, t_hi, sink);
            return;
        }
    }
    contract_tile<T, F, MIXED, RB, OPC, false, false, SPLIT>(a, ops, f, lds, i0, j0, boff, t_lo, t_hi, sink);
}

// the sum gets a copy of the body with the operator fixed.  (Copies for min and max as well were measured and lost: registers are
// allocated for the whole kernel, and the NaN-aware min / max blocks pushed every path, the sum included, into scratch memory:
// 1024^3 Float32 87 -> 165 us.)
template <class T, class F, bool MIXED, int RB, bool SPLIT, class A>
SMR_DEV void contract_by_op(A& a, const OpTab& ops, int redop, const F& f, T* lds, i64 b, i64 t_lo, i64 t_hi, T* sink) {
    if (redop == SMR_RED_ADD)
        contract_impl<T, F, MIXED, RB, SMR_RED_ADD, SPLIT>(a, ops, f, lds, b, t_lo, t_hi, sink);
    else
        contract_impl<T, F, MIXED, RB, -1, SPLIT>(a, ops, f, lds, b, t_lo, t_hi, sink);
}

#ifndef SMR_JIT
// The split form's arithmetic, shared by the single call's planner (smr_plan_contract.cpp) and the group planner
// (smr_plan_group.cpp).  The constants are those of contract_split_rule, where the rows they were measured on are quoted.
constexpr i64 CONTRACT_SPLIT_MIN_CPS = 2, CONTRACT_SPLIT_MAX_S = 64, CONTRACT_SPLIT_TARGET = 512;

// Cuts a walk of `nchunks` chunks into at most `want` slices: clamped to the chunks, then cps = ceil(nchunks / S) and
// S = ceil(nchunks / cps), so no slice is empty.  Returns S and sets `cps`; 1 (and cps = nchunks): the walk is not cut.
inline i64 contract_slices(i64 nchunks, i64 want, i64& cps) {
    i64 S = want < nchunks ? want : nchunks;
    cps = nchunks;
    if (S < 2) return 1;
    const i64 per = (nchunks + S - 1) / S;
    S = (nchunks + per - 1) / per;
    if (S < 2) return 1;
    cps = per;
    return S;
}

// The most slices the rule allows a problem of `tiles` output tiles of edge `tile`: slices of at least MIN_CPS chunks, at most MAX_S
// of them, and the partials' round trip (2 * tiles * tile^2 * es per slice) at most half the bytes the inputs move, (mi + nj) * K * Q * es
inline i64 contract_split_smax(int es, i64 mi, i64 nj, i64 K, i64 Q, i64 nchunks, i64 tiles, i64 tile) {
    const long double in_bytes = (long double)(mi + nj) * (long double)K * (long double)Q * es;
    const long double per_slice = 2.0L * (long double)tiles * (long double)(tile * tile) * es;
    i64 smax = nchunks / CONTRACT_SPLIT_MIN_CPS < CONTRACT_SPLIT_MAX_S ? nchunks / CONTRACT_SPLIT_MIN_CPS : CONTRACT_SPLIT_MAX_S;
    const i64 by_bytes = (i64)(in_bytes / 2 / per_slice);
    return smax < by_bytes ? smax : by_bytes;
}

// The tile-dependent part of the geometry: tiles along di / dj and chunks per outer reduced index, for elements of `es` bytes and
// RB = rb.  Returns the problem's workgroups, nti * ntj * (the other kept extents), as plan_contract counts them.
template <class A>
i64 contract_set_tile(A& a, int es, int rb) {
    const i64 t = CONTRACT_LANES * rb, tk = contract_tk(es, rb);
    a.nti = (a.dims[a.di] + t - 1) / t;
    a.ntj = (a.dims[a.dj] + t - 1) / t;
    a.nkc = (a.K + tk - 1) / tk;
    i64 wgs = a.nti * a.ntj;
    for (int n = 0; n < a.nrd; ++n) wgs *= a.dims[a.rdim[n]];
    return wgs;
}

// Fills everything of ContractArgs / GroupContractMemberD but the operand addresses: the geometry of canonical problem `c` tiled
// along di / dj with `vec` elements per global load of whole tiles (contract_vec).  Returns the problem's workgroups.
template <class A>
i64 contract_fill(A& a, const Canon& c, int di, int dj, int vec, int rb) {
    a.N = c.N;
    a.NK = c.NK;
    a.redop = c.redop;
    a.initop = c.initop;
    a.di = di;
    a.dj = dj;
    a.vec = vec;
    a.nrd = 0;
    for (int d = 0; d < c.NK; ++d)
        if (d != di && d != dj) a.rdim[a.nrd++] = d;
    for (int i = 0; i < MAXN; ++i) a.dims[i] = (i < c.N) ? c.dims[i] : 1;
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < MAXN; ++i) a.strides[k][i] = (i < c.N) ? c.strides[k][i] : 0;
    // whichever of (tiled dim, k) has unit stride is the fast lane axis of the staging loads
    for (int k = 1; k < 3; ++k) {
        const int dt = k == 1 ? di : dj;
        a.mode[k] = (std::llabs(c.strides[k][dt]) != 1 && std::llabs(c.strides[k][c.NK]) == 1) ? 1 : 0;
        if (vec > 1) a.mode[k] = c.strides[k][dt] == 1 ? 0 : 1;
    }
    a.beta[0] = c.initarg[0];
    a.beta[1] = c.initarg[1];
    a.K = c.dims[c.NK];
    a.Q = c.total / c.nout / a.K;
    return contract_set_tile(a, dtype_size(c.ct), rb);
}
#endif  // !SMR_JIT

}  // namespace smr
