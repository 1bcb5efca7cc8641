// smr_k_tiled.hip -- family TILED: fused N-ary map whose operands have DIFFERENT unit-stride
// axes (permutedims!, adjoint!, B .= (A .+ A')./2, the 4-way permuted sum).
//
// MI355X design (not the reference's L1-blocked loop nest, src/mapreduce.jl:385-401):
//   * a workgroup owns one N-d tile whose extents are powers of two and which is long enough
//     along EVERY operand's unit-stride axis (1024 elements on 256 lanes; 4096 on 1024 lanes
//     for big problems with three or more distinct unit axes: always 4 elements per lane);
//   * phase A: every global load of the tile is issued up front: transposed inputs in THEIR
//     OWN stride order (consecutive lanes walk that input's unit-stride axis -> coalesced,
//     16 bytes per lane), direct inputs in destination order;
//   * phase B: transposed inputs are scattered into an LDS tile laid out in DESTINATION
//     order, XOR-swizzled with masks searched on the host per plan (build_tiled_args: GF(2) rank
//     test of every staged operand's write pattern and of the read pattern) so that neither the
//     strided writes nor the linear reads of a lane group collide on a bank;
//   * phase C: linear (conflict-free) LDS reads, f applied in registers, 16-byte coalesced
//     stores.
// Variants: the classic form runs one tile per workgroup (tiled_map_body; MODE selects at compile
// time which rarely needed features it carries); long work lists use the persistent,
// software-pipelined form (tiled_map_pipe_body).  Tiles are visited in the planner's order
// (smr_plan_tiled.cpp: plan_tile_order -- orbit-major when several inputs are permuted views of one
// buffer, so that they meet in one XCD's L2).
//
// Index arithmetic.  Tile extents are powers of two, so the position e of an element inside a
// tile (in any operand's enumeration order) is a bit string, and both its global byte offset
// and its swizzled LDS index are ADD/XOR-linear in those bits.  A lane owns NREP vectors of V
// consecutive elements: e = ((r*T + tid) << vlog) + h.  The host precomputes
//     lane table  (device memory, one row per lane and operand): byte offset + LDS index of
//                 the tid bits -- ONE 8-byte vector load per operand, issued first thing;
//     Gr[r], Lr[r], Lh[h] (kernel arguments): contribution of repeat index r / sub-element h,
// so the kernel contains no index arithmetic beyond one add (address) and one xor (LDS) per
// access.  Tile coordinates come from multiply-shift division of the workgroup id.  The kernel
// arguments (smr_tiled_args.h) are built once per plan by the device-free builder in smr_plan_tiled_args.cpp
// and cached (smr_api.cpp: tiled_launch_args patches the operand addresses and the store policy per call);
// this file holds the kernels, the dispatch on tiled_variant()'s choice and the launches.
// Measured history (32^4 f64, permutedims! / 4-way sum, us per launch): generic per-dim decode
// with dependent kernarg loads 11.5 / 28.5 (~2000 scalar instructions per wave: bound by the
// CU's single scalar unit) -> per-bit tables 6.0 / 14.6 -> 16-B vectors + repeat tables
// 4.4 / 9.9 -> all loads first, branch-free variants 4.1 / 8.9 -> lane tables 3.4 / 8.4 ->
// 4096-element tiles on 1024 lanes, searched swizzle, orbit-major order 3.4 / 6.85 -> compile-time
// modes 3.4 / 6.6 (a plain 16 MiB copy: 3.2; a 5-stream contiguous add: 5.4).
#include "smr_dispatch.h"
#include "smr_tiled_args.h"

#ifndef SMR_CT
#error "compile with -DSMR_CT=0..3 or 7"
#endif
#ifndef SMR_TILED_NTL
#define SMR_TILED_NTL 0
#endif

namespace smr {

SMR_DEV uint32_t fastdiv(uint32_t n, uint32_t m, uint32_t s) { return (__umulhi(m, n) + n) >> s; }

template <class T, int V>
struct alignas(sizeof(T) * V) TVec {
    T v[V];
};

// global-memory view of a lane's vector: element alignment only (round 6: odd extents and odd row strides keep 16-byte accesses;
// the hardware takes dwordx2 / dwordx4 at any dword address, as in smr_k_stream.hip)
template <class T, int V>
struct alignas(sizeof(T)) TUVec {
    T v[V];
};

template <class T, bool MIXED>
SMR_DEV T load_at(const char* p, int dtype, int conj) {
    T v;
    if constexpr (MIXED)
        v = ld_as<T>(p, 0, dtype);
    else
        v = *reinterpret_cast<const T*>(p);
    if constexpr (tr<T>::cx) {
        if (conj) v = cj(v);
    }
    return v;
}
template <class T, bool MIXED>
SMR_DEV void store_at(char* p, int dtype, int conj, T v) {
    if constexpr (tr<T>::cx) {
        if (conj) v = cj(v);
    }
    if constexpr (MIXED)
        st_as<T>(p, 0, dtype, v);
    else
        *reinterpret_cast<T*>(p) = v;
}

// V > 1 implies !MIXED && !WIDE and every direct operand unit-stride along dim 0 (launcher).
// MODE bit 0: bounds checks for ragged tiles, bit 1: tile-order lookup, bit 2: general tile origins
// (more than 4 grid dims, or origins beyond 4 GiB / negative steps).  The plain variant (0) carries
// none of it: code size and every extra scalar wait are part of the latency of a ~3.5 us launch
// (measured: permutedims! 3.48 -> 3.43 us, 4-way sum 6.84 -> 6.59 us for dropping bit 2 alone).
// Bit 3: partial vectors (the extent of a vector axis is not a multiple of V: the last vector of a row is moved element by element).
// Instantiated: 0 (plain), 1 (plain + bounds checks on edge tiles), 9 (1 + partial vectors), 2 (orbit order), 7 (everything).
template <class T, class F, bool MIXED, bool WIDE, int V, int MODE, int THRLOG>
SMR_DEV void tiled_map_body(const TiledArgs<WIDE> a, F f) {
    constexpr bool EDGE = (MODE & 1) != 0;
    constexpr bool ORD = (MODE & 2) != 0;
    constexpr bool GENORG = (MODE & 4) != 0;
    constexpr bool PV = (MODE & 8) != 0 || MODE == 7;  // partial vectors at the end of a row (extent of a vector axis not a multiple of V)
    typedef typename off_t_of<WIDE>::type O;
    typedef TVec<T, V> VT;
    typedef TUVec<T, V> GT;  // the same vector in global memory
    constexpr int VLOG = (V == 1) ? 0 : (V == 2 ? 1 : 2);
    constexpr int NREP = EPL / V;
    constexpr int NT = 1 << THRLOG;
    constexpr int NIN_STATIC = F::NIN;
    constexpr int NINMAX = (NIN_STATIC >= 0) ? NIN_STATIC : MAXIN;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* lds = reinterpret_cast<T*>(smem_raw);
    const int nin = (NIN_STATIC >= 0) ? NIN_STATIC : a.M - 1;
    const uint32_t tid = threadIdx.x;

    // ---- per-lane rows (byte offset + swizzled LDS index of the lane's first element, per operand) ----
    // tables in device memory: the first memory instructions of the kernel
    LaneRow<WIDE> row[NINMAX + 1];
#pragma unroll
    for (int k = 0; k <= NINMAX; ++k) {
        row[k].g = 0;
        row[k].l = 0;
        if (k <= nin) row[k] = a.lanetab[k * NT + tid];
    }

    // ---- which tile ---------------------------------------------------------------------------------
    uint32_t b = blockIdx.x + a.blk0;
    if constexpr (ORD) {
        // locality-aware tile order (smr_plan_tiled.cpp: plan_tile_order).  The in-kernarg lookup is
        // issued unconditionally so that it travels with the first batch of scalar loads.
        const uint32_t pair = a.ord16[(b & (NORD16 - 1)) >> 1];
        if (a.ordmode == 1) {
            const uint32_t v = (b & 1u) ? (pair >> 16) : (pair & 0xffffu);
            b = (v == 0xffffu) ? 0xffffffffu : v;
        } else if (a.ordmode == 2) {
            b = a.ordtab[b];
        }
        if (b == 0xffffffffu) return;  // padding workgroup (whole workgroup: no barrier is skipped)
    }
    uint32_t tc[MAXN];
#pragma unroll
    for (int g = 0; g < NG; ++g) {  // unused grid dims are padded with ntiles = 1
        const uint32_t q = fastdiv(b, a.div_m[g], a.div_s[g]);
        tc[g] = b - q * a.ntiles[g];
        b = q;
    }
    if constexpr (EDGE && !GENORG) {
        // ragged grid dims run slowest and backwards: the workgroups of the partly filled last tiles -- the ones with bounds code on
        // their path -- are the FIRST to start, and their longer lives end with everybody else's instead of after them
        const uint32_t fl = a.gflip;
#pragma unroll
        for (int g = 0; g < NG; ++g)
            if ((fl >> g) & 1u) tc[g] = a.ntiles[g] - 1u - tc[g];
    }
#pragma unroll
    for (int g = NG; g < MAXN; ++g) tc[g] = 0;
    if (GENORG && a.ng > NG) {
#pragma unroll
        for (int g = NG; g < MAXN; ++g) {
            const uint32_t q = fastdiv(b, a.div_m[g], a.div_s[g]);
            tc[g] = b - q * a.ntiles[g];
            b = q;
        }
    }
    // EDGE = false is instantiated for problems without any ragged dim: no bounds code at all
    // (code size is part of the latency of a ~4 us launch)
    bool edge = false;
    uint32_t lim[MAXT];
#pragma unroll
    for (int j = 0; j < MAXT; ++j) lim[j] = 0x7fffffffu;
    // Everything the bounds checks need from the kernel arguments is fetched HERE, unconditionally, with the first batch of scalar
    // loads (round 6).  Fetched where it was used -- inside `if (edge)` -- it was a chain of ~15 dependent scalar-memory round trips
    // in the workgroups of a ragged last tile, 1-2 us each: they finished that much after everybody else and set the launch's span
    // (transposes of 7200 x 100 Float64: 4.4 us against 3.0 us for 7200 x 128, with a quarter of the workgroups nearly empty).
    constexpr int KP = (NINMAX < 3 ? NINMAX : 3) + 1;  // operands whose enumeration shifts are pinned (destination + up to 3 inputs)
    int gj[MAXT];
    uint32_t ntm1[MAXT], lastn[MAXT], tlg[MAXT], eshp[KP][MAXT];
    if constexpr (EDGE) {
#pragma unroll
        for (int j = 0; j < MAXT; ++j) {
            gj[j] = __builtin_amdgcn_readfirstlane(a.ej_g[j]);
            ntm1[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ej_ntm1[j]);
            lastn[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ej_last[j]);
            tlg[j] = (uint32_t)__builtin_amdgcn_readfirstlane(a.tlog[j]);
            asm volatile("" : "+s"(gj[j]), "+s"(ntm1[j]), "+s"(lastn[j]), "+s"(tlg[j]));
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                eshp[k][j] = (uint32_t)__builtin_amdgcn_readfirstlane(a.esh[k][j]);
                asm volatile("" : "+s"(eshp[k][j]));
            }
        }
        uint32_t emin = 0xffffffffu;  // 0 iff some grid coordinate sits on a ragged last tile
#pragma unroll
        for (int g = 0; g < MAXN; ++g)
            if (g < NG || (GENORG && a.ng > NG)) emin = min(emin, tc[g] ^ a.last_ragged[g]);
        edge = emin == 0;
        if (edge) {
#pragma unroll
            for (int j = 0; j < MAXT; ++j) {
                uint32_t t = 0xffffffffu;
#pragma unroll
                for (int gg = 0; gg < MAXN; ++gg)
                    if (gg == gj[j]) t = tc[gg];
                if (gj[j] >= 0 && t == ntm1[j]) lim[j] = lastn[j];
            }
        }
    }
    const int ntd = a.nt;
    // how many of the V elements e .. e + V - 1 of operand k's enumeration lie inside the array (they differ in the coordinate at
    // bit 0): V or 0, or -- extent of the vector axis not a multiple of V -- something between in the last vector of a row
    auto in_count = [&](int k, uint32_t e) -> uint32_t {
        uint32_t cnt = V;
#pragma unroll
        for (int j = 0; j < MAXT; ++j)
            if (j < ntd) {
                uint32_t sh = 0, tl = 0;
                if constexpr (EDGE) {
                    tl = tlg[j];
                    sh = (uint32_t)a.esh[k][j];
#pragma unroll
                    for (int kk = 0; kk < KP; ++kk)
                        if (kk == k) sh = eshp[kk][j];
                }
                const uint32_t cj = (e >> sh) & ((1u << tl) - 1u);
                if (cj >= lim[j]) cnt = 0;
                else if (PV && V > 1 && sh == 0) cnt = min(cnt, lim[j] - cj);
            }
        return cnt;
    };
    auto tile_base = [&](int k) -> char* {
        if (!GENORG || a.base32) {  // every tile origin of every operand is below 4 GiB, steps non-negative
            uint32_t o = 0;
#pragma unroll
            for (int g = 0; g < NG; ++g) o += tc[g] * a.op[k].tstep32[g];
            return (char*)a.op[k].base + o;
        }
        i64 o = 0;
#pragma unroll
        for (int g = 0; g < MAXN; ++g)
            if (g < NG || a.ng > NG) o += (i64)tc[g] * a.tstep[k][g];
        return (char*)a.op[k].base + o;
    };

    // The body below exists twice in the bounds-checking variants (round 6): a workgroup of whole tiles runs the copy WITHOUT any
    // bounds code (EDG = false) -- the ~90 extra instructions in front of its loads were 0.3 us per launch on whole tiles --, a
    // workgroup on a ragged last tile the checked one.  `edge` is uniform over the workgroup: both copies keep their barrier.
    auto body = [&](auto edge_c) {
        constexpr bool EDG = EDGE && decltype(edge_c)::value;
        // ---- phase A: issue EVERY global load of the tile before anything waits ------------------------
        VT x[NINMAX > 0 ? NINMAX : 1][NREP];
        uint32_t cnl[NINMAX > 0 ? NINMAX : 1][NREP];  // valid elements of input i's repeat r in ITS order (bounds-checking vector variants)
        uint32_t cntd[NREP];  // valid elements of repeat r in destination order (edge tiles: 0 .. V)
    #pragma unroll
        for (int r = 0; r < NREP; ++r) {
            cntd[r] = V;
            if constexpr (EDG) cntd[r] = in_count(0, (((uint32_t)r << THRLOG) | tid) << VLOG);
        }
    #pragma unroll
        for (int i = 0; i < NINMAX; ++i) {
    #pragma unroll
            for (int r = 0; r < NREP; ++r)
    #pragma unroll
                for (int h = 0; h < V; ++h) x[i][r].v[h] = T{};
            if (i < nin) {
                const OpDesc<WIDE>& d = a.op[i + 1];
                const char* bp = tile_base(i + 1);
                const bool stg = a.staged[i + 1] >= 0;
    #pragma unroll
                for (int r = 0; r < NREP; ++r) {
                    uint32_t cn = cntd[r];
                    if (EDG && stg) cn = in_count(i + 1, (((uint32_t)r << THRLOG) | tid) << VLOG);
                    if constexpr (EDG && V > 1) {
                        // Bounds-checking vector variant: the load itself is UNCONDITIONAL -- a lane outside the array reads the operand's
                        // first vector (always there: the launcher requires an extent of at least V along the vector axis) and drops it.
                        // Guarded by a branch per load, the compiler put an s_waitcnt vmcnt(0) in front of every one of them: a tile's
                        // loads went out one memory round trip after the other, in EVERY workgroup of a ragged problem (+0.5 us on whole
                        // tiles, profiles/r06_ragged_tiles.txt).  Partial vectors are patched up below, after all loads have been issued.
                        const bool full = cn == (uint32_t)V;
                        const char* p = full ? bp + (O)(row[i + 1].g + d.Gr[r]) : (const char*)d.base;
                        const GT gv = *reinterpret_cast<const GT*>(p);
    #pragma unroll
                        for (int h = 0; h < V; ++h) x[i][r].v[h] = gv.v[h];  // (nothing may USE the value here: the next load must leave first;
                        cnl[i][r] = cn;                                       //  what a lane outside the array holds is never stored)
                    } else if (cn) {
                        const char* p = bp + (O)(row[i + 1].g + d.Gr[r]);
                        if constexpr (V == 1) {
                            x[i][r].v[0] = load_at<T, MIXED>(p, d.dtype, d.conj);
                        } else {
    #if SMR_TILED_NTL == 2  // experiment (A/B build): system-scope loads (sc0 sc1: served below the L2, which keeps its contents)
                            {
                                constexpr int NQ = (int)(sizeof(VT) / 8);
                                uint64_t qw[NQ > 0 ? NQ : 1];
    #pragma unroll
                                for (int w = 0; w < NQ; ++w)
                                    qw[w] = __hip_atomic_load(reinterpret_cast<const uint64_t*>(p) + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                __builtin_memcpy(&x[i][r], qw, sizeof(VT));
                            }
    #elif SMR_TILED_NTL  // experiment (A/B build): non-temporal loads
                            x[i][r] = load_vec_ct<true, VT>(p);
    #else
                            {
                                const GT gv = *reinterpret_cast<const GT*>(p);
    #pragma unroll
                                for (int h = 0; h < V; ++h) x[i][r].v[h] = gv.v[h];
                            }
    #endif
                            if constexpr (tr<T>::cx) {
                                if (d.conj) {
    #pragma unroll
                                    for (int h = 0; h < V; ++h) x[i][r].v[h] = cj(x[i][r].v[h]);
                                }
                            }
                        }
                    }
                }
            }
        }
        if constexpr (EDG && V > 1 && tr<T>::cx) {  // conjugated inputs of the bounds-checking vector variants: behind all loads
    #pragma unroll
            for (int i = 0; i < NINMAX; ++i)
                if (i < nin && a.op[i + 1].conj) {
    #pragma unroll
                    for (int r = 0; r < NREP; ++r)
    #pragma unroll
                        for (int h = 0; h < V; ++h) x[i][r].v[h] = cj(x[i][r].v[h]);
                }
        }
        if constexpr (EDG && PV && V > 1) {  // the partial vector at the end of a row: element by element, behind the vector loads
    #pragma unroll
            for (int i = 0; i < NINMAX; ++i)
                if (i < nin) {
                    const OpDesc<WIDE>& d = a.op[i + 1];
                    const char* bp = tile_base(i + 1);
    #pragma unroll
                    for (int r = 0; r < NREP; ++r)
                        if (cnl[i][r] > 0 && cnl[i][r] < (uint32_t)V) {
                            const char* p = bp + (O)(row[i + 1].g + d.Gr[r]);
    #pragma unroll
                            for (int h = 0; h < V; ++h)
                                if ((uint32_t)h < cnl[i][r]) x[i][r].v[h] = load_at<T, MIXED>(p + h * sizeof(T), d.dtype, d.conj);
                        }
                }
        }
        char* bp0 = tile_base(0);

        // ---- phase B: staged inputs -> LDS, destination order, XOR-swizzled -----------------------------
    #pragma unroll
        for (int i = 0; i < NINMAX; ++i) {
            if (i < nin && a.staged[i + 1] >= 0) {
                const OpDesc<WIDE>& d = a.op[i + 1];
                T* L = lds + ((size_t)a.staged[i + 1] << a.tilelog);
    #pragma unroll
                for (int r = 0; r < NREP; ++r) {
                    bool ok = true;
                    if constexpr (EDG && !(V > 1)) {  // (the vector variants park every lane's vector: a lane outside the array owns its own LDS slots)
                        ok = in_count(i + 1, (((uint32_t)r << THRLOG) | tid) << VLOG) > 0;
                    }
                    if (ok) {
    #pragma unroll
                        for (int h = 0; h < V; ++h) L[row[i + 1].l ^ d.Lr[r] ^ d.Lh[h]] = x[i][r].v[h];
                    }
                }
            }
        }
        __syncthreads();

        // ---- phase C: read back in destination order, apply f, store ---------------------------------------
    #pragma unroll
        for (int i = 0; i < NINMAX; ++i) {
            if (i < nin && a.staged[i + 1] >= 0) {
                const T* L = lds + ((size_t)a.staged[i + 1] << a.tilelog);
    #pragma unroll
                for (int r = 0; r < NREP; ++r) {
                    if ((EDG && V > 1) || cntd[r]) {
    #pragma unroll
                        for (int h = 0; h < V; ++h) x[i][r].v[h] = L[row[0].l ^ a.Lrd[r] ^ a.Lhd[h]];
                    }
                }
            }
        }
        VT out[NREP];
    #pragma unroll
        for (int r = 0; r < NREP; ++r) {
            if ((EDG && V > 1) || cntd[r]) {
    #pragma unroll
                for (int h = 0; h < V; ++h) {
                    T arg[MAXIN];
    #pragma unroll
                    for (int i = 0; i < MAXIN; ++i) {
                        arg[i] = T{};
                        if (i < NINMAX) arg[i] = x[i < NINMAX ? i : 0][r].v[h];
                    }
                    out[r].v[h] = f(arg);
                }
                if constexpr (V == 1) {
                    store_at<T, MIXED>(bp0 + (O)(row[0].g + a.op[0].Gr[r]), a.op[0].dtype, a.op[0].conj, out[r].v[0]);
                } else {
                    if constexpr (tr<T>::cx) {
                        if (a.op[0].conj) {
    #pragma unroll
                            for (int h = 0; h < V; ++h) out[r].v[h] = cj(out[r].v[h]);
                        }
                    }
                }
            }
        }
        if constexpr (V > 1) {
            // one wave-uniform branch around all vector stores (see smr_device.h:store_vec)
            auto put = [&](auto NT) {
    #pragma unroll
                for (int r = 0; r < NREP; ++r)
                    if (cntd[r] == (uint32_t)V) {
                        GT gv;
    #pragma unroll
                        for (int h = 0; h < V; ++h) gv.v[h] = out[r].v[h];
                        store_vec_ct<decltype(NT)::value, GT>(bp0 + (O)(row[0].g + a.op[0].Gr[r]), gv);
                    }
            };
            // the partial vector at the end of a row (edge tiles, extent of the vector axis not a multiple of V): element by element
            auto put_partial_vecs = [&](auto WT) {
                if constexpr (EDG && PV) {
    #pragma unroll
                    for (int r = 0; r < NREP; ++r)
                        if (cntd[r] > 0 && cntd[r] < (uint32_t)V) {
    #pragma unroll
                            for (int h = 0; h < V; ++h)
                                if ((uint32_t)h < cntd[r]) {
                                    char* p = bp0 + (O)(row[0].g + a.op[0].Gr[r]) + h * sizeof(T);
                                    if constexpr (decltype(WT)::value) {
                                        TVec<T, 1> one;
                                        one.v[0] = out[r].v[h];
                                        store_vec_wt<TVec<T, 1>>(p, one);
                                    } else {
                                        *reinterpret_cast<T*>(p) = out[r].v[h];
                                    }
                                }
                        }
                }
            };
            if (a.nts == 2) {  // agent-scope write-through ("self-released" launch: smr_device.h)
                if constexpr (has_wt_store<VT>::value) {
    #pragma unroll
                    for (int r = 0; r < NREP; ++r)
                        if (cntd[r] == (uint32_t)V) store_vec_wt<VT>(bp0 + (O)(row[0].g + a.op[0].Gr[r]), out[r]);
                    if constexpr (has_wt_store<TVec<T, 1>>::value) put_partial_vecs(BoolC<true>{});
                    self_release_wait();
                }
            } else if (a.nts) {
                nt_block_guard();
                put(BoolC<true>{});
                nt_block_guard();
                put_partial_vecs(BoolC<false>{});
            } else {
                put(BoolC<false>{});
                put_partial_vecs(BoolC<false>{});
            }
        }
    };
    if constexpr (EDGE) {
        if (edge) body(BoolC<true>{});
        else body(BoolC<false>{});
    } else {
        body(BoolC<false>{});
    }
}


// ---- persistent, software-pipelined form ---------------------------------------------------------------
// For grids larger than the machine holds at once.  The classic form runs one tile per workgroup
// and its phases (table rows -> global loads -> LDS exchange -> stores) strictly one after the
// other; with one 1024-lane workgroup per CU nothing overlaps, and every workgroup re-reads its
// 40 KiB of lane-table rows (measured at 128^4: 24 % of all L2 read requests, 7.4 us per tile,
// 3 TB/s of HBM traffic).  Here a workgroup stays resident, reads its table rows ONCE and walks the
// work list with stride gridDim.x; the global loads of tile i+1 are issued right after tile i's
// staged values have gone to LDS, so they are in flight during tile i's LDS reads, f and stores.
// Only instantiated without bounds checks (no ragged tiled dim).
template <class T, class F, bool MIXED, bool WIDE, int V, int THRLOG>
SMR_DEV void tiled_map_pipe_body(const TiledArgs<WIDE> a, F f) {
    typedef typename off_t_of<WIDE>::type O;
    typedef TVec<T, V> VT;
    constexpr int NREP = EPL / V;
    constexpr int NT = 1 << THRLOG;
    constexpr int NIN_STATIC = F::NIN;
    constexpr int NINMAX = (NIN_STATIC >= 0) ? NIN_STATIC : MAXIN;
    constexpr int NX = NINMAX > 0 ? NINMAX : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* lds = reinterpret_cast<T*>(smem_raw);
    const int nin = (NIN_STATIC >= 0) ? NIN_STATIC : a.M - 1;
    const uint32_t tid = threadIdx.x;

    LaneRow<WIDE> row[NINMAX + 1];
#pragma unroll
    for (int k = 0; k <= NINMAX; ++k) {
        row[k].g = 0;
        row[k].l = 0;
        if (k <= nin) row[k] = a.lanetab[k * NT + tid];
    }

    // work-list entry -> tile id (0xffffffff: none, and none after it for this workgroup)
    auto tile_of = [&](uint32_t e) -> uint32_t {
        if (e >= (uint32_t)a.nwork) return 0xffffffffu;
        return a.ordmode == 2 ? a.ordtab[e] : e;
    };
    // tile id -> per-operand tile origins
    auto origins = [&](uint32_t b, char* (&bp)[NINMAX + 1]) {
        uint32_t tc[MAXN];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const uint32_t q = fastdiv(b, a.div_m[g], a.div_s[g]);
            tc[g] = b - q * a.ntiles[g];
            b = q;
        }
#pragma unroll
        for (int g = NG; g < MAXN; ++g) tc[g] = 0;
        if (a.ng > NG) {
#pragma unroll
            for (int g = NG; g < MAXN; ++g) {
                const uint32_t q = fastdiv(b, a.div_m[g], a.div_s[g]);
                tc[g] = b - q * a.ntiles[g];
                b = q;
            }
        }
#pragma unroll
        for (int k = 0; k <= NINMAX; ++k) {
            bp[k] = nullptr;
            if (k <= nin) {
                if (a.base32) {
                    uint32_t o = 0;
#pragma unroll
                    for (int g = 0; g < NG; ++g) o += tc[g] * a.op[k].tstep32[g];
                    bp[k] = (char*)a.op[k].base + o;
                } else {
                    i64 o = 0;
#pragma unroll
                    for (int g = 0; g < MAXN; ++g)
                        if (g < NG || a.ng > NG) o += (i64)tc[g] * a.tstep[k][g];
                    bp[k] = (char*)a.op[k].base + o;
                }
            }
        }
    };
    auto issue_loads = [&](char* const (&bp)[NINMAX + 1], VT (&x)[NX][NREP]) {
#pragma unroll
        for (int i = 0; i < NINMAX; ++i) {
            if (i < nin) {
                const OpDesc<WIDE>& d = a.op[i + 1];
#pragma unroll
                for (int r = 0; r < NREP; ++r) {
                    const char* p = bp[i + 1] + (O)(row[i + 1].g + d.Gr[r]);
                    if constexpr (V == 1) {
                        x[i][r].v[0] = load_at<T, MIXED>(p, d.dtype, d.conj);
                    } else {
                        x[i][r] = *reinterpret_cast<const VT*>(p);
                        if constexpr (tr<T>::cx) {
                            if (d.conj) {
#pragma unroll
                                for (int h = 0; h < V; ++h) x[i][r].v[h] = cj(x[i][r].v[h]);
                            }
                        }
                    }
                }
            }
        }
    };

    uint32_t e = blockIdx.x;
    uint32_t tile = tile_of(e);
    if (tile == 0xffffffffu) return;
    char* bp[NINMAX + 1];
    VT x[NX][NREP], xn[NX][NREP];
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int r = 0; r < NREP; ++r)
#pragma unroll
            for (int h = 0; h < V; ++h) {
                x[i][r].v[h] = T{};
                xn[i][r].v[h] = T{};
            }
    origins(tile, bp);
    issue_loads(bp, x);
    while (true) {
        char* const bp0 = bp[0];
        // staged inputs of the current tile -> LDS (destination order, swizzled)
#pragma unroll
        for (int i = 0; i < NINMAX; ++i) {
            if (i < nin && a.staged[i + 1] >= 0) {
                const OpDesc<WIDE>& d = a.op[i + 1];
                T* L = lds + ((size_t)a.staged[i + 1] << a.tilelog);
#pragma unroll
                for (int r = 0; r < NREP; ++r)
#pragma unroll
                    for (int h = 0; h < V; ++h) L[row[i + 1].l ^ d.Lr[r] ^ d.Lh[h]] = x[i][r].v[h];
            }
        }
        __syncthreads();
        // next tile: its loads fly while this one is finished
        e += gridDim.x;
        const uint32_t next = tile_of(e);
        const bool more = next != 0xffffffffu;
        if (more) {
            origins(next, bp);
            issue_loads(bp, xn);
        }
        // current tile: LDS -> registers (destination order), f, store
#pragma unroll
        for (int i = 0; i < NINMAX; ++i) {
            if (i < nin && a.staged[i + 1] >= 0) {
                const T* L = lds + ((size_t)a.staged[i + 1] << a.tilelog);
#pragma unroll
                for (int r = 0; r < NREP; ++r)
#pragma unroll
                    for (int h = 0; h < V; ++h) x[i][r].v[h] = L[row[0].l ^ a.Lrd[r] ^ a.Lhd[h]];
            }
        }
#pragma unroll
        for (int r = 0; r < NREP; ++r) {
            VT out;
#pragma unroll
            for (int h = 0; h < V; ++h) {
                T arg[MAXIN];
#pragma unroll
                for (int i = 0; i < MAXIN; ++i) {
                    arg[i] = T{};
                    if (i < NINMAX) arg[i] = x[i < NINMAX ? i : 0][r].v[h];
                }
                out.v[h] = f(arg);
            }
            char* p = bp0 + (O)(row[0].g + a.op[0].Gr[r]);
            if constexpr (V == 1) {
                store_at<T, MIXED>(p, a.op[0].dtype, a.op[0].conj, out.v[0]);
            } else {
                if constexpr (tr<T>::cx) {
                    if (a.op[0].conj) {
#pragma unroll
                        for (int h = 0; h < V; ++h) out.v[h] = cj(out.v[h]);
                    }
                }
                store_vec<VT>(p, out, a.nts);
            }
        }
        if (!more) break;
        __syncthreads();  // every lane has read its LDS values before the next tile overwrites them
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int r = 0; r < NREP; ++r) x[i][r] = xn[i][r];
    }
}

#ifndef SMR_JIT
template <class T, class F, bool MIXED, bool WIDE, int V, int MODE, int THRLOG>
__global__ void __launch_bounds__(1 << THRLOG) k_tiled_map(const TiledArgs<WIDE> a, F f SMR_STAMP_PARAM) {
    SMR_STAMP_BEGIN
    tiled_map_body<T, F, MIXED, WIDE, V, MODE, THRLOG>(a, f);
    SMR_STAMP_END
}

template <class T, class F, bool MIXED, bool WIDE, int V, int THRLOG>
__global__ void __launch_bounds__(1 << THRLOG) k_tiled_map_pipe(const TiledArgs<WIDE> a, F f SMR_STAMP_PARAM) {
    SMR_STAMP_BEGIN
    tiled_map_pipe_body<T, F, MIXED, WIDE, V, THRLOG>(a, f);
    SMR_STAMP_END
}

template <class T, class F, bool MIXED, bool WIDE, int V, int MODE, int THRLOG>
static int go3e(const Plan& plan, hipStream_t s, F f, const OpTab& tab, const TiledVariant& tv) {
    TiledLaunch<WIDE> L;
    constexpr bool wt_store = V > 1 && !MIXED && has_wt_store<TVec<T, V>>::value;
    if (int rc = tiled_launch_args<WIDE>(plan, tab.base, (int)sizeof(T), tv, wt_store, L)) return rc;
    const TiledArgs<WIDE>& ka = L.a;
    const unsigned block = 1u << THRLOG;
    auto launch = [&]() -> int {
        if constexpr (is_jit<F>::value) {
            const char* argtype = WIDE ? "smr::TiledArgs<true>" : "smr::TiledArgs<false>";
            if (L.pgrid) return launch_jit<T>(plan.c, s, "tiled", argtype, "tiled_map_pipe_body", "", L.pgrid, block, L.lds, ka, MIXED, WIDE, V, THRLOG);
            return launch_jit<T>(plan.c, s, "tiled", argtype, "tiled_map_body", "", L.grid, block, L.lds, ka, MIXED, WIDE, V, MODE, THRLOG);
        } else {
            if constexpr ((MODE & 1) == 0) {
                if (L.pgrid) {
                    auto kern = k_tiled_map_pipe<T, F, MIXED, WIDE, V, THRLOG>;
                    return launch_native((const void*)kern, L.lds, "k_tiled_map_pipe",
                                         [&] { SMR_LAUNCH(kern, dim3(L.pgrid), dim3(block), L.lds, s, ka, f SMR_STAMP_ARG(L.pgrid, block)); });
                }
            }
            auto kern = k_tiled_map<T, F, MIXED, WIDE, V, MODE, THRLOG>;
            return launch_native((const void*)kern, L.lds, "k_tiled_map", [&] {
                mark_sliceable(1, (unsigned)offsetof(TiledArgs<WIDE>, blk0), 0);  // a workgroup owns its tile: block ranges are independent
                if (ka.nts == 2) mark_self_released();
                SMR_LAUNCH(kern, dim3(L.grid), dim3(block), L.lds, s, ka, f SMR_STAMP_ARG(L.grid, block));
            });
        }
    };
    return launch();
}

// The kernel of tiled_variant()'s choice (smr_plan_tiled.cpp): MODE here, 64-bit offsets, vector width and threads in go_tl and go.
template <class T, class F, bool MIXED, bool WIDE, int V, int THRLOG>
static int go3(const Plan& plan, hipStream_t s, F f, const OpTab& tab, const TiledVariant& tv) {
    if constexpr (V > 1) {
        if (tv.mode == 9) return go3e<T, F, MIXED, WIDE, V, 9, THRLOG>(plan, s, f, tab, tv);
    }
    if (tv.mode == 1) return go3e<T, F, MIXED, WIDE, V, 1, THRLOG>(plan, s, f, tab, tv);
    if (tv.mode == 7) return go3e<T, F, MIXED, WIDE, V, 7, THRLOG>(plan, s, f, tab, tv);
    if (tv.mode == 2) return go3e<T, F, MIXED, WIDE, V, 2, THRLOG>(plan, s, f, tab, tv);
    if (tv.mode == 0) return go3e<T, F, MIXED, WIDE, V, 0, THRLOG>(plan, s, f, tab, tv);
    return set_error(SMR_EINVAL, "tiled: no kernel of this MODE");
}

template <class T, class F, bool MIXED, int THRLOG>
static int go_tl(const Plan& plan, hipStream_t s, F f, const OpTab& tab, const TiledVariant& tv) {
    if (tv.wide) return go3<T, F, MIXED, true, 1, THRLOG>(plan, s, f, tab, tv);
    if constexpr (!MIXED && sizeof(T) < 16) {
        // a lane's 4 elements as 16-byte vectors (8-byte for 1/2-byte element types)
        constexpr int VMAX = (16 / sizeof(T)) > 4 ? 4 : (int)(16 / sizeof(T));
        if (tv.V == VMAX) return go3<T, F, false, false, VMAX, THRLOG>(plan, s, f, tab, tv);
    }
    if (tv.V != 1) return set_error(SMR_EINVAL, "tiled: no kernel of this vector width");
    return go3<T, F, MIXED, false, 1, THRLOG>(plan, s, f, tab, tv);
}

// ---- XPOSE: the lean form of an HBM-sized transposing copy (round 5) -------------------------------------------------------------
// One staged input, 128 x 32 tiles, every tiled extent a whole number of tiles, 16-byte accesses: permutedims! / adjoint! / copy! of
// a permuted view / B .= c .* A' on arrays of 1 GiB and more.  The general kernel above carries lane tables (16 KiB of table rows per
// 1024-lane workgroup: a quarter more L2 read requests than the payload), swizzle masks, tile-order lookups and edge code through its
// prologue; at 65536 workgroups per launch that is 8 % of the run time (tools/xpose_proto.hip: 723 us against 782 us for the same
// tile shape and grid order at 128^4 Float64).  Here the lane's place in the tile is two integer divisions of its id, the tile's
// origin a handful of divisions of the workgroup id, every load of the tile is issued before the first LDS write, the LDS rows
// carry a pitch of TQ + 2 elements, stores are non-temporal.  Grid order = TilePlan::gorder.
struct XposeArgs {
    const char* src;
    char* dst;
    int32_t ng, pad;
    uint32_t ext[MAXN];     // extent of grid coordinate g (fastest first)
    i64 sstep[MAXN];        // byte step of the input / the destination per unit of grid coordinate g
    i64 dstep[MAXN];
    i64 src_row, dst_row;   // byte stride of the input along the destination's unit dim / of the destination along the input's unit dim
};

template <class T, class F, int V, int T0, int TQ>
__global__ void __launch_bounds__(1024) k_xpose_big(const XposeArgs a, F f) {
    typedef TVec<T, V> VT;
    constexpr int PITCH = TQ + 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_x[];
    T* lds = reinterpret_cast<T*>(smem_x);
    uint32_t b = blockIdx.x;
    i64 so = 0, dofs = 0;
#pragma unroll 1
    for (int g = 0; g < a.ng; ++g) {
        const uint32_t q = b / a.ext[g], r = b - q * a.ext[g];
        so += (i64)r * a.sstep[g];
        dofs += (i64)r * a.dstep[g];
        b = q;
    }
    const char* s0 = a.src + so;
    char* d0 = a.dst + dofs;
    const int tid = threadIdx.x;
    // load: lanes along the input's unit axis (TQ / V lanes per row), rows along the destination's unit dim
    constexpr int LPR = TQ / V, RPP = 1024 / LPR, NPASS = T0 / RPP;
    const int lc = tid % LPR, lr = tid / LPR;
    VT x[NPASS];
#pragma unroll
    for (int p = 0; p < NPASS; ++p) x[p] = *reinterpret_cast<const VT*>(s0 + (i64)(p * RPP + lr) * a.src_row + (i64)lc * (V * (int)sizeof(T)));
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        T* L = lds + (size_t)(p * RPP + lr) * PITCH + V * lc;  // row = position along the destination's unit dim
#pragma unroll
        for (int h = 0; h < V; ++h) L[h] = x[p].v[h];
    }
    __syncthreads();
    // store: lanes along the destination's unit dim (T0 / V lanes per row), rows along the input's unit axis
    constexpr int LPR2 = T0 / V, RPP2 = 1024 / LPR2, NPASS2 = TQ / RPP2;
    const int sc = tid % LPR2, sr = tid / LPR2;
#pragma unroll
    for (int p = 0; p < NPASS2; ++p) {
        const int iq = p * RPP2 + sr;
        VT out;
#pragma unroll
        for (int h = 0; h < V; ++h) {
            T arg[MAXIN];
#pragma unroll
            for (int i = 0; i < MAXIN; ++i) arg[i] = T{};
            arg[0] = lds[(size_t)(V * sc + h) * PITCH + iq];
            out.v[h] = f(arg);
        }
        store_vec_ct<true, VT>(d0 + (i64)iq * a.dst_row + (i64)sc * (V * (int)sizeof(T)), out);
    }
}

// SMR_OK: launched; SMR_EUNSUPPORTED (no error text set): not this case, the caller takes the general kernel
template <class T, class F>
static int try_xpose_big(const Plan& plan, hipStream_t s, F f, const OpTab& tab) {
    const Canon& c = plan.c;
    const TilePlan& t = plan.tile;
    constexpr int V = 16 / (int)sizeof(T) >= 1 ? 16 / (int)sizeof(T) : 1;
    constexpr int T0 = 128, TQ = 32;
    if constexpr (is_jit<F>::value || !tr<T>::arith || sizeof(T) < 8 || (F::NIN >= 0 && F::NIN != 1)) {
        return SMR_EUNSUPPORTED;
    } else {
        if (!options().tiled_xpose) return SMR_EUNSUPPORTED;
        // (rank 2 -- a plain matrix transpose, or a permutation that fuses to one -- stays with the general kernel: 16384^2 700 vs 708 us)
        if (c.M != 2 || c.mixed || c.N < 3 || c.N > MAXN || t.nt != 2 || t.tilelog != 12 || t.staged[1] < 0 || !t.ord.empty()) return SMR_EUNSUPPORTED;
        if (t.tdim[0] != 0 || t.tlog[0] != 7 || t.tlog[1] != 5) return SMR_EUNSUPPORTED;
        const int q = t.tdim[1];
        if (c.strides[0][0] != 1 || c.strides[1][q] != 1 || c.dims[0] % T0 || c.dims[q] % TQ) return SMR_EUNSUPPORTED;
        if (tab.conj[0] || tab.conj[1]) return SMR_EUNSUPPORTED;
        if (c.algbytes < ((i64)512 << 20)) return SMR_EUNSUPPORTED;
        const i64 es = (i64)sizeof(T);
        if ((((uintptr_t)tab.base[0]) | ((uintptr_t)tab.base[1])) % 16) return SMR_EUNSUPPORTED;
        for (int d = 0; d < c.N; ++d) {
            if (d != 0 && (c.strides[0][d] * es) % 16) return SMR_EUNSUPPORTED;
            if (d != q && (c.strides[1][d] * es) % 16) return SMR_EUNSUPPORTED;
        }
        XposeArgs a;
        std::memset(&a, 0, sizeof a);
        a.src = (const char*)tab.base[1];
        a.dst = (char*)tab.base[0];
        a.src_row = c.strides[1][0] * es;
        a.dst_row = c.strides[0][q] * es;
        i64 grid = 1;
        int ng = 0;
        for (int i = 0; i < c.N; ++i) {
            const int d = t.gorder[i] >= 0 && t.gorder[i] < c.N ? t.gorder[i] : -1;
            if (d < 0) return SMR_EUNSUPPORTED;
            const i64 tile = d == 0 ? T0 : (d == q ? TQ : 1);
            const i64 n = c.dims[d] / tile;
            if (n <= 1) continue;
            if (n > 0xffffffffLL) return SMR_EUNSUPPORTED;
            a.ext[ng] = (uint32_t)n;
            a.sstep[ng] = c.strides[1][d] * es * tile;
            a.dstep[ng] = c.strides[0][d] * es * tile;
            grid *= n;
            ++ng;
        }
        {   // gorder must be a permutation of the dims (every dim with more than one tile appears once)
            bool seen[MAXN] = {false};
            for (int i = 0; i < c.N; ++i) {
                if (seen[t.gorder[i]]) return SMR_EUNSUPPORTED;
                seen[t.gorder[i]] = true;
            }
        }
        a.ng = ng;
        if (grid < 1 || grid > 0x7fffffffLL) return SMR_EUNSUPPORTED;
        const size_t lds = (size_t)T0 * (TQ + 2) * sizeof(T);
        auto kern = k_xpose_big<T, F, V, T0, TQ>;
        return launch_native((const void*)kern, lds, "k_xpose_big", [&] { SMR_LAUNCH(kern, dim3((unsigned)grid), dim3(1024), lds, s, a, f); });
    }
}

template <class T, class F, bool MIXED>
static int go(const Plan& plan, void* const* bases, hipStream_t s, F f) {
    const Canon& c = plan.c;
    const TilePlan& t = plan.tile;
    const OpTab tab = make_optab(c, bases);
    if constexpr (!MIXED) {  // HBM-sized transposing copies: the lean form
        const int rc = try_xpose_big<T, F>(plan, s, f, tab);
        if (rc != SMR_EUNSUPPORTED) return rc;
    }
    if (t.tilelog != 10 && t.tilelog != 12) return set_error(SMR_EINVAL, "tiled: the planner must pick 1024- or 4096-element tiles");
    const TiledVariant tv = tiled_variant(plan, bases, (int)sizeof(T), MIXED);  // smr_plan_tiled.cpp: describe() prints the same choice
    if (tv.thrlog == 8) return go_tl<T, F, MIXED, 8>(plan, s, f, tab, tv);
    return go_tl<T, F, MIXED, 10>(plan, s, f, tab, tv);
}

template <>
int launch_tiled_map_ct<SMR_CT>(const Plan& plan, void* const* bases, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = plan.c;
    if (c.bitcopy) return with_bitcopy<SMR_CT>(c, [&](auto f) { return go<typename ident_elem<decltype(f)>::type, decltype(f), false>(plan, bases, s, f); });
    if (c.mixed) return with_prog<T>(c, [&](auto f) { return go<T, decltype(f), true>(plan, bases, s, f); });
    switch (c.fkind) {  // natively compiled functors of this family; everything else is compiled at run time
        case FK_IDENT: return go<T, FIdent<T>, false>(plan, bases, s, FIdent<T>{});
        case FK_ADD2: return go<T, FAdd2<T>, false>(plan, bases, s, FAdd2<T>{});
        case FK_ADD3: return go<T, FAdd3<T>, false>(plan, bases, s, FAdd3<T>{});
        case FK_ADD4: return go<T, FAdd4<T>, false>(plan, bases, s, FAdd4<T>{});
        case FK_SCALE: return go<T, FScale<T>, false>(plan, bases, s, FScale<T>{hostmk<T>(c.fc[0], c.fc[1])});
        case FK_SYM: return go<T, FSym<T>, false>(plan, bases, s, FSym<T>{hostmk<T>(c.fc[0], c.fc[1])});
        case FK_AXPY: return go<T, FAxpy<T>, false>(plan, bases, s, FAxpy<T>{hostmk<T>(c.fc[0], c.fc[1])});
        case FK_AXPBY:
            return go<T, FAxpby<T>, false>(plan, bases, s, FAxpby<T>{hostmk<T>(c.fc[0], c.fc[1]), hostmk<T>(c.fc[2], c.fc[3])});
        default: break;
    }
    return with_prog<T>(c, [&](auto f) { return go<T, decltype(f), false>(plan, bases, s, f); });
}
#endif  // !SMR_JIT

}  // namespace smr
