// smr_k_orbit.hip -- family ORBIT: fused N-ary map whose inputs are differently PERMUTED VIEWS OF ONE
// BUFFER (B .= (A .+ A')./2, the 4-way permuted sum of the reference's README, any symmetrisation).
//
// The classic tiled kernel (smr_k_tiled.hip) treats the views as independent operands: the buffer passes
// through L1 once per view, and with three or more distinct unit-stride axes most of those passes move
// 32-/64-byte runs.  Here the permutation group G the views generate (|G| <= 4) acts on the TILES: tile
// extents are equal along every cycle of G, so the image of a tile under g in G is again a tile.  A
// workgroup owns one orbit {g.t : g in G}:
//   * slot a of the LDS holds the buffer on tile g_a.t, loaded ONCE, in the buffer's natural order
//     (16 B per lane along the buffer's unit-stride axis -- every slot has the same shape, so one set
//     of per-lane offsets serves all of them);
//   * an output element of tile g_a.t reads view k from slot (pi_k o g_a) at the local coordinate
//     permuted by pi_k; the identity view comes straight from the lane's own registers;
//   * outputs leave in the same natural order (the destination has the identity view's strides).
// Every element of the buffer crosses L1 once instead of once per view, and an in-place update
// (destination = the buffer) is safe: an orbit is read completely before it is written, and orbits are
// disjoint.  Orbits are executed super-cell by super-cell in XCD-contiguous runs (smr_plan_orbit.cpp:
// plan_orbit), so the partner halves of 64-B runs meet in one XCD's L2.
// All index arithmetic is bit slicing of the lane id with kernel-argument shifts (no lane tables, no
// dependent memory round trip before the first global load).
// Measured on MI355X (4-way sum, Float64): 32^4 6.6 -> 4.7 us, 64^4 83 -> 46 us, 128^4 1.73 -> 1.41 ms
// (tools/c3_proto.hip is the design experiment this kernel follows).
// The kernel arguments (smr_orbit_args.h) are built once per plan by the device-free builders in smr_plan_orbit_args.cpp and cached
// (smr_api.cpp: orbit_launch_args sets the operand addresses, the store policy and the persistent grid per call); which kernel runs
// is orbit_variant()'s choice (smr_plan_orbit.cpp).  This file holds the kernels, the dispatch on that choice and the launches.
#include "smr_dispatch.h"
#include "smr_orbit_args.h"

#ifndef SMR_CT
#error "compile with -DSMR_CT=0..3 or 7"
#endif

namespace smr {

template <class T, int V>
struct alignas(sizeof(T) * V) OVec {
    T v[V];
};

// conjugate iff bit == 0x80000000, without a branch (sign flip of the imaginary part)
SMR_DEV float ocj(float x, uint32_t) { return x; }
SMR_DEV double ocj(double x, uint32_t) { return x; }
SMR_DEV c32 ocj(c32 x, uint32_t bit) { return c32{x.re, __uint_as_float(__float_as_uint(x.im) ^ bit)}; }
SMR_DEV c64 ocj(c64 x, uint32_t bit) {
    return c64{x.re, __longlong_as_double(__double_as_longlong(x.im) ^ ((long long)bit << 32))};
}

// LDS access by absolute 32-bit address (base of the dynamic segment included), element as one 4- / 8- / 16-byte word: lets a kernel
// form every address of the exchange BEFORE its barrier (left to the compiler, base and scaling are added behind it, in front of the reads)
template <int BYTES> struct lds_word;
template <> struct lds_word<4> { typedef uint32_t type; };
template <> struct lds_word<8> { typedef unsigned long long type; };
template <> struct lds_word<16> { typedef uint32_t type __attribute__((ext_vector_type(4))); };
template <class T>
SMR_DEV void lds_put(uint32_t addr, const T& v) {
    typedef typename lds_word<sizeof(T)>::type W;
    W w;
    __builtin_memcpy(&w, &v, sizeof(T));
    *(__attribute__((address_space(3))) W*)(uintptr_t)addr = w;
}
template <class T>
SMR_DEV T lds_get(uint32_t addr) {
    typedef typename lds_word<sizeof(T)>::type W;
    const W w = *(const __attribute__((address_space(3))) W*)(uintptr_t)addr;
    T v;
    __builtin_memcpy(&v, &w, sizeof(T));
    return v;
}

// NG = |G| (2 or 4; a group of order 3 is padded with a copy of slot 0), OWN0: view 0 is the identity view
// (its value is the lane's own register).  Apart from the rare > 4 grid dims there is no branch on a
// kernel argument before the stores: every scalar branch on a just-loaded argument is a serial
// scalar-cache round trip, and at 32^4 the whole launch lasts 4-5 us.
// PIPE: persistent form for orbits whose LDS footprint leaves one workgroup per CU -- the workgroup walks the
// list with stride gridDim.x (a multiple of 8: it stays on its XCD's run) and issues the loads of its next orbit
// right after the barrier, so that they fly during the exchange and the stores of the current one.
template <class T, class F, int V, int NREP, int NG, bool OWN0, bool PIPE = false>
SMR_DEV void orbit_map_body(const OrbitArgs a, const OrbitHead h, F f) {
    typedef OVec<T, V> VT;
    constexpr int NIN_STATIC = F::NIN;
    constexpr int NINMAX = (NIN_STATIC >= 0) ? NIN_STATIC : MAXIN;
    constexpr int NK = NINMAX > 0 ? NINMAX : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* lds = reinterpret_cast<T*>(smem_raw);
    const int nin = (NIN_STATIC >= 0) ? NIN_STATIC : a.nin;
    const uint32_t tid = threadIdx.x;
    // ---- slot origins: one wide scalar load of this workgroup's table row -----------------------------
    i64 org[NG];
    uint64_t smap;
    bool live;
    auto load_row = [&](uint32_t b, i64(&og)[NG], uint64_t& mp, bool& lv) {
        typedef uint32_t rowv __attribute__((ext_vector_type(2 * NG)));
        const rowv row = reinterpret_cast<const rowv*>(h.list)[b];
        uint32_t o32[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) o32[g] = row[g];
        mp = (uint64_t)row[NG] | ((uint64_t)row[NG + 1] << 32);
        // a padding workgroup (first word 0xffffffff) runs on slot origins 0 and only skips its stores: an early
        // exit here would keep every other kernel-argument load behind this row's round trip
        lv = o32[0] != 0xffffffffu;
#pragma unroll
        for (int g = 0; g < NG; ++g) og[g] = lv ? (i64)o32[g] * (i64)sizeof(T) : 0;
    };
    load_row(blockIdx.x, org, smap, live);

    // ---- per-lane byte offsets inside a tile + LDS read indices -----------------------------------------
    constexpr int NLR = NK - (OWN0 ? 1 : 0);      // views read from LDS
    uint32_t goff[NREP];
    uint32_t lr[NK][NREP];  // LDS index of the lane's first element seen through view k
    uint32_t cj[NREP][OMAXT];
#pragma unroll
    for (int r = 0; r < NREP; ++r) {
        const uint32_t e = (((uint32_t)r << h.ntlog) | tid) * V;
        uint32_t g = 0;
#pragma unroll
        for (int j = 0; j < OMAXT; ++j) {
            cj[r][j] = __builtin_amdgcn_ubfe(e, (h.eshp >> (8 * j)) & 0xffu, (h.elenp >> (8 * j)) & 0xffu);
            g += cj[r][j] * h.estride[j];
        }
        goff[r] = g;
    }

    // ---- load every slot (natural order) --------------------------------------------------------------
    VT x[NG][NREP];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < NREP; ++r) x[g][r] = *reinterpret_cast<const VT*>(h.src + org[g] + goff[r]);

    // ---- while the loads fly: everything the exchange needs from the kernel arguments ---------------
    // (left to itself the compiler sinks these scalar loads below the barrier: one more serial scalar-memory
    // round trip in a 5 us launch; the empty asm statements pin the values in registers here)
#pragma unroll
    for (int r = 0; r < NREP; ++r)
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            uint32_t l = 0;
            if (!(OWN0 && k == 0)) {
#pragma unroll
                for (int j = 0; j < OMAXT; ++j) l |= cj[r][j] << a.lsh[k][j];
            }
            lr[k][r] = l;
        }
    uint32_t swz_s1 = a.swz_s1, swz_s2 = a.swz_s2, swz_mask = a.swz_mask;
    asm volatile("" : "+s"(swz_s1), "+s"(swz_s2), "+s"(swz_mask));
    uint32_t sbase[NG][NK], hbit[NK], cbit[NK];
    uint32_t tilelog = (uint32_t)a.tilelog;
    asm volatile("" : "+s"(tilelog));
    // the LDS slot every (output slot, view) pair reads from: fields of this workgroup's row (orbits that share a workgroup have
    // their own little maps: smr_plan_orbit.cpp, plan_orbit)
    auto slot_bases = [&](uint64_t mp) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                sbase[g][k] = ((uint32_t)(mp >> ((g * 8 + k) * 2)) & 3u) << tilelog;
                asm volatile("" : "+s"(sbase[g][k]));
            }
    };
    slot_bases(smap);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        hbit[k] = (uint32_t)a.lsh[k][0];
        cbit[k] = a.conjbit[k];
        asm volatile("" : "+s"(hbit[k]), "+s"(cbit[k]));
#pragma unroll
        for (int r = 0; r < NREP; ++r) asm volatile("" : "+v"(lr[k][r]));
    }
    uint32_t conj0 = a.conj0 ? 0x80000000u : 0u, nts_flag = (uint32_t)a.nts;
    asm volatile("" : "+s"(conj0), "+s"(nts_flag));
    auto swz = [&](uint32_t i) { return i ^ (((i >> swz_s1) ^ (i >> swz_s2)) & swz_mask); };
    // one-shot form: the swizzled LDS indices of the lane's writes and of its transposing reads are formed HERE, while the global
    // loads fly (left alone the compiler computes them behind the barrier: ~45 vector instructions on the critical path of a
    // launch whose waves live 2 us).  The persistent form recomputes them per orbit (its registers hold two orbits).
    constexpr int NPRE = PIPE ? 1 : NREP;
    uint32_t wi[NPRE][V], ri[NK][NPRE][V];
    if constexpr (!PIPE) {
#pragma unroll
        for (int r = 0; r < NREP; ++r)
#pragma unroll
            for (int hh = 0; hh < V; ++hh) {
                wi[r][hh] = swz(((((uint32_t)r << h.ntlog) | tid) * V) + hh);
                asm volatile("" : "+v"(wi[r][hh]));
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    ri[k][r][hh] = 0;
                    if (!(OWN0 && k == 0)) {
                        ri[k][r][hh] = swz(lr[k][r] | ((uint32_t)hh << hbit[k]));
                        asm volatile("" : "+v"(ri[k][r][hh]));
                    }
                }
            }
    }

    // one-shot form with few addresses (the 4-way sum: 24 of reads, 8 of writes): whole LDS addresses, formed here (round 6: the
    // base and the scaling used to be added behind the barrier -- ~50 vector instructions in front of the transposing reads)
    constexpr bool ABS = !PIPE && (NG * NLR * NREP * V <= 32) && (sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16);
    uint32_t pa[ABS ? NG : 1][NREP][V], la[ABS ? NG : 1][NK][NREP][V];
    if constexpr (ABS) {
        const uint32_t lbase = (uint32_t)(uintptr_t)smem_raw;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int r = 0; r < NREP; ++r)
#pragma unroll
                for (int hh = 0; hh < V; ++hh) {
                    pa[g][r][hh] = lbase + ((((uint32_t)g) << tilelog) + wi[r][hh]) * (uint32_t)sizeof(T);
                    asm volatile("" : "+v"(pa[g][r][hh]));
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        la[g][k][r][hh] = 0;
                        if (!(OWN0 && k == 0)) {
                            la[g][k][r][hh] = lbase + (sbase[g][k] + ri[k][r][hh]) * (uint32_t)sizeof(T);
                            asm volatile("" : "+v"(la[g][k][r][hh]));
                        }
                    }
                }
    }

    uint32_t wg = blockIdx.x, tidp = tid;
    for (;;) {
        if constexpr (PIPE) {
            // loop-invariant LDS addresses (one per view x repeat x slot) would be hoisted and spill: recompute them
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int r = 0; r < NREP; ++r) asm volatile("" : "+v"(lr[k][r]));
#pragma unroll
            for (int r = 0; r < NREP; ++r) asm volatile("" : "+v"(goff[r]));
            asm volatile("" : "+v"(tidp));
        }
        // the NEXT orbit's origin row is requested before the slots are parked (unconditionally, on a clamped index:
        // no branch in front of the LDS stores), so that it has arrived when the barrier opens and the next loads
        // leave right behind it
        i64 norg[NG];
        uint64_t nmap = 0;
        bool nlive = false, more = false;
        if constexpr (PIPE) {
            wg += gridDim.x;
            more = wg < (uint32_t)a.nlist;
            load_row(more ? wg : (uint32_t)a.nlist - 1u, norg, nmap, nlive);
        }
        // ---- park the slots in LDS ---------------------------------------------------------------------------
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            T* L = lds + ((size_t)g << a.tilelog);
#pragma unroll
            for (int r = 0; r < NREP; ++r) {
                const uint32_t e = (((uint32_t)r << h.ntlog) | tidp) * V;
#pragma unroll
                for (int hh = 0; hh < V; ++hh) {
                    if constexpr (PIPE) L[swz(e + hh)] = x[g][r].v[hh];
                    else if constexpr (ABS) lds_put<T>(pa[g][r][hh], x[g][r].v[hh]);
                    else L[wi[r][hh]] = x[g][r].v[hh];
                }
            }
        }
        __syncthreads();
        VT xn[NG][NREP];
        if constexpr (PIPE) {
            if (more) {
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int r = 0; r < NREP; ++r) xn[g][r] = *reinterpret_cast<const VT*>(h.src + norg[g] + goff[r]);
            }
        }

        // ---- outputs of every slot: all LDS reads of a repeat are issued before the first use ----------------
        // (the one-shot form batches the reads of all slots: one LDS latency per repeat; the persistent form has the
        // next orbit's loads in registers as well and batches per slot)
        constexpr int GB = (PIPE && NREP > 1) ? 1 : NG;
#pragma unroll
        for (int r = 0; r < NREP; ++r) {
#pragma unroll
            for (int g0 = 0; g0 < NG; g0 += GB) {
                T val[GB][V][NK];
#pragma unroll
                for (int gi = 0; gi < GB; ++gi)
#pragma unroll
                    for (int h = 0; h < V; ++h)
#pragma unroll
                        for (int k = 0; k < NK; ++k) {
                            const int g = g0 + gi;
                            if (OWN0 && k == 0) {
                                val[gi][h][k] = x[g][r].v[h];
                            } else {
                                // sub-element h moves along tiled dim 0 of the natural order
                                if constexpr (PIPE) {
                                    const uint32_t idx = lr[k][r] | ((uint32_t)h << hbit[k]);
                                    val[gi][h][k] = lds[sbase[g][k] + swz(idx)];
                                } else if constexpr (ABS) {
                                    val[gi][h][k] = lds_get<T>(la[g][k][r][h]);
                                } else {
                                    val[gi][h][k] = lds[sbase[g][k] + ri[k][r][h]];
                                }
                            }
                        }
                __builtin_amdgcn_sched_barrier(0);  // keep the reads together: one LDS latency per batch, not one per output
#pragma unroll
                for (int gi = 0; gi < GB; ++gi) {
                    const int g = g0 + gi;
                    VT out;
#pragma unroll
                    for (int h = 0; h < V; ++h) {
                        T arg[MAXIN];
#pragma unroll
                        for (int k = 0; k < MAXIN; ++k) {
                            arg[k] = T{};
                            if (k < NK) {
                                T v = val[gi][h][k < NK ? k : 0];
                                if constexpr (tr<T>::cx) v = ocj(v, cbit[k < NK ? k : 0]);
                                arg[k] = v;
                            }
                        }
                        (void)nin;
                        T o = f(arg);
                        if constexpr (tr<T>::cx) o = ocj(o, conj0);
                        out.v[h] = o;
                    }
                    x[g][r] = out;
                }
                if constexpr (PIPE) __builtin_amdgcn_sched_barrier(0);  // one slot at a time: the registers hold two orbits
            }
        }
        if constexpr (!PIPE) {
            if (!live) return;
        }
        const bool nts = nts_flag != 0;
        if (!PIPE || live) {
            if (nts_flag == 2) {  // agent-scope write-through ("self-released" launch: smr_device.h)
                if constexpr (has_wt_store<VT>::value) {
#pragma unroll
                    for (int g = 0; g < NG; ++g)
#pragma unroll
                        for (int r = 0; r < NREP; ++r) store_vec_wt<VT>(h.dst + org[g] + goff[r], x[g][r]);
                }
            } else if (nts) {
                nt_block_guard();
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int r = 0; r < NREP; ++r) store_vec_ct<true, VT>(h.dst + org[g] + goff[r], x[g][r]);
                nt_block_guard();
            } else {
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int r = 0; r < NREP; ++r) store_vec_ct<false, VT>(h.dst + org[g] + goff[r], x[g][r]);
            }
        }
        if constexpr (!PIPE) {
            if (nts_flag == 2) self_release_wait();
            return;
        } else {
            if (!more) {
                if (nts_flag == 2) self_release_wait();
                return;
            }
            __syncthreads();  // every lane has read its LDS values: the slots may be overwritten
            live = nlive;
            slot_bases(nmap);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                org[g] = norg[g];
#pragma unroll
                for (int r = 0; r < NREP; ++r) x[g][r] = xn[g][r];
            }
        }
    }
}

// ---- PAIR form (round 6): 4^4 cubes of 8-byte elements, |G| = 4, identity view first ---------------------------------------------
// tools/orbit16_probe.hip: the memory system serves this pattern by REQUESTS -- one per 32-byte run of a cube (TCP_TCC_READ_REQ =
// 262144 for the 8 MiB of the 4-way sum at 32^4, a quarter of what a line-wide kernel needs per request) -- and a lane quad that
// covers two neighbouring cubes' halves of one 64-byte run makes one request of two.  A workgroup of 256 lanes owns TWO slot sets
// (plan_orbit: where it can, set 1 is the orbit of set 0's unit-axis neighbour); lane bit 1 selects the set, so slot 0 of both moves
// as 64-byte runs -- 4.29 -> 4.13 us warm, 6.5 -> 5.9 us from HBM (the 16-cube form with two paired slots loses: one workgroup
// per CU waits for ALL its loads before the first exchange).  Every cube has its own 2-KiB LDS region; the in-region index folds its
// three high bits into bank bits 1..3 and set 1's regions are XORed with 17: the 32 lanes of a half-wave then hit 32 distinct
// 8-byte banks in the parking writes and in every transposing read (16 lanes of a set stay inside {bit 0 ^ bit 4 = const}).
// Table: per workgroup 4 entries (one per slot j) of 8 words -- origin of set 0 / set 1 (element offsets; first word 0xffffffff:
// idle), the own region words (16 bits per set: region << 8 | parity * 17), then for views 1..3 the region words of the cubes an
// output of slot j reads that view from.
template <class T, class F, int SMODE = -1>  // SMODE: store policy fixed at compile time (0 plain, 1 non-temporal, 2 write-through), -1: from the arguments
SMR_DEV void orbit_pair_body(const OrbitArgs a, const OrbitHead h, F f) {
    constexpr int V = 2;
    typedef OVec<T, V> VT;
    constexpr int NK = F::NIN;
    static_assert(NK >= 2 && NK <= 4 && sizeof(T) == 8, "PAIR form: 2..4 views of 8-byte elements");
    typedef uint32_t entv __attribute__((ext_vector_type(8)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const uint32_t tid = threadIdx.x;
    const uint32_t b = (tid >> 1) & 1u;
    const uint32_t u = (tid & 1u) | ((tid >> 2) << 1);  // the lane's place in its cube (7 bits)
    const uint32_t e = u * V;
    entv ent[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ent[j] = reinterpret_cast<const entv*>(h.list)[blockIdx.x * 4u + (uint32_t)j];
    const bool live = ent[0][0] != 0xffffffffu;
    uint32_t cj[OMAXT], goff = 0;
#pragma unroll
    for (int j = 0; j < OMAXT; ++j) {
        cj[j] = __builtin_amdgcn_ubfe(e, (h.eshp >> (8 * j)) & 0xffu, (h.elenp >> (8 * j)) & 0xffu);
        goff += cj[j] * h.estride[j];
    }
    i64 org[4];
    VT x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t o32 = live ? (b ? ent[j][1] : ent[j][0]) : 0u;
        org[j] = (i64)o32 * (i64)sizeof(T);
        x[j] = *reinterpret_cast<const VT*>(h.src + org[j] + goff);
    }
    // ---- while the loads fly: LDS indices ----------------------------------------------------------------------------------------
    auto swz = [](uint32_t i) { return i ^ (((i >> 5) & 7u) << 1); };
    const uint32_t sh = b * 16u;
    uint32_t wi[V], ri[NK][V], own[4], src[4][NK];
#pragma unroll
    for (int hh = 0; hh < V; ++hh) wi[hh] = swz(e + (uint32_t)hh);
#pragma unroll
    for (int k = 1; k < NK; ++k) {
        uint32_t l = 0;
#pragma unroll
        for (int j = 0; j < OMAXT; ++j) l |= cj[j] << a.lsh[k][j];
#pragma unroll
        for (int hh = 0; hh < V; ++hh) ri[k][hh] = swz(l | ((uint32_t)hh << a.lsh[k][0]));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        own[j] = (ent[j][2] >> sh) & 0xffffu;
#pragma unroll
        for (int k = 1; k < NK; ++k) src[j][k] = (ent[j][2 + k] >> sh) & 0xffffu;
    }
    uint32_t cbit[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) cbit[k] = a.conjbit[k];
    uint32_t conj0 = a.conj0 ? 0x80000000u : 0u, nts_flag = (uint32_t)a.nts;
    // everything above is pinned in registers HERE, while the global loads fly (left alone the compiler fetches the kernel arguments
    // it needs behind the barrier: two serial scalar-memory round trips in a launch whose waves live 2 us)
    asm volatile("" : "+s"(conj0), "+s"(nts_flag));
#pragma unroll
    for (int k = 0; k < NK; ++k) asm volatile("" : "+s"(cbit[k]));
    // the LDS addresses themselves (24 of reads, 8 of writes): formed here, not behind the barrier -- whole 32-bit LDS addresses (the
    // base of the dynamic segment included: added behind the barrier it cost 24 more vector instructions in front of the reads)
    const uint32_t lbase = (uint32_t)(uintptr_t)smem_raw;
    uint32_t wa[4][V], ra[4][V][NK];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int hh = 0; hh < V; ++hh) {
            wa[j][hh] = lbase + (own[j] ^ wi[hh]) * (uint32_t)sizeof(T);
            asm volatile("" : "+v"(wa[j][hh]));
#pragma unroll
            for (int k = 1; k < NK; ++k) {
                ra[j][hh][k] = lbase + (src[j][k] ^ ri[k][hh]) * (uint32_t)sizeof(T);
                asm volatile("" : "+v"(ra[j][hh][k]));
            }
        }
    // ---- park, exchange ----------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int hh = 0; hh < V; ++hh) lds_put<T>(wa[j][hh], x[j].v[hh]);
    __syncthreads();
    T val[4][V][NK];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int hh = 0; hh < V; ++hh) {
            val[j][hh][0] = x[j].v[hh];
#pragma unroll
            for (int k = 1; k < NK; ++k) val[j][hh][k] = lds_get<T>(ra[j][hh][k]);
        }
    __builtin_amdgcn_sched_barrier(0);  // all LDS reads issued before the first use: one LDS latency, then per slot adds and its store
    if (!live) return;
    auto outputs = [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            VT out;
#pragma unroll
            for (int hh = 0; hh < V; ++hh) {
                T arg[MAXIN];
#pragma unroll
                for (int k = 0; k < MAXIN; ++k) {
                    arg[k] = T{};
                    if (k < NK) {
                        T v = val[j][hh][k < NK ? k : 0];
                        if constexpr (tr<T>::cx) v = ocj(v, cbit[k < NK ? k : 0]);
                        arg[k] = v;
                    }
                }
                T o = f(arg);
                if constexpr (tr<T>::cx) o = ocj(o, conj0);
                out.v[hh] = o;
            }
            char* p = h.dst + org[j] + goff;
            if constexpr (MODE == 2) {
                store_vec_wt<VT>(p, out);
            } else if constexpr (MODE == 1) {
                nt_block_guard();
                store_vec_ct<true, VT>(p, out);
                nt_block_guard();
            } else {
                store_vec_ct<false, VT>(p, out);
            }
        }
    };
    if constexpr (SMODE == 0) {
        outputs(IntC<0>{});
    } else if constexpr (SMODE == 1) {
        outputs(IntC<1>{});
    } else if constexpr (SMODE == 2) {
        if constexpr (has_wt_store<VT>::value) outputs(IntC<2>{});
        self_release_wait();
    } else if (nts_flag == 2) {
        if constexpr (has_wt_store<VT>::value) outputs(IntC<2>{});
        self_release_wait();
    } else if (nts_flag) {
        outputs(IntC<1>{});
    } else {
        outputs(IntC<0>{});
    }
}

#ifndef SMR_JIT
template <class T, class F, int SMODE>
__global__ void __launch_bounds__(256) k_orbit_pair(const uint32_t* list, const char* src, char* dst, uint32_t eshp, uint32_t elenp, uint32_t es0, uint32_t es1,
                                                    uint32_t es2, uint32_t es3, uint32_t ntlog, const OrbitArgs a, F f SMR_STAMP_PARAM) {
    SMR_STAMP_BEGIN
    OrbitHead h;
    h.list = list;
    h.src = src;
    h.dst = dst;
    h.eshp = eshp;
    h.elenp = elenp;
    h.estride[0] = es0;
    h.estride[1] = es1;
    h.estride[2] = es2;
    h.estride[3] = es3;
    h.ntlog = ntlog;
    orbit_pair_body<T, F, SMODE>(a, h, f);
    SMR_STAMP_END
}

template <class T, class F, int V, int NREP, int NG, bool OWN0, bool PIPE>
__global__ void __launch_bounds__(1024) k_orbit_map(const uint32_t* list, const char* src, char* dst, uint32_t eshp, uint32_t elenp, uint32_t es0, uint32_t es1,
                                                    uint32_t es2, uint32_t es3, uint32_t ntlog, const OrbitArgs a, F f SMR_STAMP_PARAM) {
    // the leading scalars = OrbitHead, preloaded into SGPRs: the origin row's load is the first thing the wave does, and the global
    // loads leave as soon as it is back (tools/orbit32_probe.hip: 4.76 -> 4.45 us at 32^4)
    SMR_STAMP_BEGIN
    OrbitHead h;
    h.list = list;
    h.src = src;
    h.dst = dst;
    h.eshp = eshp;
    h.elenp = elenp;
    h.estride[0] = es0;
    h.estride[1] = es1;
    h.estride[2] = es2;
    h.estride[3] = es3;
    h.ntlog = ntlog;
    orbit_map_body<T, F, V, NREP, NG, OWN0, PIPE>(a, h, f);
    SMR_STAMP_END
}

// the natively compiled kernels take OrbitHead as leading scalar parameters (preloaded into SGPRs), then the struct
#define SMR_ORBIT_LAUNCH(kern, L, s, f)                                                                                                  \
    do {                                                                                                                                 \
        const OrbitHead h_ = orbit_head((L).a);                                                                                          \
        SMR_LAUNCH(kern, dim3((L).grid), dim3((L).block), (L).lds, s, h_.list, h_.src, h_.dst, h_.eshp, h_.elenp, h_.estride[0],          \
                   h_.estride[1], h_.estride[2], h_.estride[3], h_.ntlog, (L).a, f SMR_STAMP_ARG((L).grid, (L).block));                  \
    } while (0)

// native_nin of orbit_variant(): the PAIR form exists for natively compiled functors only
template <class F> constexpr int orbit_native_nin() { return is_jit<F>::value ? -1 : F::NIN; }

template <class T, class F, int V, int NREP, int NG, bool OWN0, bool PIPE>
static int go4(const Plan& plan, hipStream_t s, F f, const OpTab& tab, const OrbitVariant& ov) {
    OrbitLaunch L;
    if (int rc = orbit_launch_args(plan, tab.base, (int)sizeof(T), ov, has_wt_store<OVec<T, V>>::value, L)) return rc;
    if constexpr (is_jit<F>::value) {
        return launch_jit<T>(plan.c, s, "orbit", "smr::OrbitArgs", "orbit_map_body", "smr::orbit_head(a), ", L.grid, L.block, L.lds, L.a, V, NREP,
                             NG, OWN0, PIPE);
    } else {
        auto kern = k_orbit_map<T, F, V, NREP, NG, OWN0, PIPE>;
        return launch_native((const void*)kern, L.lds, "k_orbit_map", [&] {
            if (!PIPE) mark_sliceable(2, 0u, (unsigned)(2 * NG * sizeof(uint32_t)));  // one table row per workgroup; the pointer is parameter 0
            if (L.a.nts == 2) mark_self_released();
            SMR_ORBIT_LAUNCH(kern, L, s, f);
        });
    }
}

template <class T, class F>
static int go_pair(const Plan& plan, hipStream_t s, F f, const OpTab& tab, const OrbitVariant& ov) {
    OrbitLaunch L;
    if (int rc = orbit_launch_args(plan, tab.base, (int)sizeof(T), ov, has_wt_store<OVec<T, 2>>::value, L)) return rc;
    return launch_native(nullptr, L.lds, "k_orbit_pair", [&] {
        mark_sliceable(2, 0u, (unsigned)(4 * 8 * sizeof(uint32_t)));  // one table row (four entries) per workgroup; the pointer is parameter 0
        if (L.a.nts == 2) mark_self_released();
        // one kernel per store policy: no branch on a kernel argument between the exchange and the stores
        if (L.a.nts == 2)
            SMR_ORBIT_LAUNCH((k_orbit_pair<T, F, 2>), L, s, f);
        else if (L.a.nts)
            SMR_ORBIT_LAUNCH((k_orbit_pair<T, F, 1>), L, s, f);
        else
            SMR_ORBIT_LAUNCH((k_orbit_pair<T, F, 0>), L, s, f);
    });
}

// The kernel of orbit_variant()'s choice (smr_plan_orbit.cpp) among those compiled for (V, NREP): the PAIR form (go2), or the
// one-orbit form with 2 or 4 slots, view 0 the identity view or not (go2), one-shot or persistent (go3)
// The `if constexpr` conditions below say which kernels are compiled; orbit_variant() says which one runs.  The three "no ... kernel
// of this variant" errors (go3, go2, go) can fire only if the two ever drift apart: they guard, no plan reaches them.
template <class T, class F, int V, int NREP, int NG, bool OWN0>
static int go3(const Plan& plan, hipStream_t s, F f, const OpTab& tab, const OrbitVariant& ov) {
    if constexpr (V * sizeof(T) == 16) {
        if (ov.pipe) return go4<T, F, V, NREP, NG, OWN0, true>(plan, s, f, tab, ov);
    }
    if (ov.pipe) return set_error(SMR_EINVAL, "orbit: no persistent kernel of this variant");
    return go4<T, F, V, NREP, NG, OWN0, false>(plan, s, f, tab, ov);
}

template <class T, class F, int V, int NREP>
static int go2(const Plan& plan, hipStream_t s, F f, const OpTab& tab, const OrbitVariant& ov) {
    if constexpr (V == 2 && NREP == 1 && sizeof(T) == 8 && orbit_native_nin<F>() >= 2 && orbit_native_nin<F>() <= 4) {
        if (ov.pair) return go_pair<T, F>(plan, s, f, tab, ov);
    }
    if (ov.pair) return set_error(SMR_EINVAL, "orbit: no PAIR kernel of this variant");
    if (ov.ng == 2) return ov.own0 ? go3<T, F, V, NREP, 2, true>(plan, s, f, tab, ov) : go3<T, F, V, NREP, 2, false>(plan, s, f, tab, ov);
    return ov.own0 ? go3<T, F, V, NREP, 4, true>(plan, s, f, tab, ov) : go3<T, F, V, NREP, 4, false>(plan, s, f, tab, ov);
}

template <class T, class F>
static int go(const Plan& plan, void* const* bases, hipStream_t s, F f) {
    const Canon& c = plan.c;
    const OrbitPlan& o = plan.orbit;
    const OpTab tab = make_optab(c, bases);
    // every view must still be a view of ONE buffer after rebinding
    for (int k = 1; k < c.M; ++k)
        if (tab.base[k] != tab.base[o.k0]) return set_error(SMR_EINVAL, "orbit plan: the inputs must stay views of one buffer");
    OrbitVariant ov;
    if (int rc = orbit_variant(plan, bases, (int)sizeof(T), orbit_native_nin<F>(), ov)) return rc;
    constexpr int VMAX = (16 / sizeof(T)) > 1 ? (int)(16 / sizeof(T)) : 1;
    if constexpr (VMAX > 1) {  // 16-byte accesses; element-wise ones (operands not 16-byte aligned) for tiles of up to 1024 elements
        if (ov.V == VMAX && ov.nrep == 1) return go2<T, F, VMAX, 1>(plan, s, f, tab, ov);
        if (ov.V == VMAX && ov.nrep == 2) return go2<T, F, VMAX, 2>(plan, s, f, tab, ov);
        if (ov.V == 1 && ov.nrep == 1) return go2<T, F, 1, 1>(plan, s, f, tab, ov);
    } else {
        if (ov.V == 1 && ov.nrep == 1) return go2<T, F, 1, 1>(plan, s, f, tab, ov);
        if (ov.V == 1 && ov.nrep == 2) return go2<T, F, 1, 2>(plan, s, f, tab, ov);
        if (ov.V == 1 && ov.nrep == 4) return go2<T, F, 1, 4>(plan, s, f, tab, ov);
    }
    return set_error(SMR_EINVAL, "orbit: no kernel of this variant");
}

template <>
int launch_orbit_map_ct<SMR_CT>(const Plan& plan, void* const* bases, hipStream_t s) {
    typedef ct_type<SMR_CT>::type T;
    const Canon& c = plan.c;
    switch (c.fkind) {  // natively compiled functors of this family; everything else is compiled at run time
        case FK_ADD2: return go<T, FAdd2<T>>(plan, bases, s, FAdd2<T>{});
        case FK_ADD4: return go<T, FAdd4<T>>(plan, bases, s, FAdd4<T>{});
        case FK_SYM: return go<T, FSym<T>>(plan, bases, s, FSym<T>{hostmk<T>(c.fc[0], c.fc[1])});
        default: break;
    }
    return with_prog<T>(c, [&](auto f) { return go<T, decltype(f)>(plan, bases, s, f); });
}
#endif  // !SMR_JIT

}  // namespace smr
