// smr_tiled_args.h -- the kernel arguments of family TILED (smr_k_tiled.hip): the structs the kernels read, the pure builder that
// computes them from a plan (smr_plan_tiled_args.cpp) and the per-call wrapper around it (smr_api.cpp).  Shared by the kernels'
// translation units, the planner and tools/plan_dump.cpp; the top part is also compiled by hiprtc (SMR_JIT).
#pragma once

#include "smr_internal.h"

namespace smr {

constexpr int MAXT = 5;
constexpr int NG = TILED_NG;  // grid dims decoded branch-free; further ones in a (rare) loop
constexpr int EPL = 4;  // elements per lane (tile elements / workgroup size)
constexpr int NORD16 = 512;  // tile-order entries that fit into the kernel arguments

template <bool WIDE> struct off_t_of { typedef uint32_t type; };
template <> struct off_t_of<true> { typedef i64 type; };

// one row of the per-lane table
template <bool WIDE> struct LaneRow { uint32_t g; uint32_t l; };
template <> struct alignas(16) LaneRow<true> { i64 g; uint32_t l; uint32_t pad; };

// Wave-uniform description of one operand (a few wide scalar loads).
template <bool WIDE>
struct OpDesc {
    typedef typename off_t_of<WIDE>::type O;
    void* base;            // element offset already applied
    uint32_t tstep32[NG];  // byte offset of one tile step along grid dim g (when base32)
    O Gr[EPL];             // byte offset of repeat index r (own order if staged, else dst order)
    uint32_t Lr[EPL];      // staged: swizzled LDS index of repeat index r (own order)
    uint32_t Lh[EPL];      // staged: ... of sub-element h
    int32_t dtype, conj;
};

template <bool WIDE>
struct TiledArgs {
    // header + tile decode first: they arrive with the first batch of scalar loads
    int32_t M, ng, tilelog, nstaged, base32, nt, ordmode, nwork;  // nwork: entries of the work list (persistent form)
    int32_t nts;           // nts: non-temporal stores (small destinations: see Options::nt_store)
    uint32_t blk0;         // first workgroup of a block-range slice (smr_seq.cpp); 0 for a whole launch.  One-shot form only
    int32_t pad_[2];
    int32_t staged[MAXM];  // [1 + i]: LDS slot of input i or -1 ([0] unused)
    uint32_t ntiles[MAXN], div_m[MAXN], div_s[MAXN], last_ragged[MAXN];
    const LaneRow<WIDE>* lanetab;  // [(operand k) * T + tid], k = 0 destination
    const uint32_t* ordtab;        // ordmode 2: tile executed by workgroup b (0xffffffff = none)
    OpDesc<WIDE> op[MAXM];         // [0] destination, [1 + i] input i
    uint32_t Lrd[EPL], Lhd[EPL];   // destination-order LDS index of repeat r / sub-element h
    i64 tstep[MAXM][MAXN];         // 64-bit tile steps (only read when !base32)
    // edge tiles only
    uint32_t gflip, gflip_pad;        // bit g: grid coordinate g counts DOWN (ragged dims: their last, partly filled tiles start first)
    int32_t ej_g[MAXT];               // per tiled dim j: its grid slot (-1: none), the index of its LAST tile and the valid elements in
    uint32_t ej_ntm1[MAXT], ej_last[MAXT];  // that tile (round 6: one batch of scalar loads instead of a dependent chain through tgrid / gdims / glog)
    int32_t tgrid[MAXT], tlog[MAXT];  // grid dim / log2 extent of tiled dim j
    int32_t esh[MAXM][MAXT];          // bit position of tiled dim j in operand k's enumeration
    i64 gdims[MAXN];
    int32_t glog[MAXN];
    uint32_t ord16[NORD16 / 2];  // ordmode 1: the same as 16-bit entries inside the kernel arguments
    // Unused: the 656 bytes the retired BITS form (lane rows computed from bit slices of the lane id) kept here; always zero, read by
    // no kernel.  Left in place because the general variant (MODE 7) copies the whole struct to scratch: without them its scratch
    // size and instruction stream change (profiles/args_refactor.txt), which wants a measurement of its own.
    uint32_t unused_tail_[164];
};

#ifndef SMR_JIT
// What the pure builder returns: the arguments of kernel variant (WIDE, tv.V, tv.mode, tv.thrlog) with every pointer null, and the
// per-lane table `lanetab` will address.  (The tile-order table `ordtab` addresses when ordmode == 2 is the plan's own TilePlan::ord.)
template <bool WIDE>
struct TiledBuild {
    TiledArgs<WIDE> a;
    std::vector<LaneRow<WIDE>> rows;  // [(operand k) * threads + tid]
};
// smr_plan_tiled_args.cpp: a function of the plan, the element size, the variant and options() alone -- no device, no cache
template <bool WIDE>
int build_tiled_args(const Plan& plan, int esize, const TiledVariant& tv, TiledBuild<WIDE>& b);

// A TILED launch of kernel variant (WIDE, V, MODE, THRLOG) apart from the kernel itself
template <bool WIDE>
struct TiledLaunch {
    TiledArgs<WIDE> a;
    unsigned grid = 0;        // workgroups of the one-shot form
    unsigned pgrid = 0;       // of the persistent, software-pipelined form (0: the one-shot form runs)
    size_t lds = 0;
};
// smr_api.cpp: the arguments of one execution.  Built on the plan's first execution of the variant (WIDE, V) with its lane and
// tile-order tables uploaded, and cached in the plan (Plan::tiled_cache; nothing is uploaded or cached by a dry run); the operand
// addresses `base` (OpTab::base) and the store policy are set per call.  wt_store: the kernel's vector type has write-through stores.
template <bool WIDE>
int tiled_launch_args(const Plan& plan, void* const* base, int esize, const TiledVariant& tv, bool wt_store, TiledLaunch<WIDE>& L);
#endif

}  // namespace smr
