// smr_orbit_args.h -- the kernel arguments of family ORBIT (smr_k_orbit.hip): the structs the kernels read, the pure builders that
// compute them from a plan (smr_plan_orbit_args.cpp) and the per-call wrapper around them (smr_api.cpp).  Shared by the kernels'
// translation units, the planner and tools/plan_dump.cpp; the top part is also compiled by hiprtc (SMR_JIT).
#pragma once

#include "smr_internal.h"

namespace smr {

constexpr int OMAXT = 4;  // tiled dims = dims of the unit class <= |G| <= 4

struct OrbitArgs {
    const char* src;  // the shared buffer, element offset applied
    char* dst;
    const uint32_t* list;  // per workgroup a row of 2 * NG words: the NG slot origins (element offsets; [0] = 0xffffffff: idle), then the
                           // 64-bit slot map -- field (g * 8 + k) * 2: the LDS slot an output of slot g reads input k from.  (The
                           // natively compiled kernels receive this pointer once more as their FIRST parameter: it is preloaded
                           // into SGPRs with the wave, and the row's load leaves before the kernel arguments have been fetched.)
    int32_t nin, tilelog, ntlog, conj0, nts, nlist;  // nlist: rows of `list` (PIPE form)
    uint32_t swz_s1, swz_s2, swz_mask, pad1;
    // element enumeration inside a tile (natural order of the buffer); unused tiled dims have elen = 0
    int32_t esh[OMAXT], elen[OMAXT];
    uint32_t estride[OMAXT];       // byte stride of tiled dim j
    int32_t lsh[MAXIN][OMAXT];     // LDS bit position of tiled dim j as seen through view k
    uint32_t conjbit[MAXIN];       // 0x80000000 when view k is conjugated (complex types)
};

// What a wave needs before its first global load can leave: the natively compiled kernels receive these as LEADING SCALAR
// parameters, which gfx950 preloads into SGPRs with the wave (Makefile: -mllvm -amdgpu-kernarg-preload-count=16) -- the only
// memory round trip in front of the loads is then the origin row's.  (Left in the argument struct the compiler fetched them in
// two dependent batches of scalar loads: tools/orbit32_probe.hip, profiles/r06_orbit_phases.txt.)
struct OrbitHead {
    const uint32_t* list;  // = OrbitArgs::list
    const char* src;       // = OrbitArgs::src
    char* dst;             // = OrbitArgs::dst (left in the struct, its scalar load was sunk between the LDS reads and the adds)
    uint32_t eshp, elenp;  // esh[j] / elen[j] in byte j
    uint32_t estride[OMAXT];
    uint32_t ntlog;
};
static inline __host__ __device__ OrbitHead orbit_head(const OrbitArgs& a) {
    OrbitHead h;
    h.list = a.list;
    h.src = a.src;
    h.dst = a.dst;
    h.eshp = h.elenp = 0;
    for (int j = 0; j < OMAXT; ++j) {
        h.eshp |= (uint32_t)a.esh[j] << (8 * j);
        h.elenp |= (uint32_t)a.elen[j] << (8 * j);
        h.estride[j] = a.estride[j];
    }
    h.ntlog = (uint32_t)a.ntlog;
    return h;
}

#ifndef SMR_JIT
// What the pure builders return: the arguments with every pointer null and the work list `list` will address -- one-orbit form: per
// workgroup the slot origins and the slot map; PAIR form: per workgroup four 8-word entries (orbit_pair_body).
struct OrbitBuild {
    OrbitArgs a;
    std::vector<uint32_t> rows;
};
// smr_plan_orbit_args.cpp: functions of the plan, the element size, the variant and options() alone -- no device, no cache.
// One-orbit form of orbit_variant()'s (V, nrep, ng, own0)
int build_orbit_args(const Plan& plan, int esize, const OrbitVariant& v, OrbitBuild& b);
// PAIR form (orbit_pair_body: 256 lanes per two slot sets, 2 elements per access)
int build_pair_args(const Plan& plan, int esize, OrbitBuild& b);

// An ORBIT launch apart from the kernel itself
struct OrbitLaunch {
    OrbitArgs a;
    unsigned grid = 0, block = 0;
    size_t lds = 0;
};
// smr_api.cpp: the arguments of one execution of the form `v` names.  Built on the plan's first execution of the form with its work
// list uploaded, and cached in the plan (Plan::orbit_cache, orbit_list, pair_cache; nothing is uploaded or cached by a dry run); the
// operand addresses `base` (OpTab::base), the grid and the store policy are set per call.  wt_store: the kernel's vector type has
// write-through stores.
int orbit_launch_args(const Plan& plan, void* const* base, int esize, const OrbitVariant& v, bool wt_store, OrbitLaunch& L);
#endif

}  // namespace smr
