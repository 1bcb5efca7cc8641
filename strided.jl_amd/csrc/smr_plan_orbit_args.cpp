// smr_plan_orbit_args.cpp -- the pure builders of ORBIT's kernel arguments (smr_orbit_args.h): tile enumeration, the searched LDS
// swizzle, per-workgroup origin rows and the PAIR form's work list.  Device-free like the rest of the planner: tools/plan_dump.cpp
// digests their output and runs them under AddressSanitizer + UBSan.  The per-call wrapper (cache, uploads, operand addresses, store
// policy, persistent grid) is orbit_launch_args, smr_api.cpp.
#include <cstdio>
#include <cstring>

#include "smr_plan.h"
#include "smr_orbit_args.h"

namespace smr {

// XOR-fold swizzle l ^ (((l >> s1) ^ (l >> s2)) & mask): parameters picked per plan by counting the
// bank conflicts of the transposing LDS reads (a lane group of the hardware must hit distinct banks)
struct OSwz {
    uint32_t s1 = 31, s2 = 31, mask = 0;
    uint32_t operator()(uint32_t i) const { return i ^ (((i >> s1) ^ (i >> s2)) & mask); }
};

static OSwz choose_orbit_swizzle(const OrbitArgs& a, int nin, bool own0, int esize, int V, int NREP) {
    // lane group / bank-slot model: ds_read_b32/b64 are served in two halves of 32 lanes over 32 slots
    // of the access width; ds_read_b128 in groups of 16 lanes over 16 slots
    const int group = esize >= 16 ? 16 : 32;
    const uint32_t slots = (uint32_t)group;
    const uint32_t nt = 1u << a.ntlog;
    auto cost = [&](const OSwz& s) {
        long c = 0;
        for (int k = own0 ? 1 : 0; k < nin; ++k)
            for (int r = 0; r < NREP; ++r)
                for (int h = 0; h < V; ++h)
                    for (uint32_t w0 = 0; w0 < std::min(nt, 256u); w0 += group) {
                        uint32_t first[32];
                        int cnt[32];
                        int worst = 0;
                        for (uint32_t q = 0; q < slots; ++q) cnt[q] = 0;
                        for (int lane = 0; lane < group; ++lane) {
                            const uint32_t e = (((uint32_t)r << a.ntlog) | (w0 + lane)) * V + h;
                            uint32_t idx = 0;
                            for (int j = 0; j < OMAXT; ++j) idx |= ((e >> a.esh[j]) & ((1u << a.elen[j]) - 1u)) << a.lsh[k][j];
                            const uint32_t l = s(idx), q = l % slots;
                            if (cnt[q] == 0) {
                                first[q] = l;
                                cnt[q] = 1;
                            } else if (first[q] != l) {
                                ++cnt[q];
                            }
                        }
                        for (uint32_t q = 0; q < slots; ++q) worst = std::max(worst, cnt[q]);
                        c += worst - 1;
                    }
        return c;
    };
    OSwz best;
    long bc = cost(best);
    auto consider = [&](uint32_t s1, uint32_t s2) {
        OSwz t;
        t.s1 = s1;
        t.s2 = s2;
        t.mask = slots - 1;
        const long cc = cost(t);
        if (cc < bc) {
            bc = cc;
            best = t;
        }
    };
    for (uint32_t s1 = 2; s1 <= 6 && bc > 0; ++s1) {
        consider(s1, 31);  // one-term fold
        for (uint32_t s2 = s1 + 1; s2 <= 13 && bc > 0; ++s2) consider(s1, s2);
    }
    if (std::getenv("SMR_DEBUG_SWIZZLE"))
        std::fprintf(stderr, "[smr] orbit swizzle: s1=%u s2=%u mask=%u conflict cost %ld\n", best.s1, best.s2, best.mask, bc);
    return best;
}

// The part of the arguments both forms share: tiled dims in canonical (= natural) order, each view's LDS bit positions and conjugation
static int orbit_dims(const Plan& plan, int esize, OrbitArgs& a) {
    const Canon& c = plan.c;
    const OrbitPlan& o = plan.orbit;
    a.nin = c.M - 1;
    a.tilelog = o.tilelog;
    a.conj0 = c.conj[0];
    int nt = 0, sh = 0, jof[MAXN];
    for (int d = 0; d < c.N; ++d) {
        jof[d] = -1;
        if (o.lg[d] == 0) continue;
        if (nt >= OMAXT) return set_error(SMR_EUNSUPPORTED, "orbit: too many tiled dims");
        jof[d] = nt;
        a.esh[nt] = sh;
        a.elen[nt] = o.lg[d];
        a.estride[nt] = (uint32_t)(c.strides[o.k0][d] * esize);
        sh += o.lg[d];
        ++nt;
    }
    for (int k = 1; k < c.M; ++k) {
        for (int d = 0; d < c.N; ++d)
            if (jof[d] >= 0) a.lsh[k - 1][jof[d]] = a.esh[jof[o.pdim[k][d]]];
        a.conjbit[k - 1] = c.conj[k] ? 0x80000000u : 0u;
    }
    return SMR_OK;
}

// element offset of tile `id` (canonical tile index) in the shared buffer
static uint32_t orbit_tile_origin(const Plan& plan, i64 id) {
    const OrbitPlan& o = plan.orbit;
    i64 org = 0;
    for (int d = 0; d < plan.c.N; ++d) {
        org += (id % o.ntiles[d]) * (plan.c.strides[o.k0][d] << o.lg[d]);
        id /= o.ntiles[d];
    }
    return (uint32_t)org;
}

int build_orbit_args(const Plan& plan, int esize, const OrbitVariant& v, OrbitBuild& b) {
    const Canon& c = plan.c;
    const OrbitPlan& o = plan.orbit;
    const int V = v.V, NREP = v.nrep, NG = v.ng;
    const bool OWN0 = v.own0;
    OrbitArgs& a = b.a;
    std::memset(&a, 0, sizeof a);
    int vlog = 0, nreplog = 0;
    while ((1 << vlog) < V) ++vlog;
    while ((1 << nreplog) < NREP) ++nreplog;
    a.ntlog = o.tilelog - vlog - nreplog;
    if (int rc = orbit_dims(plan, esize, a)) return rc;
    if (o.nslots != NG) return set_error(SMR_EINVAL, "orbit: slot count mismatch");
    const OSwz sw = choose_orbit_swizzle(a, c.M - 1, OWN0, esize, V, NREP);
    a.swz_s1 = sw.s1;
    a.swz_s2 = sw.s2;
    a.swz_mask = sw.mask;
    a.nlist = (int32_t)o.wmap.size();
    // one row per workgroup: the NG slot origins (element offset of the tile in each slot), then the slot map (plan_orbit)
    const size_t nwg = o.wmap.size();
    b.rows.assign(nwg * 2 * NG, 0u);
    for (size_t w = 0; w < nwg; ++w) {
        uint32_t* row = &b.rows[w * 2 * NG];
        if (o.wtile[w * NG] == 0xffffffffu) {
            row[0] = 0xffffffffu;
            continue;
        }
        for (int g = 0; g < NG; ++g) row[g] = orbit_tile_origin(plan, o.wtile[w * NG + g]);
        row[NG] = (uint32_t)o.wmap[w];
        row[NG + 1] = (uint32_t)(o.wmap[w] >> 32);
    }
    return SMR_OK;
}

int build_pair_args(const Plan& plan, int esize, OrbitBuild& out) {
    const Canon& c = plan.c;
    const OrbitPlan& o = plan.orbit;
    constexpr int NS = 4;
    OrbitArgs& a = out.a;
    std::memset(&a, 0, sizeof a);
    a.ntlog = 8;
    if (int rc = orbit_dims(plan, esize, a)) return rc;
    a.nlist = (int32_t)(o.pmap.size() / 2);
    const size_t nwg = o.pmap.size() / 2;
    std::vector<uint32_t>& rows = out.rows;
    rows.assign(nwg * 4 * 8, 0u);
    auto region = [](int slot, int b) { return (uint32_t)(((2 * slot + b) << 8) | (b ? 17 : 0)); };
    for (size_t w = 0; w < nwg; ++w) {
        if (o.ptile[w * 8] == 0xffffffffu) {
            rows[w * 32] = 0xffffffffu;
            continue;
        }
        for (int j = 0; j < NS; ++j) {
            uint32_t* en = &rows[(w * 4 + (size_t)j) * 8];
            for (int b = 0; b < 2; ++b) {
                en[b] = orbit_tile_origin(plan, o.ptile[w * 8 + (size_t)b * 4 + (size_t)j]);
                en[2] |= region(j, b) << (16 * b);
                const uint64_t mp = o.pmap[w * 2 + (size_t)b];
                // view k of the kernel = input k + 1; input 1 is the identity view (the lane's own registers)
                for (int k = 1; k < c.M - 1 && k < 4; ++k) en[2 + k] |= region((int)((mp >> ((j * 8 + k) * 2)) & 3u), b) << (16 * b);
            }
        }
    }
    return SMR_OK;
}

}  // namespace smr
