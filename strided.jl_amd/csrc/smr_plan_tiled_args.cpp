// smr_plan_tiled_args.cpp -- the pure builder of TILED's kernel arguments (smr_tiled_args.h): lane tables, the searched LDS swizzle,
// tile decode and edge tables.  Device-free like the rest of the planner: tools/plan_dump.cpp digests its output and runs it under
// AddressSanitizer + UBSan.  The per-call wrapper (cache, uploads, operand addresses, store policy) is tiled_launch_args, smr_api.cpp.
#include <cstdio>
#include <cstring>

#include "smr_plan.h"
#include "smr_tiled_args.h"

namespace smr {

// ---- LDS swizzle ------------------------------------------------------------------------------------
// l' = l ^ XOR_{b >= w, bit b of l set} mask[b]: the low w index bits (the 128 B one LDS write
// group spans, in elements) are XORed with one w-bit mask per higher index bit.  A lane group's
// accesses are conflict-free iff the slot images of the index bits its lanes toggle are linearly
// independent over GF(2).  The masks are searched on the host (a small hill climb, once per plan)
// against the write pattern of every staged operand and the destination-order read pattern; the
// start point is the plain fold mask[b] = 1 << ((b - w) mod w).
struct Swizzle {
    int w;
    uint32_t mask[32];
    uint32_t apply(uint32_t l) const {
        uint32_t r = l;
        for (int b = w; b < 32; ++b)
            if ((l >> b) & 1u) r ^= mask[b];
        return r;
    }
};

static int gf2_rank(const uint32_t* v, int n) {
    uint32_t basis[32];
    int r = 0;
    for (int i = 0; i < n; ++i) {
        uint32_t x = v[i];
        for (int j = 0; j < r; ++j)
            if ((x ^ basis[j]) < x) x ^= basis[j];
        if (x) {
            basis[r++] = x;
            for (int j = r - 1; j > 0 && basis[j] > basis[j - 1]; --j) std::swap(basis[j], basis[j - 1]);
        }
    }
    return r;
}

// the index bits one hardware lane group toggles + the width of the bank-slot space it lands in
struct LanePattern {
    int n;
    int bits[8];
    int slotbits;
};

static Swizzle choose_swizzle(int tilelog, int w, const std::vector<LanePattern>& pats, int* cost0 = nullptr, int* cost1 = nullptr) {
    Swizzle sw;
    sw.w = (w > 0 && tilelog > w) ? w : 32;
    for (int b = 0; b < 32; ++b) sw.mask[b] = 0;
    if (sw.w == 32) return sw;
    for (int b = w; b < tilelog; ++b) sw.mask[b] = 1u << ((b - w) % w);
    auto cost = [&](const Swizzle& s) {
        int c = 0;
        for (const LanePattern& p : pats) {
            uint32_t img[8];
            const uint32_t sm = (1u << p.slotbits) - 1u;
            for (int i = 0; i < p.n; ++i) {
                const int b = p.bits[i];
                uint32_t v = 1u << b;          // the bit itself (dropped below if outside the slot space)
                if (b >= w) v ^= s.mask[b];   // its swizzle mask (acts on the low w bits)
                img[i] = v & sm;
            }
            c += (1 << (p.n - gf2_rank(img, p.n))) - 1;
        }
        return c;
    };
    int best = cost(sw);
    if (cost0) *cost0 = best;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    for (int it = 0; it < 6000 && best > 0; ++it) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        const int b = w + (int)((rng >> 33) % (uint64_t)(tilelog - w));
        const uint32_t m = (uint32_t)((rng >> 20) & ((1u << w) - 1u));
        Swizzle t = sw;
        t.mask[b] = m;
        const int c = cost(t);
        if (c <= best) {
            best = c;
            sw = t;
        }
    }
    if (cost1) *cost1 = best;
    return sw;
}

template <bool WIDE>
int build_tiled_args(const Plan& plan, int esize, const TiledVariant& tv, TiledBuild<WIDE>& out) {
    typedef typename off_t_of<WIDE>::type O;
    const int V = tv.V, MODE = tv.mode, THRLOG = tv.thrlog;
    const bool EDGE = (MODE & 1) != 0, LEAN = (MODE & 4) == 0;
    const int NREP = EPL / V, NT = 1 << THRLOG;
    const Canon& c = plan.c;
    const TilePlan& t = plan.tile;
    const Options& o = options();
    int vlog = 0;
    while ((1 << vlog) < V) ++vlog;
    TiledArgs<WIDE>& a = out.a;
    std::memset(&a, 0, sizeof a);
    a.nwork = (int32_t)(t.ord.empty() ? (unsigned)t.grid : (unsigned)t.ord.size());
    if (!t.ord.empty() && t.ord.size() <= (size_t)NORD16 && t.grid < 0xffff) {
        a.ordmode = 1;
        for (size_t i = 0; i < t.ord.size(); ++i) {
            const uint32_t v = t.ord[i] == 0xffffffffu ? 0xffffu : t.ord[i];
            a.ord16[i >> 1] |= v << (16 * (i & 1));
        }
    } else if (!t.ord.empty()) {
        a.ordmode = 2;  // the wrapper uploads TilePlan::ord
    }
    a.M = c.M;
    a.nt = t.nt;
    a.tilelog = t.tilelog;
    a.nstaged = t.nstaged;
    int tlogdim[MAXN] = {0};
    int lsh[MAXT];
    int sh = 0;
    for (int j = 0; j < t.nt; ++j) {
        lsh[j] = sh;
        tlogdim[t.tdim[j]] = t.tlog[j];
        sh += t.tlog[j];
    }
    // LDS swizzle: slot width = the 128 B an LDS write group spans, in elements
    int w = 0;
    while ((esize << w) < 128) ++w;
    std::vector<LanePattern> pats;
    if (esize >= 4 && t.tilelog > w) {
        const int nread = esize == 16 ? 4 : 5;  // ds_read_b32/b64: 32 lanes, b128: 16 lanes per pass
        for (int k = 1; k < c.M; ++k) {
            if (t.staged[k] < 0) continue;
            // operand k's enumeration: its bit (vlog + i) is lane bit i of the write group
            int bitpos[32], pos = 0;
            for (int jj = 0; jj < t.nt; ++jj) {
                const int j = t.order[k][jj];
                for (int bit = 0; bit < t.tlog[j]; ++bit) bitpos[pos++] = lsh[j] + bit;
            }
            LanePattern p;
            p.n = w;
            p.slotbits = w;
            for (int i2 = 0; i2 < w; ++i2) p.bits[i2] = bitpos[vlog + i2];
            pats.push_back(p);
        }
        LanePattern r;
        r.n = nread;
        r.slotbits = nread;
        for (int i2 = 0; i2 < nread; ++i2) r.bits[i2] = vlog + i2;
        pats.push_back(r);
    }
    int cost0 = 0, cost1 = 0;
    const Swizzle swz = choose_swizzle(t.tilelog, w, pats, &cost0, &cost1);
    if (std::getenv("SMR_DEBUG_SWIZZLE"))
        std::fprintf(stderr, "[smr] tiled swizzle: w=%d V=%d patterns=%zu conflict cost fold=%d searched=%d\n", w, V, pats.size(), cost0, cost1);
    // grid dims: canonical dims with more than one tile, in the order the planner chose (TilePlan::gorder: canonical order, or --
    // HBM-sized transposes -- the tile index along the INPUT's unit axis second: plan_tiles)
    int gof[MAXN], ng = 0;
    for (int d = 0; d < c.N; ++d) gof[d] = -1;
    for (int i = 0; i < c.N; ++i) {
        const int d = t.gorder[i];
        if (d >= 0 && d < c.N && gof[d] < 0 && t.ntiles[d] > 1) gof[d] = ng++;
    }
    for (int d = 0; d < c.N; ++d)  // (anything the planner's order left out: canonical order behind it)
        if (gof[d] < 0 && t.ntiles[d] > 1) gof[d] = ng++;
    a.gflip = 0;
    auto is_ragged = [&](int d) { return tlogdim[d] > 0 && (c.dims[d] & (((i64)1 << tlogdim[d]) - 1)) != 0; };
    int nragged = 0;
    for (int d = 0; d < c.N; ++d)
        if (gof[d] >= 0 && is_ragged(d)) ++nragged;
    // (measured with ONE ragged grid dim: transposes of (7200,104) 4.05 -> 3.23 us, (7168,100) 4.08 -> 3.72, (96,9000) 3.42 -> 3.21;
    // with two -- (100,90,80) permutes -- a tie or a loss: those keep the planner's order.  tiled_edge_first = 2: whenever it applies)
    // ... with two or more they keep the planner's order and only count backwards ((257,129,65) 8.2 -> 7.8 us, (1400,1500) 6.6 -> 6.5;
    // moved to the slow end as well: (300,301,35) 12.1 -> 13.1).  tiled_edge_first = 3: backwards only, 2: moved + backwards, always
    if (EDGE && LEAN && t.ord.empty() && (o.tiled_edge_first == 3 || (o.tiled_edge_first == 1 && nragged >= 2))) {
        for (int d = 0; d < c.N; ++d)
            if (gof[d] >= 0 && gof[d] < NG && is_ragged(d)) a.gflip |= 1u << gof[d];
    } else if (EDGE && LEAN && t.ord.empty() && (o.tiled_edge_first == 2 || (o.tiled_edge_first == 1 && nragged == 1))) {
        // ragged dims to the slow end of the grid (stable), counted backwards
        int order[MAXN], n2 = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int g = 0; g < ng; ++g)
                for (int d = 0; d < c.N; ++d)
                    if (gof[d] == g && (is_ragged(d) ? 1 : 0) == pass) order[n2++] = d;
        for (int i = 0; i < n2; ++i) {
            gof[order[i]] = i;
            if (is_ragged(order[i])) a.gflip |= 1u << i;
        }
    }
    for (int g = 0; g < MAXN; ++g) {
        a.ntiles[g] = 1;
        a.div_m[g] = 0;
        a.div_s[g] = 0;
        a.last_ragged[g] = 0xffffffffu;
        a.gdims[g] = 1;
        a.glog[g] = 0;
    }
    for (int d = 0; d < c.N; ++d) {
        const int g = gof[d];
        if (g < 0) continue;
        const uint32_t nt = (uint32_t)t.ntiles[d];
        a.ntiles[g] = nt;
        int l = 0;
        while ((1ull << l) < nt) ++l;
        a.div_m[g] = (uint32_t)((((1ull << 32) * ((1ull << l) - nt)) / nt) + 1);
        a.div_s[g] = (uint32_t)l;
        a.gdims[g] = c.dims[d];
        a.glog[g] = tlogdim[d];
        if (c.dims[d] & (((i64)1 << tlogdim[d]) - 1)) a.last_ragged[g] = nt - 1;
    }
    for (int j = 0; j < t.nt; ++j) {
        a.tlog[j] = t.tlog[j];
        int g = gof[t.tdim[j]];
        if (g < 0 && (c.dims[t.tdim[j]] & (((i64)1 << t.tlog[j]) - 1))) {
            // a tiled dim covered by a single, partly empty tile: give it a one-tile grid slot so
            // that every workgroup takes the bounds-checked path
            if (ng >= MAXN) return set_error(SMR_EUNSUPPORTED, "tiled: too many grid dims");
            g = ng++;
            a.gdims[g] = c.dims[t.tdim[j]];
            a.glog[g] = t.tlog[j];
            a.last_ragged[g] = 0;  // tc == 0 always
        }
        a.tgrid[j] = g;
    }
    for (int j = 0; j < MAXT; ++j) {
        a.ej_g[j] = -1;
        a.ej_ntm1[j] = 0;
        a.ej_last[j] = 0x7fffffffu;
        if (j < t.nt && a.tgrid[j] >= 0) {
            const i64 ext = c.dims[t.tdim[j]], tile = (i64)1 << t.tlog[j], nt = (ext + tile - 1) / tile;
            a.ej_g[j] = a.tgrid[j];
            a.ej_ntm1[j] = (uint32_t)(nt - 1);
            a.ej_last[j] = (uint32_t)(ext - (nt - 1) * tile);  // 1 .. tile (a whole last tile keeps every lane: lim = tile)
        }
    }
    a.ng = ng;
    // 32-bit tile-origin arithmetic when every operand's tile origins stay below 4 GiB (plan_tiles; tiled_variant picks variant 7 otherwise)
    a.base32 = t.origins32 ? 1 : 0;
    if (LEAN && (!t.origins32 || ng > NG)) return set_error(SMR_EINVAL, "tiled: a lean variant was picked for a plan without 32-bit tile origins");

    // per-lane table: one row per operand and lane
    std::vector<LaneRow<WIDE>>& rows = out.rows;
    rows.assign((size_t)c.M * NT, LaneRow<WIDE>{});

    for (int k = 0; k < MAXM; ++k) a.staged[k] = -1;
    for (int k = 0; k < c.M; ++k) {
        const bool own = k > 0 && t.staged[k] >= 0;
        OpDesc<WIDE>& d = a.op[k];
        const i64 es = c.esize[k];
        a.staged[k] = own ? t.staged[k] : -1;
        d.dtype = c.dtype[k];
        d.conj = c.conj[k];
        for (int dd = 0; dd < c.N; ++dd)
            if (gof[dd] >= 0) {
                const i64 st = c.strides[k][dd] * ((i64)1 << tlogdim[dd]) * es;
                a.tstep[k][gof[dd]] = st;
                if (gof[dd] < NG) d.tstep32[gof[dd]] = (uint32_t)st;
            }
        // per-bit contributions in this operand's enumeration order
        i64 gbit[32] = {0};
        uint32_t lbit[32] = {0};
        int pos = 0;
        for (int jj = 0; jj < t.nt; ++jj) {
            const int j = own ? t.order[k][jj] : jj;
            a.esh[k][j] = pos;
            for (int bit = 0; bit < t.tlog[j]; ++bit) {
                gbit[pos + bit] = c.strides[k][t.tdim[j]] * ((i64)1 << bit) * es;
                lbit[pos + bit] = swz.apply(1u << (lsh[j] + bit));
            }
            pos += t.tlog[j];
        }
        for (int h = 0; h < V; ++h) {
            uint32_t l = 0;
            for (int bit = 0; bit < vlog; ++bit)
                if ((h >> bit) & 1) l ^= lbit[bit];
            d.Lh[h] = l;
        }
        for (int r = 0; r < NREP; ++r) {
            i64 g = 0;
            uint32_t l = 0;
            for (int bit = 0; bit < 5; ++bit)
                if ((r >> bit) & 1) {
                    g += gbit[vlog + THRLOG + bit];
                    l ^= lbit[vlog + THRLOG + bit];
                }
            d.Gr[r] = (O)g;
            d.Lr[r] = l;
        }
        for (int tid = 0; tid < NT; ++tid) {
            i64 g = 0;
            uint32_t l = 0;
            for (int bit = 0; bit < THRLOG; ++bit)
                if ((tid >> bit) & 1) {
                    g += gbit[vlog + bit];
                    l ^= lbit[vlog + bit];
                }
            rows[(size_t)k * NT + tid].g = (O)g;
            rows[(size_t)k * NT + tid].l = l;
        }
    }
    for (int r = 0; r < NREP; ++r) a.Lrd[r] = a.op[0].Lr[r];
    for (int h = 0; h < V; ++h) a.Lhd[h] = a.op[0].Lh[h];
    return SMR_OK;
}

template int build_tiled_args<false>(const Plan&, int, const TiledVariant&, TiledBuild<false>&);
template int build_tiled_args<true>(const Plan&, int, const TiledVariant&, TiledBuild<true>&);

}  // namespace smr
