// smr_plan_orbit.cpp -- planner of FAM_ORBIT.
#include "smr_plan.h"

namespace smr {

// B .= (A .+ A')./2, the 4-way permuted sum, ... : every input is a permuted view of ONE buffer.  The
// classic tiled kernel reads that buffer once per view (through L1: 4 x 8 MiB for the 4-way sum at 32^4);
// here the workgroup that owns a tile also owns its images under the permutation group, loads the buffer
// on those tiles once (natural order, full vectors) and serves every view from LDS.  Measured on MI355X
// (tools/c3_proto.hip, 4-way sum f64): 32^4 6.6 -> 4.7 us, 64^4 83 -> 46 us, 128^4 1.73 -> 1.41 ms.

// Step 1, the group.  On success: one buffer and one element type; o.k0 is the identity view (the destination's strides, positive and distinct);
// o.pdim[k] is pi_k; o.gdim / o.slot hold the group G the pi_k generate (identity first, 2 <= |G| = o.ng <= MAXG) and its multiplication table.
static bool orbit_group(const Canon& c, OrbitPlan& o) {
    // one buffer, one element type
    for (int k = 2; k < c.M; ++k)
        if (c.dtype[k] != c.dtype[1] || !same_buffer(c, k, 1)) return false;
    if (c.dtype[0] != c.dtype[1]) return false;
    // identity view: an input with exactly the destination's strides
    o.k0 = -1;
    for (int k = 1; k < c.M && o.k0 < 0; ++k) {
        bool same = true;
        for (int d = 0; d < c.N; ++d) same = same && c.strides[k][d] == c.strides[0][d];
        if (same) o.k0 = k;
    }
    if (o.k0 < 0) return false;
    const i64* s = c.strides[o.k0];
    for (int d = 0; d < c.N; ++d) {
        if (s[d] <= 0) return false;
        for (int e = 0; e < d; ++e)
            if (s[e] == s[d]) return false;
    }
    for (int k = 1; k < c.M; ++k)
        if (!stride_permutation(c, o.k0, k, o.pdim[k], false)) return false;
    // the group they generate (closure under composition), identity first
    std::vector<std::array<int, MAXN>> G;
    std::array<int, MAXN> id;
    for (int d = 0; d < MAXN; ++d) id[d] = d;
    G.push_back(id);
    auto index_of_product = [&](int k, int a) {  // of pi_k o g_a in G; a new element joins G while there is room, else MAXG comes back
        std::array<int, MAXN> h = id;
        for (int d = 0; d < c.N; ++d) h[d] = o.pdim[k][G[a][d]];
        const int at = (int)(std::find(G.begin(), G.end(), h) - G.begin());
        if (at == (int)G.size() && at < MAXG) G.push_back(h);
        return at;
    };
    for (int head = 0; head < (int)G.size(); ++head)
        for (int k = 1; k < c.M; ++k)
            if (index_of_product(k, head) >= MAXG) return false;
    o.ng = (int)G.size();
    if (o.ng < 2) return false;
    for (int a = 0; a < o.ng; ++a) {
        for (int d = 0; d < MAXN; ++d) o.gdim[a][d] = G[a][d];
        for (int k = 1; k < c.M; ++k) o.slot[a][k] = index_of_product(k, a);
        o.slot[a][0] = a;
    }
    return true;
}

// Step 2, the tile.  On success: o.lg / o.ntiles / o.tilelog describe cubes over the unit class that divide the box, fit LDS (o.lds_bytes) and
// hold >= 256 elements; at most 2^22 tiles; o.vec: 16-byte accesses apply; offsets inside a tile and of tile origins fit 32 bits.
static bool orbit_tile_edge(const Canon& c, OrbitPlan& o) {
    const Options& opt = options();
    const int es = dtype_size(c.ct);
    const i64* s = c.strides[o.k0];
    // the unit class: dims that are the unit-stride axis of some view
    bool unit[MAXN] = {false};
    int nu = 0;
    for (int a = 0; a < o.ng; ++a)
        if (!unit[o.gdim[a][0]]) {
            unit[o.gdim[a][0]] = true;
            ++nu;
        }
    // tile edge: the largest power of two that divides the unit dims, fits LDS and leaves enough orbits
    const i64 n0 = c.dims[0];
    i64 others = 1;
    for (int d = 0; d < c.N; ++d)
        if (!unit[d]) others *= c.dims[d];
    const int vmax = std::max(1, 16 / es);
    const int vlog = ceil_log2(vmax);
    // 16-byte accesses need aligned operands and vector-multiple strides; element-wise tiles stay <= 1024 elements
    bool vec_ok = vmax > 1;
    for (int d = 1; d < c.N; ++d)
        if (s[d] % vmax) vec_ok = false;
    if ((((uintptr_t)c.base[0] + (uintptr_t)(c.offsets[0] * c.esize[0])) | ((uintptr_t)c.base[o.k0] + (uintptr_t)(c.offsets[o.k0] * c.esize[o.k0]))) % 16) vec_ok = false;
    const int maxbits = (vmax > 1 && !vec_ok) ? 10 : 12;
    // LDS: the launch pads a group of order 3 to four slots; "max_lds_bytes" can raise (never lower) the 128 KiB cap
    const size_t slots = o.ng == 3 ? 4 : (size_t)o.ng;
    int best = -1;
    for (int l = maxbits / nu; l >= 1; --l) {
        if (n0 & (((i64)1 << l) - 1)) continue;
        if (slots * ((size_t)es << (l * nu)) > std::min<size_t>((size_t)160 * 1024, std::max<size_t>((size_t)opt.max_lds_bytes, (size_t)128 * 1024))) continue;
        if (((i64)es << l) < opt.orbit_minrun || l < vlog) continue;  // runs of at least 32 bytes (option orbit_minrun)
        if (l * nu < 8) continue;                        // at least 256 elements per tile (128 lanes x 16 B)
        if (opt.orbit_lg >= 0) {
            if (l == opt.orbit_lg) best = l;
            continue;
        }
        i64 tiles = others;
        for (int u = 0; u < nu; ++u) tiles *= n0 >> l;
        best = l;  // the smallest admissible edge when no edge yields orbit_min orbits
        if (tiles / o.ng >= opt.orbit_min) break;
        // a handful of big workgroups loses against the classic kernel's many small ones (measured: 24^4 f32,
        // 20 orbits of 8^4: 3.96 vs 3.38 us)
        if (l == 1 || (((i64)es << (l - 1)) < opt.orbit_minrun) || l - 1 < vlog || (l - 1) * nu < 8)
            if (tiles / o.ng < opt.orbit_few) best = -1;
    }
    if (best < 0) return false;
    o.tilelog = best * nu;
    o.ntiles_total = 1;
    for (int d = 0; d < MAXN; ++d) {  // (dims >= N: one tile of extent 1)
        o.lg[d] = unit[d] ? best : 0;
        o.ntiles[d] = d < c.N ? c.dims[d] >> o.lg[d] : 1;
        o.ntiles_total *= o.ntiles[d];
    }
    if (o.ntiles_total > ((i64)1 << 22)) return false;
    // 16-byte accesses: every non-unit stride a multiple of the vector (alignment is re-checked at launch)
    o.vec = vec_ok ? vmax : 1;
    o.lds_bytes = slots * ((size_t)es << o.tilelog);
    // 32-bit byte offsets inside a tile
    long double span = 0;
    for (int d = 0; d < c.N; ++d) span += (long double)(((i64)1 << o.lg[d]) - 1) * (long double)s[d] * es;
    if (span >= 2147483648.0L) return false;
    // slot origins travel as 32-bit element offsets
    long double last = 0;
    for (int d = 0; d < c.N; ++d) last += (long double)(c.dims[d] - 1) * (long double)s[d];
    return last < 4294967295.0L;
}

// the images g_a . t, a = 0 .. |G| - 1, of tile `id`, as linear tile ids
static void orbit_of(const OrbitPlan& o, const Radix& tiles, uint32_t id, uint32_t* out) {
    i64 tc[MAXN];
    tiles.decode(id, tc);
    for (int a = 0; a < o.ng; ++a) out[a] = (uint32_t)image_of(tc, o.gdim[a], tiles.mul, tiles.N);
}

// Step 3: o.list holds the root (smallest tile id) of every orbit of tile coordinates, super-cell by super-cell (2 tiles along every
// tiled dim: the partner halves of 64-B runs then meet in one XCD's L2 once the list is dealt out).
static void orbit_roots(OrbitPlan& o, const Radix& tiles, const CellGrid& cells) {
    std::vector<char> seen((size_t)o.ntiles_total, 0);
    o.list.clear();
    for (i64 cell = 0; cell < cells.cells.count; ++cell)
        cells.for_each_in_cell(cell, [&](const i64* t) {
            i64 root = tiles.encode(t);
            for (int a = 1; a < o.ng; ++a) root = std::min(root, image_of(t, o.gdim[a], tiles.mul, tiles.N));
            if (seen[(size_t)root]) return;
            seen[(size_t)root] = 1;
            o.list.push_back((uint32_t)root);
        });
    o.norbits = (int)o.list.size();
}

// The workgroups of the one-orbit form in list order: NS tile ids each, the slot map (OrbitPlan::wmap), and whether the workgroup holds
// ONE orbit of |G| distinct tiles with slot g = g_g . t (what the PAIR form can re-base)
struct WgList {
    int NS;
    std::vector<uint32_t> tile;
    std::vector<uint64_t> map;
    std::vector<char> full;
    void push(const uint32_t* t, uint64_t m, bool f) {
        tile.insert(tile.end(), t, t + NS);
        map.push_back(m);
        full.push_back(f ? 1 : 0);
    }
};
static unsigned field(int g, int k) { return (unsigned)((g * 8 + k) * 2); }  // of a slot map; k = input index - 1

// an orbit of n < |G| distinct tiles waiting for company: the tiles, and per tile the reads as indices into the orbit's own tiles
struct Part {
    uint32_t tile[MAXG];
    int rd[MAXG][MAXM];
    int n;
};

// the waiting orbits `pp` become one workgroup: their tiles side by side in its slots, every read re-based to where its orbit begins
static void emit_packed(const Canon& c, std::vector<Part>& pp, WgList& wgs) {
    if (pp.empty()) return;
    uint32_t tile[MAXG];
    uint64_t map = 0;
    int base = 0;
    for (const Part& q : pp) {
        for (int j = 0; j < q.n; ++j) {
            tile[base + j] = q.tile[j];
            for (int k = 1; k < c.M; ++k) map |= (uint64_t)(base + q.rd[j][k]) << field(base + j, k - 1);
        }
        base += q.n;
    }
    for (int g = base; g < wgs.NS; ++g) {  // an incomplete last workgroup: the free slots repeat slot 0 (identical values are stored twice)
        tile[g] = tile[0];
        for (int k = 1; k < c.M; ++k) map |= ((map >> field(0, k - 1)) & 3u) << field(g, k - 1);
    }
    wgs.push(tile, map, false);
    pp.clear();
}

// Step 4: every orbit of o.list is in exactly one workgroup of wgs: its tiles fill the LDS slots; orbits with fewer distinct tiles
// share a workgroup (option orbit_pack) as soon as enough of the same size have come by, the rest at the end.
static void orbit_workgroups(const Canon& c, const OrbitPlan& o, const Radix& tiles, WgList& wgs) {
    const int NS = wgs.NS;
    std::vector<Part> pending[MAXG + 1];  // by the number of distinct tiles
    for (uint32_t root : o.list) {
        uint32_t ids[MAXG];
        orbit_of(o, tiles, root, ids);
        int first[MAXG], ndist = 0, dix[MAXG];  // dix[a]: index of g_a . t among the distinct tiles
        for (int a = 0; a < o.ng; ++a) {
            dix[a] = -1;
            for (int b = 0; b < a && dix[a] < 0; ++b)
                if (ids[b] == ids[a]) dix[a] = dix[b];
            if (dix[a] < 0) {
                dix[a] = ndist;
                first[ndist++] = a;
            }
        }
        if (ndist == o.ng || !options().orbit_pack || NS / ndist < 2) {
            uint32_t tile[MAXG];
            uint64_t map = 0;
            for (int g = 0; g < NS; ++g) {
                const int a = g < o.ng ? g : 0;
                tile[g] = ids[a];
                for (int k = 1; k < c.M; ++k) map |= (uint64_t)o.slot[a][k] << field(g, k - 1);
            }
            wgs.push(tile, map, ndist == o.ng && NS == o.ng);
            continue;
        }
        Part q;
        q.n = ndist;
        for (int j = 0; j < ndist; ++j) {
            q.tile[j] = ids[first[j]];
            for (int k = 1; k < c.M; ++k) q.rd[j][k] = dix[o.slot[first[j]][k]];
        }
        pending[ndist].push_back(q);
        if ((int)pending[ndist].size() * ndist + ndist > NS) emit_packed(c, pending[ndist], wgs);
    }
    for (int sd = 1; sd <= MAXG; ++sd) emit_packed(c, pending[sd], wgs);
}

// Step 5, the PAIR form (4^4 cubes of 8-byte elements, |G| = 4, >= 16 workgroups; else o.pair_ok stays false): o.ptile / o.pmap hold two
// slot sets per workgroup, unit-axis neighbours first, one run per XCD; every workgroup of wgs is in exactly one set (an odd one out in two).
static void orbit_pairs(const Canon& c, OrbitPlan& o, const Radix& tiles, const CellGrid& cells, const WgList& wgs) {
    const int NS = wgs.NS;
    o.pair_ok = false;
    int ntd = 0;
    bool cubes = true;
    for (int d = 0; d < c.N; ++d)
        if (o.lg[d] > 0) {
            ++ntd;
            if (o.lg[d] != 2) cubes = false;
        }
    if (!(options().orbit_pair && o.ng == 4 && NS == 4 && ntd == 4 && cubes && o.tilelog == 8 && dtype_size(c.ct) == 8 && o.vec == 2 && o.lg[0] == 2 && wgs.map.size() >= 16)) return;
    std::vector<int> owner((size_t)o.ntiles_total, -1);
    for (size_t i = 0; i < wgs.map.size(); ++i)
        if (wgs.full[i])
            for (int g = 0; g < NS; ++g) owner[wgs.tile[i * NS + g]] = (int)i;
    std::vector<char> used(wgs.map.size(), 0);
    std::vector<uint32_t> pt;
    std::vector<uint64_t> pm;
    auto push_set = [&](const uint32_t* tile, uint64_t map) {
        pt.insert(pt.end(), tile, tile + NS);
        pm.push_back(map);
    };
    uint64_t stdmap = 0;
    for (int g = 0; g < NS; ++g)
        for (int k = 1; k < c.M; ++k) stdmap |= (uint64_t)o.slot[g][k] << field(g, k - 1);
    // super-cell by super-cell, in the cell's own tile order: the tile with an even unit-axis coordinate and its neighbour, both
    // taken as slot 0 of their orbits (any tile of a full orbit can be its slot 0: slot g = g_g . id) -- the eight pairs of a super-cell
    // then run back to back on one XCD and cover its four rotated images completely (pairing an orbit's smallest tile with whatever
    // sits next to it scattered the pairs: 4.72 us per launch against 4.27 with this list, tools/orbit16_probe.hip)
    for (i64 cell = 0; cell < cells.cells.count; ++cell)
        cells.for_each_in_cell(cell, [&](const i64* t) {
            if ((t[0] & 1) || t[0] + 1 >= o.ntiles[0]) return;
            const i64 id = tiles.encode(t);
            const int i = owner[(size_t)id], j = owner[(size_t)id + 1];  // (tiles.mul[0] == 1: the unit-axis neighbour is id + 1)
            if (i < 0 || j < 0 || i == j || used[(size_t)i] || used[(size_t)j]) return;
            uint32_t ta[MAXG], tb[MAXG];
            orbit_of(o, tiles, (uint32_t)id, ta);
            orbit_of(o, tiles, (uint32_t)id + 1, tb);
            push_set(ta, stdmap);
            push_set(tb, stdmap);
            used[(size_t)i] = used[(size_t)j] = 1;
        });
    std::vector<size_t> loose;
    for (size_t i = 0; i < wgs.map.size(); ++i)
        if (!used[i]) loose.push_back(i);
    for (size_t q = 0; q < loose.size(); q += 2) {  // what found no neighbour (diagonals, packed orbits): any two
        const size_t a = loose[q], b = loose[q + 1 < loose.size() ? q + 1 : q];  // an odd one out runs twice (same values stored twice)
        push_set(&wgs.tile[a * NS], wgs.map[a]);
        push_set(&wgs.tile[b * NS], wgs.map[b]);
    }
    deal_per_xcd(pt.data(), pm.size() / 2, (size_t)2 * NS, o.ptile, IDLE_TILE);
    deal_per_xcd(pm.data(), pm.size() / 2, (size_t)2, o.pmap, (uint64_t)0);
    o.pair_ok = true;
}

// The steps in order.  A failing step leaves o half written: make_plan calls this at most once per plan and reads plan.orbit on success only.
bool plan_orbit(const Canon& c, OrbitPlan& o) {
    const Options& opt = options();
    if (!opt.orbit) return false;
    if (c.redop != SMR_RED_NONE || c.mixed || c.bitcopy) return false;
    if (c.M < 3 || c.N < 2 || c.strides[0][0] != 1) return false;
    if (!orbit_group(c, o) || !orbit_tile_edge(c, o)) return false;
    // linear tile ids, and the super-cells (option orbit_group: tiles along every tiled dim) in which the lists are ordered
    const Radix tiles(o.ntiles, c.N);
    i64 sub[MAXN];
    for (int d = 0; d < c.N; ++d) sub[d] = (o.lg[d] > 0 && o.ntiles[d] > 1) ? std::max<i64>(1, std::min<i64>(opt.orbit_group, o.ntiles[d])) : 1;
    const CellGrid cells(o.ntiles, sub, c.N);
    orbit_roots(o, tiles, cells);
    o.nslots = o.ng == 3 ? 4 : o.ng;  // a group of order 3 runs in four slots (the fourth repeats the first)
    WgList wgs{o.nslots, {}, {}, {}};
    orbit_workgroups(c, o, tiles, wgs);
    orbit_pairs(c, o, tiles, cells, wgs);
    // one contiguous run of the workgroup list per XCD
    deal_per_xcd(wgs.tile.data(), wgs.map.size(), (size_t)o.nslots, o.wtile, IDLE_TILE);
    deal_per_xcd(wgs.map.data(), wgs.map.size(), (size_t)1, o.wmap, (uint64_t)0);
    return true;
}

int orbit_variant(const Plan& plan, void* const* bases, int esize, int native_nin, OrbitVariant& v) {
    const Canon& c = plan.c;
    const OrbitPlan& o = plan.orbit;
    v = OrbitVariant();
    auto addr = [&](int k) { return (uintptr_t)(bases ? bases[c.orig[k]] : c.base[k]) + (uintptr_t)(c.offsets[k] * (i64)c.esize[k]); };
    const int VMAX = 16 / esize > 1 ? 16 / esize : 1;
    bool vec = o.vec == VMAX && VMAX > 1;
    if (vec && ((addr(0) | addr(o.k0)) % 16)) vec = false;
    const int tile = 1 << o.tilelog;
    if (VMAX > 1) {
        if (vec) {
            v.V = VMAX;
            v.nrep = std::max(1, tile / (VMAX * 1024));
            if (v.nrep != 1 && v.nrep != 2) return set_error(SMR_EINVAL, "orbit: unexpected tile size");
        } else if (tile > 1024) {
            // element-wise accesses (operands not 16-byte aligned): only instantiated for tiles of up to 1024 elements
            return set_error(SMR_EUNSUPPORTED, "orbit plan: operands must be 16-byte aligned (rebind aligned pointers or create a new plan)");
        }
    } else {
        v.nrep = std::max(1, tile / 1024);
        if (v.nrep != 1 && v.nrep != 2 && v.nrep != 4) return set_error(SMR_EINVAL, "orbit: unexpected tile size");
    }
    v.own0 = true;  // is input 1 the identity view?
    for (int d = 0; d < c.N; ++d)
        if (o.pdim[1][d] != d) v.own0 = false;
    v.ng = o.ng == 2 ? 2 : 4;
    if (v.V == 2 && v.nrep == 1 && esize == 8 && native_nin >= 2 && native_nin <= 4) {
        // Write-through launches (store policy 2: recorded sequences, eager calls on library-owned streams) gain most -- every store
        // travels to the memory side on its own and 64-byte pieces pay: replay of the 4-way sum at 32^4 4.72 -> 4.31 us on one queue,
        // 3.66 -> 3.04 cut in two, bench step 5.65 -> 5.2 us -- plain-store launches through HIP 4.40 -> 4.27 us.  (With the first
        // work list -- an orbit's smallest tile paired with whatever sat next to it -- the form LOST through HIP, 4.72 us: the list
        // matters as much as the kernel, plan_orbit.)  orbit_pair = 0 switches the form off (tests, tools/cold_orbit_sweep.py).
        if (o.pair_ok && v.own0 && o.ng == 4 && c.M - 1 == native_nin && options().orbit_pair >= 1) {
            v.pair = true;
            return SMR_OK;
        }
    }
    // persistent pipelined form: when the LDS footprint leaves one workgroup per CU and every CU gets several orbits
    if (v.V * esize == 16) {
        const size_t lds = (size_t)v.ng * ((size_t)esize << o.tilelog);
        const i64 want = options().orbit_pipe;
        // at least 8 orbits per CU: with 4 (64^4) the pipelined ComplexF32 kernel -- 128 VGPRs, 20 bytes of scratch -- loses
        // (68.4 vs 47.6 us) and the Float64 one ties; from 80^4 on it gains 2-4 % (tools/orbit_cplx.py)
        v.pipe = want > 0 ? o.list.size() > 256 : (want < 0 && lds > 80 * 1024 && o.list.size() >= 8 * 256);
    }
    return SMR_OK;
}

}  // namespace smr
