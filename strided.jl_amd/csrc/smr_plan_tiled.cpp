// smr_plan_tiled.cpp -- FAM_TILED: tile shape (plan_tiles), tile orders, the variant a launch takes (tiled_variant)
#include "smr_plan.h"

namespace smr {

// fast (unit-stride) axis of operand k, or -1
static int fast_axis(const Canon& c, int k) {
    for (int i = 0; i < c.N; ++i)
        if (c.dims[i] > 1 && (c.strides[k][i] == 1 || c.strides[k][i] == -1)) return i;
    return -1;
}

// When several inputs are differently permuted views of ONE buffer (B .= (A .+ A')./2, the 4-way
// permuted sum), the tiles T, pi(T), pi^2(T), ... read the same regions of that buffer.  In natural tile order every XCD
// (smr_plan.h: NXCD) fetches every region it touches by itself: the buffer crosses the fabric once per permutation.  Here the
// tiles are grouped into super-tiles whose extents are invariant under the permutations, the super-tiles into orbits of the
// permutation group, and the orbit-major list is dealt out in one contiguous run per XCD (deal_per_xcd): the members of an
// orbit meet in one L2 at about the same time.
static void plan_tile_order(const Canon& c, TilePlan& t, const int* lg) {
    if (t.grid < 2 * NXCD || t.grid > ((i64)1 << 22)) return;
    // generators: input k reads through strides that are a permutation of input j's
    std::vector<std::array<int, MAXN>> gens;
    for (int j = 1; j < c.M; ++j)
        for (int k = j + 1; k < c.M; ++k) {
            if (c.esize[j] != c.esize[k] || !same_buffer(c, j, k)) continue;
            std::array<int, MAXN> pi;
            if (!stride_permutation(c, j, k, pi.data(), true)) continue;
            bool ident = true;
            for (int d = 0; d < c.N; ++d) ident = ident && pi[d] == d;
            if (!ident) gens.push_back(pi);
        }
    if (gens.empty()) return;
    // super-tile extents: equal along every cycle of every generator
    // (measured: widening the super-tiles to a full 128-B line along every permuted dim does not help)
    int E[MAXN];
    for (int d = 0; d < c.N; ++d) E[d] = lg[d];
    for (bool changed = true; changed;) {
        changed = false;
        for (const auto& pi : gens)
            for (int d = 0; d < c.N; ++d) {
                const int m = std::max(E[d], E[pi[d]]);
                if (E[d] != m || E[pi[d]] != m) {
                    E[d] = E[pi[d]] = m;
                    changed = true;
                }
            }
    }
    i64 edge[MAXN];  // of a super-tile, in tiles
    for (int d = 0; d < c.N; ++d) edge[d] = (i64)1 << (E[d] - lg[d]);
    const CellGrid super(t.ntiles, edge, c.N);
    // orbits of super-tile coordinates (breadth first), largest orbits first
    std::vector<char> seen((size_t)super.cells.count, 0);
    std::vector<std::vector<uint32_t>> orbits;
    for (i64 s0 = 0; s0 < super.cells.count; ++s0) {
        if (seen[(size_t)s0]) continue;
        std::vector<uint32_t> orb{(uint32_t)s0};
        seen[(size_t)s0] = 1;
        for (size_t head = 0; head < orb.size(); ++head) {
            i64 sc[MAXN], sp[MAXN];
            super.cells.decode(orb[head], sc);
            for (const auto& pi : gens) {
                // input k at box coordinate sc touches what input j touches at sp, sp[pi[d]] = sc[d]
                for (int d = 0; d < c.N; ++d) sp[pi[d]] = sc[d];
                const i64 id = super.cells.encode(sp);
                if (!seen[(size_t)id]) {
                    seen[(size_t)id] = 1;
                    orb.push_back((uint32_t)id);
                }
            }
        }
        orbits.push_back(std::move(orb));
    }
    std::stable_sort(orbits.begin(), orbits.end(), [](const std::vector<uint32_t>& a, const std::vector<uint32_t>& b) { return a.size() > b.size(); });
    // orbit by orbit, its members one after the other (interleaving them measured the same), a super-tile's tiles in natural order
    const Radix tiles(t.ntiles, c.N);
    std::vector<uint32_t> list;
    list.reserve((size_t)t.grid);
    for (const auto& orb : orbits)
        for (uint32_t sid : orb) super.for_each_in_cell(sid, [&](const i64* tc) { list.push_back((uint32_t)tiles.encode(tc)); });
    if ((i64)list.size() != t.grid) return;  // cannot happen; keep the natural order if it does
    deal_per_xcd(list.data(), list.size(), 1, t.ord, IDLE_TILE);
    t.ord_groups = (int)orbits.size();
}

// Block order for inputs that are DISTINCT arrays with different unit axes (no orbit structure to exploit): the
// tiles that run at the same time form compact blocks (blk tiles along every tiled dim) instead of a slab that is
// long along dim 0 only, so that every operand -- whatever its unit axis -- has its 32-/64-byte runs completed to
// longer contiguous pieces by tiles that are in flight together (DRAM row locality; option "tile_block").
// blk < 0: run-balanced blocks -- along every dim the block is as many tiles long as it takes for the operand whose unit
// axis that dim is to see ~256 contiguous bytes (a 16 x 8 x 8 x 4 Float64 tile: 2 x 4 x 4 x 8 tiles), about 256 tiles in all.
static void plan_block_order(const Canon& c, TilePlan& t, const int* lg, int blk, bool xcd_runs) {
    if (blk == 0 || blk == 1 || t.grid < 64 || t.grid > ((i64)1 << 22)) return;
    i64 bd[MAXN];
    const int es = elem_bytes(c);
    for (int d = 0; d < c.N; ++d) bd[d] = blk > 0 ? blk : 1;
    if (blk < 0) {
        i64 prod = 1;
        for (int d = 0; d < c.N; ++d) {
            bool unit = false;
            for (int k = 0; k < c.M; ++k)
                if (c.strides[k][d] == 1 || c.strides[k][d] == -1) unit = true;
            if (unit) bd[d] = std::max<i64>(1, 256 / (((i64)es) << lg[d]));
            bd[d] = std::min<i64>(bd[d], t.ntiles[d]);
            prod *= bd[d];
        }
        for (int guard = 0; prod < 192 && guard < 32; ++guard) {  // fill up to about 256 tiles: grow the shortest extents first
            int best = -1;
            for (int d = 0; d < c.N; ++d)
                if (bd[d] < t.ntiles[d] && (best < 0 || (bd[d] << lg[d]) < (bd[best] << lg[best]))) best = d;
            if (best < 0) break;
            prod = prod / bd[best] * std::min<i64>(bd[best] * 2, t.ntiles[best]);
            bd[best] = std::min<i64>(bd[best] * 2, t.ntiles[best]);
        }
    }
    // block by block, the tiles of a block in natural order
    const CellGrid blocks(t.ntiles, bd, c.N);
    const Radix tiles(t.ntiles, c.N);
    std::vector<uint32_t> list;
    list.reserve((size_t)t.grid);
    for (i64 b = 0; b < blocks.cells.count; ++b) blocks.for_each_in_cell(b, [&](const i64* tc) { list.push_back((uint32_t)tiles.encode(tc)); });
    if ((i64)list.size() != t.grid) return;
    if (xcd_runs) {  // one contiguous run of the list per XCD (a block then meets in ONE L2)
        deal_per_xcd(list.data(), list.size(), 1, t.ord, IDLE_TILE);
    } else {  // round-robin over the XCDs: the list as it is
        while (list.size() % NXCD) list.push_back(IDLE_TILE);
        t.ord = std::move(list);
    }
    t.ord_groups = (int)blocks.cells.count;
}

// the dim along which operand k's memory continues after a (short) dim 0: stride == extent of dim 0, or -1
static int continuation_of_dim0(const Canon& c, int k) {
    if (c.strides[k][0] != 1) return -1;
    for (int d = 1; d < c.N; ++d)
        if (c.dims[d] > 1 && std::llabs(c.strides[k][d]) == c.dims[0]) return d;
    return -1;
}

// A short common unit axis (a physical index of 2..4, the colour channel of an image) with operands that continue
// along DIFFERENT dims behind it -- permutedims of (2,128,128) to (1,3,2) -- is a transposition one level up: rows
// of dims[0] elements are all the STREAM family would move.  Such inputs are staged like transposed ones.
bool short_dim0_transposition(const Canon& c, int k, int es) {
    if (c.N < 3 || c.dims[0] * es >= 64 || c.strides[0][0] != 1 || c.strides[k][0] != 1) return false;
    const int d0 = continuation_of_dim0(c, 0), dk = continuation_of_dim0(c, k);
    return d0 > 0 && dk > 0 && d0 != dk;
}

// The dim along which operand k's memory advances least: its unit-stride dim, or -- a stepped range, A[1:3:end, :] seen through a
// permutation -- a dim whose step is 2..4 elements: lanes laid along it still share cache lines (a third of each at step 3), where
// lanes laid along the destination's dim 0 would touch one line each (round 4; `step-3 cols transpose-add` 0.6 TB/s in r2 / r3).
static int near_axis(const Canon& c, int k) {
    int q = fast_axis(c, k);
    if (q >= 0) return q;
    i64 best = 5;
    for (int i = 0; i < c.N; ++i) {
        const i64 s = std::llabs(c.strides[k][i]);
        if (c.dims[i] > 1 && s >= 2 && s < best) {
            best = s;
            q = i;
        }
    }
    return q;
}

bool plan_tiles(const Canon& c, TilePlan& t) {
    if (c.redop != SMR_RED_NONE) return false;
    if (c.N < 2 || c.strides[0][0] != 1) return false;
    const int es = elem_bytes(c);
    // which inputs need staging: unit-stride axis exists and differs from the destination's
    bool axis_used[MAXN] = {false};
    axis_used[0] = true;
    int nst = 0;
    t.staged[0] = -1;
    for (int k = 1; k < c.M; ++k) {
        int q = near_axis(c, k);
        t.staged[k] = -1;
        if (q > 0 && c.strides[k][0] != 0 && std::llabs(c.strides[k][0]) != 1) {
            t.staged[k] = nst++;
            axis_used[q] = true;
        } else if (q == 0 && short_dim0_transposition(c, k, es)) {
            t.staged[k] = nst++;
            axis_used[continuation_of_dim0(c, 0)] = true;
            axis_used[continuation_of_dim0(c, k)] = true;
        }
        // (an input that is broadcast along dim 0 and has another unit axis stays direct: its reads are wave-uniform along dim 0 anyway)
    }
    if (nst == 0) return false;
    t.nstaged = nst;
    int axes[MAXN], na = 0;
    for (int i = 0; i < c.N; ++i)
        if (axis_used[i]) axes[na++] = i;
    // target contiguous run per axis
    const Options& o = options();
    i64 runbytes = (na == 2) ? 256 : (na == 3 ? 128 : 64);
    // The tiled kernel is specialised for 1024-element tiles (256 lanes x 4 elements): measured
    // on MI355X, 1024-element tiles beat 4096-element ones at 32^4 (more workgroups in flight)
    // and tie at 128^4.
    // Three or more distinct unit axes and a big problem: 4096-element tiles on 1024 threads (the
    // same 4 elements per lane) keep every operand's contiguous run at >= 64 B.  Measured on the
    // 4-way permuted sum: 32^4 8.0 vs 8.4 us, 64^4 141 vs 175 us, 128^4 3.24 vs 4.64 ms (needs at
    // least one big tile per CU).
    int tl_cap = 10;
    bool big_transpose = false;
    if (o.tile_log2 == 12) tl_cap = 12;
    // true-HBM sized transposes (two unit axes, >= 1 GiB moved, 8-/16-byte elements): 128 x 32 tiles on 1024 lanes --
    // 1-KiB non-temporal write runs along the destination's unit axis, 256-byte read runs along the source's.
    // Measured (tools/perm_tiles2.py, Float64): permutedims! 128^4 32x32 940, 64x64 798, 128x32 792 us; transposes
    // 16384^2 840 / 778 / 719 us, 8192^2 270 (218 persistent) / 215 / 206 us; sizes that are not powers of two
    // (4000^2, 12000^2) tie.  Float32 stays with 32 x 32 (128^4: 451 vs 480 / 535 us)
    else if (o.tile_log2 == 0 && na == 2 && nst == 1 && es >= 8 && (long double)c.total * es * 2 >= 1073741824.0L) {
        // ... only when the 128 x 32 tile is (nearly) filled: on 96^4 / 144^4 the 128-wide tile idles 25 / 44 % of its
        // lanes (round 3: 144^4 3.47 TB/s with it)
        auto util = [&](int d, i64 e) { return (long double)c.dims[d] / (long double)(((c.dims[d] + e - 1) / e) * e); };
        if (util(axes[0], 128) * util(axes[1], 32) >= 0.9L) {
            tl_cap = 12;
            runbytes = 32 * es;
            big_transpose = true;
        }
    }
    else if (o.tile_log2 == 0 && na >= 3 && (size_t)nst * 4096 * es <= (size_t)128 * 1024 && c.total >= (i64)4096 * 256) {
        bool fits = true;  // every axis must be able to reach its share of the 12 bits
        int bits = 0;
        for (int a = 0; a < na; ++a) bits += std::min(ceil_log2(c.dims[axes[a]]), 12);
        if (bits < 12) fits = false;
        // one round of big tiles (<= 256 CUs, 1024 lanes each) or a long persistent work list: big;
        // in between (measured 48^4: 25.8 vs 32.0 us, 64^4: 73.5 vs 83.3 us) several small workgroups per
        // CU overlap better than a few rounds of one big workgroup per CU
        const i64 nbig = c.total >> 12;
        // ... when the inputs are views of ONE buffer (they hit in L2).  DISTINCT arrays stream from HBM / the
        // Infinity Cache and want the longer runs of the big tiles much earlier (round 3, tools/cliff_ab.py, Float64:
        // A .+ perm(C) .* perm'(D) 48^4 35.7 -> 26.6 us, 64^4 117.8 -> 105.5 us; four arrays with four unit axes:
        // 64^4 177 -> 157 us, 96^4 888 -> 755 us together with the block order below, 48^4 stays with small tiles)
        bool one_buffer = false;
        for (int j = 1; j < c.M; ++j)
            for (int k = j + 1; k < c.M; ++k) one_buffer = one_buffer || same_buffer(c, j, k);
        if (one_buffer) {
            if (nbig > 256 && nbig < 8192) fits = false;
        } else if (nbig > 256 && nbig < (na >= 4 ? 2048 : 257)) {
            fits = false;
        }
        if (fits) tl_cap = 12;
    }
    if ((size_t)nst * ((size_t)1 << tl_cap) * es > std::max<size_t>((size_t)o.max_lds_bytes, tl_cap == 12 ? (size_t)128 * 1024 : 0)) return false;
    int lg[MAXN] = {0};
    int total = 0;
    // grow the axes round-robin towards the run target
    int want = std::max(1, ceil_log2(std::max<i64>(1, runbytes / es)));
    bool forced = false;
    for (int i = 0; i < c.N; ++i)
        if (o.tile_lg[i] >= 0) forced = true;
    if (forced) {  // tuning override: exact per-dim log2 extents
        for (int i = 0; i < c.N; ++i) {
            lg[i] = (int)std::max<i64>(0, o.tile_lg[i]);
            while (lg[i] > 0 && ((i64)1 << (lg[i] - 1)) >= c.dims[i]) --lg[i];
            total += lg[i];
        }
        tl_cap = total;
    }
    if (!forced && tl_cap == 12) {
        // big tiles: give the destination axis a full 128-B line first (stores and the direct
        // inputs then move whole lines; measured on the 4-way sum at 32^4: 16x8x8x4 7.7 us,
        // 16x8x4x8 7.6 us, 8x8x8x8 8.0 us), the other axes share the rest
        const int want0 = big_transpose ? 7 : std::max(1, ceil_log2(std::max<i64>(1, 128 / es)));
        while (lg[0] < want0 && ((i64)1 << lg[0]) < c.dims[0] && total < tl_cap) {
            ++lg[0];
            ++total;
        }
    }
    bool grew = !forced;
    while (grew && total < tl_cap) {
        grew = false;
        for (int a = 0; a < na && total < tl_cap; ++a) {
            int i = axes[a];
            if (i == 0 && tl_cap == 12 && lg[0] >= want) continue;  // already served above
            if (lg[i] < want && ((i64)1 << lg[i]) < c.dims[i]) {
                ++lg[i];
                ++total;
                grew = true;
            }
        }
    }
    // an operand whose unit axis is shorter than the run target (3 x H x W images, physical indices of 2..4 in front):
    // its memory run continues along the dim whose stride equals that extent -- grow that one before the
    // destination-order widening below (permutedims (3,1000,700) -> (700,1000,3): 256 x 4 tiles read 24-byte
    // runs, 32 x 8 x 4 tiles read 192-byte runs)
    if (!forced) {
        for (int k = 0; k < c.M; ++k) {
            if (k > 0 && t.staged[k] < 0) continue;
            const int q = (k == 0) ? 0 : fast_axis(c, k);
            if (q < 0 || ((i64)1 << lg[q]) < c.dims[q] || c.dims[q] >= ((i64)1 << want)) continue;
            int v = -1;
            for (int d = 0; d < c.N; ++d)
                if (d != q && std::llabs(c.strides[k][d]) == c.dims[q]) v = d;
            if (v < 0) continue;
            while (total < tl_cap && (c.dims[q] << lg[v]) < ((i64)1 << want) && ((i64)1 << lg[v]) < c.dims[v]) {
                ++lg[v];
                ++total;
            }
        }
    }
    // small problems / short axes: widen the tile with the remaining dims (destination order)
    // until a block has at least 1024 elements of work
    int minlog = forced ? 0 : tl_cap;
    for (int i = 0; i < c.N && total < minlog; ++i)
        while (total < minlog && ((i64)1 << lg[i]) < c.dims[i]) {
            ++lg[i];
            ++total;
        }
    if (total != 10 && total != 12) return false;  // smaller problems go to the generic family
    t.nt = 0;
    t.tilelog = total;
    for (int i = 0; i < c.N; ++i)
        if (lg[i] > 0) {
            if (t.nt >= 5) return false;
            t.tdim[t.nt] = i;
            t.tlog[t.nt] = lg[i];
            ++t.nt;
        }
    if (t.tdim[0] != 0) return false;
    // enumeration order per staged input: its own stride order over the tiled dims
    for (int k = 1; k < c.M; ++k) {
        int idx[MAXN];
        for (int j = 0; j < t.nt; ++j) idx[j] = j;
        if (t.staged[k] >= 0)
            std::stable_sort(idx, idx + t.nt, [&](int a, int b) {
                i64 sa = std::llabs(c.strides[k][t.tdim[a]]), sb = std::llabs(c.strides[k][t.tdim[b]]);
                // zero strides last: they do not move the address
                if ((sa == 0) != (sb == 0)) return sb == 0;
                return sa < sb;
            });
        for (int j = 0; j < t.nt; ++j) t.order[k][j] = idx[j];
    }
    for (int j = 0; j < t.nt; ++j) t.order[0][j] = j;
    t.threads = (total == 12) ? 1024 : 256;  // (2048 elements on 512 lanes measured: never the best)
    t.grid = 1;
    for (int i = 0; i < c.N; ++i) {
        i64 e = (i64)1 << lg[i];
        t.ntiles[i] = (c.dims[i] + e - 1) / e;
        t.grid *= t.ntiles[i];
    }
    t.lds_bytes = (size_t)nst * ((size_t)1 << total) * es;
    if (t.grid > 0x7fffffffLL) return false;
    // Order of the grid dims (which tile coordinate varies fastest with the workgroup id).  Canonical order = by destination
    // stride: consecutive workgroups continue the destination's memory.  For HBM-sized transposing copies whose input's unit axis is
    // cut into several tiles (permutedims!(B, A, (4,3,2,1)) of 128^4: 128 x 32 tiles, four tiles along A's rows of 1 KiB) the tile
    // index along THAT axis goes second: the ~512 workgroups resident at once then cover whole rows of the input as well as
    // contiguous runs of the destination, instead of quarter rows of four different input rows -- tools/xpose_proto.hip: 843 -> 723
    // us for the same tile shape.  In the library (tools/gorder_ab.py, profiles/r05_gorder_ab.txt, Float64): 144^4 (4,3,2,1) 1336 ->
    // 1182 us, (256,128,128,64) reversed 879 -> 811, (64,64,64,64,16) reversed 834 -> 791, Float32 128^4 457 -> 434; neutral for 2-D
    // transposes and when the input's axis is one tile; so: every transposing copy of >= 512 MiB with one staged input and rank >= 3.
    for (int i = 0; i < MAXN; ++i) t.gorder[i] = i < c.N ? i : -1;
    {
        const i64 mode = o.tiled_gorder;
        const bool big = c.algbytes >= ((i64)512 << 20);
        if ((mode > 0 || (mode < 0 && big && na == 2 && nst == 1)) && c.N >= 3) {
            // staged inputs' unit axes that are tiled AND split into several tiles, moved to position 1 (behind the fastest grid dim)
            int order[MAXN], n = 0, first = -1;
            for (int d = 0; d < c.N; ++d)
                if (t.ntiles[d] > 1) {
                    first = d;
                    break;
                }
            if (first >= 0) {
                order[n++] = first;
                for (int k = 1; k < c.M; ++k) {
                    if (t.staged[k] < 0) continue;
                    const int q = fast_axis(c, k);
                    if (q >= 0 && q != first && lg[q] > 0 && t.ntiles[q] > 1) {
                        bool have = false;
                        for (int i = 0; i < n; ++i) have = have || order[i] == q;
                        if (!have) order[n++] = q;
                    }
                }
                for (int d = 0; d < c.N; ++d) {
                    bool have = false;
                    for (int i = 0; i < n; ++i) have = have || order[i] == d;
                    if (!have) order[n++] = d;
                }
                for (int i = 0; i < c.N; ++i) t.gorder[i] = order[i];
            }
        }
    }
    t.ord.clear();
    t.ord_groups = 0;
    if (o.tile_order) plan_tile_order(c, t, lg);
    // 128 x 32 transposing tiles run one-shot: measured round 3 (tools/perm_block_ab.py, Float64) permutedims! 128^4
    // 826 -> 791 us, (2,3,4,1) 866 -> 745 us, (3,4,1,2) 801 -> 699 us, transpose 16384^2 859 -> 719 us, 8192^2 / 12000^2 tie
    t.no_persist = big_transpose;
    if (t.ord.empty() && na >= 3 && o.tile_block != 0 && (o.tile_block > 0 || o.tile_block == -2 || t.grid >= 1024)) {
        // one contiguous run of the list per XCD while the operands fit the Infinity Cache (a block's partner pieces meet in ONE
        // L2: 48^4 45.0 -> 38.5 us); round-robin once they stream from HBM (64^4: 157 vs 175 us)
        const bool xcd_runs = o.tile_block_xcd > 0 || (o.tile_block_xcd < 0 && c.algbytes <= ((i64)256 << 20));
        plan_block_order(c, t, lg, o.tile_block > 0 ? (int)o.tile_block : (o.tile_block == -2 ? -1 : 4), xcd_runs);
        t.no_persist = t.no_persist || !t.ord.empty();  // measured: the one-shot form wins on block-ordered lists (128^4: 2715 vs 2773 us)
    }
    if (!t.ord.empty())  // work lists hold linear tile ids in canonical grid order
        for (int i = 0; i < MAXN; ++i) t.gorder[i] = i < c.N ? i : -1;
    // 32-bit tile-origin arithmetic over at most TILED_NG grid dims (the lean kernels): grid dims are the dims with more than one tile
    // plus one slot per tiled dim that is a single, partly empty tile; every operand's tile origins stay below 4 GiB
    int ng = 0;
    for (int d = 0; d < c.N; ++d)
        if (t.ntiles[d] > 1) ++ng;
    for (int j = 0; j < t.nt; ++j)
        if (t.ntiles[t.tdim[j]] <= 1 && (c.dims[t.tdim[j]] & (((i64)1 << t.tlog[j]) - 1))) ++ng;
    t.origins32 = ng <= TILED_NG;
    for (int k = 0; k < c.M && t.origins32; ++k) {
        long double span = 0;
        for (int d = 0; d < c.N; ++d) {
            if (t.ntiles[d] <= 1) continue;
            if (c.strides[k][d] < 0) t.origins32 = false;
            span += (long double)c.strides[k][d] * c.esize[k] * (long double)(t.ntiles[d] - 1) * (long double)((i64)1 << lg[d]);
        }
        if (span >= 4294967296.0L) t.origins32 = false;
    }
    return true;
}

TiledVariant tiled_variant(const Plan& plan, void* const* bases, int esize, bool mixed) {
    const Canon& c = plan.c;
    const TilePlan& t = plan.tile;
    const Options& o = options();
    TiledVariant v;
    // always 4 elements per lane: 1024-element tiles on 256 lanes, 4096-element tiles on 1024 lanes.
    // Measured alternatives (32^4 f64): 2048/4096-element tiles on 256 lanes are 10-40 % slower.
    v.thrlog = t.tilelog - 2;
    // 32-bit within-tile byte offsets when every tiled stride is >= 0 and the tile spans < 4 GiB
    for (int k = 0; k < c.M && !v.wide; ++k) {
        long double span = 0;
        for (int j = 0; j < t.nt; ++j) {
            const i64 st = c.strides[k][t.tdim[j]];
            if (st < 0) v.wide = true;
            span += (long double)st * (((i64)1 << t.tlog[j]) - 1) * c.esize[k];
        }
        if (span >= 4294967296.0L) v.wide = true;
    }
    // a lane's 4 elements as 16-byte vectors (8-byte for 1/2-byte element types): can every operand be accessed V elements at a time?
    // `whole`: aligned vectors, every extent and stride a multiple of V.  Else at element alignment (round 6): odd extents, odd row
    // strides, views that begin inside a vector.  Every operand still runs along its unit axis; the one partial vector at the end of a
    // row (extent not a multiple of V) is moved element by element by the workgroups of the ragged last tile.  Elements of 4 or 8 bytes.
    if (!v.wide && !mixed && esize < 16 && o.tiled_vec) {
        const int V = 16 / esize > 4 ? 4 : 16 / esize;
        int vlog = 0;
        while ((1 << vlog) < V) ++vlog;
        bool whole = V > 1, ua = V > 1 && o.tiled_uavec && esize >= 4;
        for (int k = 0; k < c.M && (whole || ua); ++k) {
            const bool staged = k > 0 && t.staged[k] >= 0;
            const int j0 = staged ? t.order[k][0] : 0;  // first axis of this operand's enumeration
            const int d0 = t.tdim[j0];
            const uintptr_t base = (uintptr_t)(bases ? bases[c.orig[k]] : c.base[k]) + (uintptr_t)(c.offsets[k] * (i64)c.esize[k]);
            // a direct input that is not unit-stride along dim 0 (broadcast, odd stride) has no V-wide form
            if (t.tlog[j0] < vlog || c.strides[k][d0] != 1) whole = ua = false;
            if (c.dims[d0] % V || base % ((size_t)V * esize)) whole = false;
            for (int d = 0; d < c.N && whole; ++d)
                if (d != d0 && (c.strides[k][d] % V)) whole = false;
            if (c.dims[d0] < V || base % esize) ua = false;
        }
        if (whole || ua) {
            v.V = V;
            v.ua = !whole;
        }
    }
    bool ragged = false;
    for (int j = 0; j < t.nt; ++j)
        if (c.dims[t.tdim[j]] & (((i64)1 << t.tlog[j]) - 1)) ragged = true;
    // ragged extents: the lean kernel plus bounds checks in the workgroups that sit on a last, partly filled tile (round 6; every
    // ragged problem used to take variant 7 -- lane tables from memory, 64-bit origins, order lookups -- and paid ~2 us for it:
    // transposes of 7200 x 100 Float64 5.4 us against 3.0 us for 7200 x 128, profiles/r06_ragged_tiles.txt)
    bool pv = false;  // does some operand's vector axis end in a partial vector?
    if (v.V > 1)
        for (int k = 0; k < c.M; ++k) {
            const int j0 = (k > 0 && t.staged[k] >= 0) ? t.order[k][0] : 0;
            if (c.dims[t.tdim[j0]] % v.V) pv = true;
        }
    if (ragged) v.mode = !t.ord.empty() ? 7 : (pv ? 9 : 1);
    else v.mode = t.ord.empty() ? 0 : 2;
    if (!t.origins32) v.mode = 7;  // the lean variants (MODE & 4 == 0) assume 32-bit tile origins over at most TILED_NG grid dims
    // persistent, software-pipelined form when the work list is longer than the machine holds at once
    if ((v.mode & 1) == 0 && o.tiled_persist && !t.no_persist && !v.ua) {  // (the persistent form keeps aligned vector accesses)
        const size_t lds = (size_t)t.nstaged * ((size_t)1 << t.tilelog) * esize;
        const i64 grid = t.ord.empty() ? t.grid : (i64)t.ord.size();
        i64 wpc = std::min<i64>(2048 >> v.thrlog, lds ? (i64)(160 * 1024 / lds) : 8);
        wpc = std::max<i64>(1, std::min<i64>(wpc, 4));  // measured: 4 workgroups per CU beat 8 and 2
        if (o.tiled_persist_wpc > 0) wpc = o.tiled_persist_wpc;
        const i64 cap = (i64)cu_count() * wpc / 8 * 8;
        if ((i64)(unsigned)grid >= cap * o.tiled_persist_min && cap >= 8) v.pgrid = (unsigned)cap;
    }
    return v;
}

}  // namespace smr
