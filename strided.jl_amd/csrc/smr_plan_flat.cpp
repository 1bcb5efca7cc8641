// smr_plan_flat.cpp -- planners of the three forms of FAM_FLAT.
#include "smr_plan.h"

namespace smr {

constexpr i64 FLAT_GROUP_MAX = 64;

// A unary transposing map in which one side's memory run consists of short leading dims with extents that are not powers of
// two (an image's 3 channels, a physical index of 3 in a tensor network): smr_k_flat.hip addresses that side through the
// flattened run.  side = 0: the destination is flat, 1: the input.
// The FLAT forms take ONE input with a layout of its own (it crosses LDS); any further input must have exactly the destination's
// strides (C .= beta .* C .+ alpha .* permutedims(A, p)).  Returns that input's operand index, or -1.
static int flat_transposed_input(const Canon& c) {
    int kt = -1;
    for (int k = 1; k < c.M; ++k) {
        bool same = true;
        for (int d = 0; d < c.N; ++d)
            if (c.strides[k][d] != c.strides[0][d]) same = false;
        if (same) continue;
        if (kt >= 0) return -1;
        kt = k;
    }
    return kt;
}

static bool plan_flat_side(const Canon& c, FlatPlan& f, int side, int es) {
    const int kf = side == 0 ? 0 : f.kt, kl = side == 0 ? f.kt : 0;
    const i64* sf = c.strides[kf];
    const i64* sl = c.strides[kl];
    // leading dim of the flat side
    int lead = -1;
    for (int d = 0; d < c.N; ++d)
        if (sf[d] == 1 && c.dims[d] > 1) lead = d;
    if (lead < 0) return false;
    const i64 e0 = c.dims[lead];
    // long or power-of-two leading dims: the tiled family's ground -- except (round 6, option flat_wide) whole rows of 65..128
    // elements whose byte length is not a multiple of the 128-byte line: there every 256-byte tile row of TILED is three partial
    // lines, while rows taken whole make the tile one contiguous, line-aligned piece of this side's memory
    // Measured (tools/ragged_family_ab.py, profiles/r06_flat_wide_ab.txt): this form's phases are loops of dependent loads, so at
    // 11 MiB it loses ((7200,100) 5.4 against 4.4 us) and it must not take leads of 65 elements away from the two-sided form
    // ((257,129,65) 13.3 against 9.9 us); on tall matrices of 32 MiB and more (per array) it wins: (100,100000) Float32 23.2 -> 15.1 us,
    // Float64 34.9 -> 28.5, (100000,100) Float32 21.9 -> 17.4.  flat_wide = 2 forces the form wherever it applies (tests).
    const i64 fw = options().flat_wide;
    const bool wide = fw && e0 * es >= 128 && e0 <= 128 && (e0 * es) % 128 != 0 && (fw >= 2 || (c.N == 2 && c.total * es >= ((i64)32 << 20)));
    if ((e0 * es >= 128 && !wide) || (e0 & (e0 - 1)) == 0) return false;
    // unit axis of the line side: not the lead ...
    int q = -1;
    for (int d = 0; d < c.N; ++d)
        if (d != lead && sl[d] == 1 && c.dims[d] * es >= 64) q = d;   // line-side runs of at least 64 bytes
    // ... or the lead itself, continued by a dim of stride e0: a transposition of e0-element groups ((3,W,H) -> (3,H,W))
    f.lshare = false;
    if (q < 0 && sl[lead] == 1) {
        for (int d = 0; d < c.N; ++d)
            if (d != lead && sl[d] == e0 && sf[d] != e0 && c.dims[d] * e0 * es >= 64) q = d;
        f.lshare = q >= 0;
    }
    if (q < 0) return false;
    if (!f.lshare && (sl[lead] == 1 || sl[lead] == -1)) return false;
    for (int d = 0; d < MAXN; ++d) f.ingroup[d] = false;
    f.ingroup[lead] = true;
    i64 R = e0;
    int p = -1;
    // take further contiguous dims whole while the run stays short, then tile the next one
    for (;;) {
        int nxt = -1;
        for (int d = 0; d < c.N; ++d)
            if (!f.ingroup[d] && d != q && sf[d] == R && c.dims[d] > 1) nxt = d;
        if (nxt < 0) break;
        if (!f.lshare && R * es < 192 && R * c.dims[nxt] <= FLAT_GROUP_MAX && R * c.dims[nxt] * es <= 512) {
            f.ingroup[nxt] = true;
            R *= c.dims[nxt];
            continue;
        }
        p = nxt;
        break;
    }
    if (R > (wide ? 128 : 64)) return false;
    int tplog = 0;
    if (p >= 0)
        while ((R << tplog) * es < 256 && ((i64)1 << tplog) < c.dims[p] && (R << (tplog + 1)) <= 128) ++tplog;
    const i64 L = R << tplog;
    // planar <-> interleaved (NCHW <-> NHWC with 3 channels): the flat side continues along q ITSELF
    f.fuse = p < 0 && sf[q] == R && !f.lshare;
    if (f.lshare && p < 0) return false;
    const int vmax = std::max(1, 16 / es);
    if (!f.fuse) {
        if (L * es < 96 || L > 128) return false;      // no run worth flattening
        if (L / vmax < 2) return false;
    }
    f.dir = side;
    f.R = (int)R;
    f.tplog = tplog;
    f.tqlog = es >= 8 ? 5 : 6;
    if (f.fuse) {  // the whole R x TQ tile is one run: up to 2048 elements per workgroup (3 channels: 512 pixels)
        f.tqlog = 5;
        while (f.tqlog < 9 && (R << (f.tqlog + 1)) <= 2048 && ((i64)1 << f.tqlog) < c.dims[q]) ++f.tqlog;
    }
    f.p = p;
    f.q = q;
    // line-side offsets of the leading index r (mixed radix over the group dims in flat-side stride order)
    std::vector<int> order;
    for (int d = 0; d < c.N; ++d)
        if (f.ingroup[d]) order.push_back(d);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return sf[x] < sf[y]; });
    for (i64 r = 0; r < R; ++r) {
        i64 rem = r, off = 0;
        for (int d : order) {
            off += (rem % c.dims[d]) * sl[d];
            rem /= c.dims[d];
        }
        if (off > 2147483647LL || off < -2147483647LL) return false;
        f.roff[r] = (int32_t)off;
    }
    return true;
}

bool plan_flat(const Canon& c, FlatPlan& f) {
    const Options& o = options();
    if (!o.flat || c.redop != SMR_RED_NONE || c.M < 2 || c.mixed || c.N < 2) return false;
    const int es = elem_bytes(c);
    if (es < 4) return false;
    f.kt = flat_transposed_input(c);
    if (f.kt < 0) return false;
    if (c.total < 65536) return false;  // small boxes: generic / tiled are fine and launch-bound anyway
    for (int d = 0; d < c.N; ++d)
        if (c.strides[0][d] <= 0) return false;
    return plan_flat_side(c, f, 0, es) || plan_flat_side(c, f, 1, es);
}

// Batched FLAT form: see FlatBPlan (smr_internal.h).  Conditions: one input; the destination's first g >= 2 dims are dense
// (strides 1, n0, n0 n1, ...) with P = n0 ... n_{g-1} <= 512 elements and at most 4 KiB; the input's strides over those dims are a
// dense layout of the same P elements in another order; dim g has stride P in the destination (consecutive blocks are adjacent
// there).  When the input's blocks follow one another the same way and the dims behind agree, a chunk is contiguous on both sides;
// otherwise (blocks of at least 256 bytes) the input side is read block by block.
bool plan_flatb(const Canon& c, FlatBPlan& f) {
    const Options& o = options();
    f.on = false;
    if (!o.flatb || !o.flat || c.redop != SMR_RED_NONE || c.M != 2 || c.mixed || c.N < 3) return false;
    const int es = elem_bytes(c);
    if (es < 4 || c.total < 65536) return false;
    if (c.strides[0][0] != 1) return false;
    // the longest dense destination prefix that stays within the size limits
    int g = 0;
    i64 P = 1;
    while (g < c.N - 1 && c.strides[0][g] == P && P * c.dims[g] <= FLATB_MAXP && P * c.dims[g] * es <= 4096) {
        P *= c.dims[g];
        ++g;
    }
    for (; g >= 2; P /= c.dims[g - 1], --g) {
        // the input over dims 0..g-1: a dense permutation of the same block?
        int ord[MAXN];
        for (int i = 0; i < g; ++i) ord[i] = i;
        std::sort(ord, ord + g, [&](int a, int b) { return c.strides[1][a] < c.strides[1][b]; });
        i64 run = 1;
        bool dense = true, moved = false;
        for (int i = 0; i < g && dense; ++i) {
            if (c.strides[1][ord[i]] != run) dense = false;
            run *= c.dims[ord[i]];
            if (ord[i] != i) moved = true;
        }
        if (!dense || !moved) continue;
        // blocks whose extents are all powers of two are TILED's home ground ((2,128,2,128,8) permutations: 2.6 us there, 4.0-5.5 here)
        bool pow2 = true;
        for (int i = 0; i < g; ++i)
            if (c.dims[i] & (c.dims[i] - 1)) pow2 = false;
        if (pow2) continue;
        // the destination's blocks follow one another along dim g; the input's blocks may sit anywhere (a batch grid that is permuted
        // as well: (9,11,300,300) -> (11,9,300',300)): its side then moves in whole blocks, which must not be tiny
        if (c.strides[0][g] != P) continue;
        bool same = c.strides[1][g] == P;
        for (int d = g + 1; d < c.N; ++d)
            if (c.strides[0][d] != c.strides[1][d]) same = false;
        if (!same && (P * es < 256 || c.strides[1][g] < P)) continue;
        f.g = g;
        f.P = (int)P;
        // K blocks per workgroup: about 4096 elements (32 KiB of Float64 in LDS), an even count so that 16-byte vectors line up
        i64 K = std::max<i64>(1, 4096 / P);
        K = std::min<i64>(K, c.dims[g]);
        if (K > 1) K &= ~(i64)1;
        f.K = (int)K;
        for (i64 r = 0; r < P; ++r) {
            i64 rem = r, off = 0;
            for (int d = 0; d < g; ++d) {
                off += (rem % c.dims[d]) * c.strides[1][d];
                rem /= c.dims[d];
            }
            f.srcoff[r] = (uint16_t)off;
        }
        f.on = true;
        return true;
    }
    return false;
}

// Two-sided FLAT form: the unit-stride dims of BOTH sides are short (under 256 bytes) and at least one of them is not a
// power of two (or under 32 bytes): no power-of-two tile fits either side -- (17,33,65,31) reversed runs a 32 x 32 tile over a
// 31 x 17 face with 51 % of its lanes.  Each side's run = its leading dims taken whole while the run stays short + a tile of the
// next contiguous dim, about flat2_bytes long; the runs share no dim (smr_k_flat.hip, flat2_body).
bool plan_flat2(const Canon& c, Flat2Plan& f) {
    const Options& o = options();
    f.on = false;
    if (!o.flat2 || !o.flat || c.redop != SMR_RED_NONE || c.M < 2 || c.mixed || c.N < 2) return false;
    const int es = elem_bytes(c);
    if (es < 4 || c.total < 65536) return false;
    f.kt = flat_transposed_input(c);
    if (f.kt < 0) return false;
    const i64* st[2] = {c.strides[0], c.strides[f.kt]};  // side 0 = destination, side 1 = the transposed input
    int lead[2] = {-1, -1};
    for (int s = 0; s < 2; ++s)
        for (int d = 0; d < c.N; ++d) {
            if (st[s][d] <= 0) return false;
            if (st[s][d] == 1 && c.dims[d] > 1) lead[s] = d;
        }
    if (lead[0] < 0 || lead[1] < 0 || lead[0] == lead[1]) return false;
    // Round 4: a LONG unit-stride dim that 32-wide power-of-two tiles fit badly (100 -> 3 x 32 + 4: a quarter of the last tile's lanes,
    // 257 -> 8 x 32 + 1) is cut EVENLY instead -- its side's run is then a tile of the unit dim itself (R = 1, p = the lead,
    // TP = extent / ceil(extent / ~48)): (100,90,80) -> tiles of 34 x 30, no lane idles.
    // Measured (tools/flat2_long_ab.py, profiles/r04_flat2_long_ab.txt, Float64): (257,129,65) 12.3-14.0 -> 9.5-10.1 us, (17,33,65,31)
    // (3,2,0,1) 9.0 -> 6.5 us, (999,1001) 7.2 -> 6.4 us; but (100,90,80) (6 MB) 5.5 -> 6.4 us and well-filled tiles ((200,300,70),
    // (1400,1500), (4000,4100), every power of two) stay ahead in TILED -- so: the padded tiles would be under flat2_long % full and
    // the array has at least 8 MiB, or the OTHER side's lead is short and awkward anyway.
    bool awkward = false, cutlead[2] = {false, false}, novec = false, odd_short = false;
    long double fill = 1;
    const i64 vlen = std::max<i64>(1, 16 / es);
    for (int s = 0; s < 2; ++s) {
        const i64 e = c.dims[lead[s]];
        if (e * es >= o.flat2_lead_bytes) {
            if (!o.flat2_long) return false;
            cutlead[s] = true;
            fill *= (long double)e / (long double)((e + 31) / 32 * 32);
            // (round 6: TILED keeps 16-byte accesses at element alignment -- (999,1001) Float64 5.7 us there against 6.45 here, Float32 4.6
            // against 6.1 -- but at 64 MiB this form is ahead again: (2049,2051) Float64 14.6 against 18.4 us)
            if (e % vlen && (!o.tiled_uavec || c.total * es >= ((i64)32 << 20))) novec = true;  // TILED then moves 4- / 8-byte elements one by one as well, in padded tiles: (999,1001) 7.2 -> 6.4 us
            continue;
        }
        if ((e & (e - 1)) != 0) awkward = odd_short = true;
        else if (e * es < 32) awkward = true;
    }
    if (cutlead[0] || cutlead[1]) {
        // next to a cut lead only a short lead that is NOT a power of two counts ((2,2,256,2,2,256) and (64,2,64,2,16) permutations with a
        // 16-byte lead beside a 2-KiB one: TILED 3.2-3.9 us, this form 6.9-7.1)
        const bool anysize = o.flat2_long >= 100;  // tests / experiments: wherever the form applies
        // (round 5: ... and under 1 GiB: at HBM size the padded 32 x 32 tiles win again -- permutedims!(4,3,2,1) of 136^4 Float64, 72 %
        // fill: 1562 us in this form, 1373 us in TILED, profiles/r05_pow2.txt)
        awkward = odd_short || (fill * 100 < (long double)o.flat2_long && (anysize || (c.total * es >= ((i64)8 << 20) && c.total * es < ((i64)1 << 30)))) ||
                  (novec && (anysize || c.total * es >= ((i64)3 << 20)));
    }
    if (!awkward) return false;
    bool used[MAXN];
    for (int d = 0; d < MAXN; ++d) used[d] = f.ingroup[0][d] = f.ingroup[1][d] = false;
    used[lead[0]] = used[lead[1]] = true;
    const i64 target = std::max<i64>(64, o.flat2_bytes);
    for (int s = 0; s < 2; ++s) {
        if (cutlead[s]) {
            const i64 e = c.dims[lead[s]];
            i64 tp = std::max<i64>(8, std::min<i64>(target / es, 128));
            const i64 nt = (e + tp - 1) / tp;
            f.R[s] = 1;
            f.p[s] = lead[s];
            f.TP[s] = (int)((e + nt - 1) / nt);
            continue;
        }
        f.ingroup[s][lead[s]] = true;
        i64 R = c.dims[lead[s]];
        f.p[s] = -1;
        f.TP[s] = 1;
        for (;;) {
            int nxt = -1;
            for (int d = 0; d < c.N; ++d)
                if (!used[d] && st[s][d] == R && c.dims[d] > 1) nxt = d;
            if (nxt < 0) break;
            used[nxt] = true;
            if (R * c.dims[nxt] <= 64 && R * c.dims[nxt] * es <= target) {
                f.ingroup[s][nxt] = true;
                R *= c.dims[nxt];
                continue;
            }
            i64 tp = std::max<i64>(1, std::min<i64>(std::min<i64>(target / (R * es), 128 / R), c.dims[nxt]));
            const i64 nt = (c.dims[nxt] + tp - 1) / tp;
            tp = (c.dims[nxt] + nt - 1) / nt;  // evened out over the extent
            f.p[s] = nxt;
            f.TP[s] = (int)tp;
            break;
        }
        if (R > 64) return false;
        f.R[s] = (int)R;
    }
    // both sides continue along the same dim behind their leads ((5,N,7) -> (7,N,5)): the destination got it; the input's run is
    // its lead alone, but input memory is still walked contiguously (Flat2Plan::shared)
    f.shared = f.p[1] < 0 && f.p[0] >= 0 && st[1][f.p[0]] == f.R[1] && f.TP[0] > 1;
    if (f.shared) {  // the tile is R[0] x TP[0] x R[1]: a longer tile along the shared dim (16 KiB, at most 512 positions of the destination run)
        const i64 dimp = c.dims[f.p[0]];
        i64 tp = std::max<i64>(1, std::min<i64>(std::min<i64>(512 / f.R[0], 16384 / ((i64)f.R[0] * f.R[1] * es)), dimp));
        const i64 nt = (dimp + tp - 1) / tp;
        f.TP[0] = (int)((dimp + nt - 1) / nt);
    }
    // enough tiles for the device: shorten the longer run while it stays above 128 bytes
    auto ntiles = [&]() {
        i64 n = 1;
        for (int d = 0; d < c.N; ++d) {
            if (f.ingroup[0][d] || f.ingroup[1][d]) continue;
            if (d == f.p[0]) n *= (c.dims[d] + f.TP[0] - 1) / f.TP[0];
            else if (d == f.p[1]) n *= (c.dims[d] + f.TP[1] - 1) / f.TP[1];
            else n *= c.dims[d];
        }
        return n;
    };
    for (int guard = 0; guard < 16 && ntiles() < 1024; ++guard) {
        const int s = ((i64)f.R[0] * f.TP[0] >= (i64)f.R[1] * f.TP[1]) ? 0 : 1;
        int pick = -1;
        for (int t : {s, 1 - s})
            if (pick < 0 && f.TP[t] > 1 && (i64)f.R[t] * ((f.TP[t] + 1) / 2) * es >= 128) pick = t;
        if (pick < 0) break;
        f.TP[pick] = (f.TP[pick] + 1) / 2;
    }
    if (f.TP[0] <= 1) f.shared = false;  // one position along the shared dim: the two orders coincide
    if ((i64)f.R[0] * f.TP[0] > (f.shared ? 512 : 128) || (i64)f.R[1] * f.TP[1] > 128) return false;
    if ((i64)f.R[0] * f.TP[0] * es < 64 && (i64)f.R[1] * f.TP[1] * es < 64) return false;  // nothing gained over the generic kernel
    if (ntiles() > 0x7fffffffLL) return false;
    // offsets on the other side of the leading index r of each run (mixed radix over the group dims in this side's stride order)
    for (int s = 0; s < 2; ++s) {
        std::vector<int> order;
        for (int d = 0; d < c.N; ++d)
            if (f.ingroup[s][d]) order.push_back(d);
        std::sort(order.begin(), order.end(), [&](int x, int y) { return st[s][x] < st[s][y]; });
        for (i64 r = 0; r < f.R[s]; ++r) {
            i64 rem = r, off = 0;
            for (int d : order) {
                off += (rem % c.dims[d]) * st[1 - s][d];
                rem /= c.dims[d];
            }
            if (off > 2147483647LL) return false;
            f.roff[s][r] = (int32_t)off;
        }
    }
    f.on = true;
    return true;
}

}  // namespace smr
