// contract_walk.cpp -- CPU check of FAM_CONTRACT's work decomposition: for a few hundred random contraction shapes it plans the problem
// (the planner itself is linked in), then walks every workgroup, lane, register and chunk exactly as smr_k_contract.hip does -- the
// blockIdx.x decode, the lane's register -> tile index map (contract_idx of smr_internal.h, the kernel's own), the chunk walk over (q, k) bounded by the true extent -- and
// checks that every (i, j, rest, q, k) of the box is visited exactly once, by exactly one (workgroup, lane, register), and that no
// visit falls outside the box.  Every shape is then planned again with a forced tile ("contract_tile") and forced slices
// ("contract_split") and walked as the split form's two launches do: workgroup b of the main launch is (tile = b % tiles, slice =
// b / tiles) and walks chunks [slice * cps, min((slice + 1) * cps, Q * nkc)); every slice must be non-empty, every box element visited
// exactly once, every partial index a (workgroup, lane, register) stores must lie inside scratch_bytes and be stored once, and the
// fold's walk -- workgroup (register = b % RB^2, tile = b / RB^2), lane, slice -- must read each of them exactly once and reach every
// output exactly once, through the same (register, lane) -> (i, j) map as the main kernel (both use contract_idx with r = register / RB along di).
// No GPU, no library.  Build and run under AddressSanitizer + UBSan: make -C strided.jl_amd/csrc contract_walk
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../strided.jl_amd/csrc/smr_internal.h"

namespace smr {
int set_error(int code, const std::string&) { return code; }
int cu_count() { return 256; }
}  // namespace smr
extern "C" const char* smr_last_error(void) { return ""; }  // (the group planner, linked with the other planner files, quotes it)
using namespace smr;

// Walks one CONTRACT plan (split or not) as the kernels do; 0 when every box element is visited exactly once and -- split -- the
// partials are stored and read exactly once, inside the buffer.
static int walk(const Plan& plan, int it) {
    const Canon& c = plan.c;
    const ContractPlan& cp = plan.contract;
    const int es = dtype_size(c.ct), rb = cp.rb, tile = CONTRACT_LANES * rb, tk = contract_tk(es, rb);
    if (cp.ti != tile || cp.tj != tile || cp.tk != tk) return std::printf("problem %d: tile numbers\n", it), 1;
    const i64 K = c.dims[c.NK], Q = c.total / c.nout / K, nkc = (K + tk - 1) / tk, nchunks = Q * nkc;
    const i64 S = cp.kparts, cps = S > 1 ? cp.cps : nchunks;
    if (S > 1) {
        if ((S - 1) * cps >= nchunks || S * cps < nchunks) return std::printf("problem %d: an empty slice, or chunks left over (%s)\n", it, plan.desc.c_str()), 1;
        if (cp.scratch_bytes != (size_t)(cp.grid * S * tile * tile * es)) return std::printf("problem %d: scratch_bytes\n", it), 1;
    } else if (cp.scratch_bytes != 0 || cp.cps != 0) {
        return std::printf("problem %d: an unsplit plan with partials\n", it), 1;
    }
    const size_t npart = S > 1 ? cp.scratch_bytes / (size_t)es : 0;
    std::vector<unsigned char> stored(npart, 0), read(npart, 0);
    std::vector<unsigned char> seen((size_t)c.total, 0);  // canonical box, dim 0 fastest
    i64 mul_[MAXN], s = 1;
    for (int d = 0; d < c.N; ++d) {
        mul_[d] = s;
        s *= c.dims[d];
    }
    std::vector<int> rdim;
    for (int d = 0; d < c.NK; ++d)
        if (d != cp.di && d != cp.dj) rdim.push_back(d);
    for (i64 wg = 0; wg < cp.grid * S; ++wg) {
        const i64 sl = wg / cp.grid, tl = wg - sl * cp.grid;  // k_contract_split: the slice is the slow digit
        const i64 t_lo = sl * cps, t_hi = std::min(t_lo + cps, nchunks);
        if (t_lo >= t_hi) return std::printf("problem %d: slice %lld is empty\n", it, (long long)sl), 1;
        i64 b = tl;
        const i64 bi = b % cp.nti;
        b /= cp.nti;
        const i64 bj = b % cp.ntj;
        b /= cp.ntj;
        i64 rest = 0;
        for (int d : rdim) {
            rest += (b % c.dims[d]) * mul_[d];
            b /= c.dims[d];
        }
        if (b != 0) return std::printf("problem %d: workgroup %lld decodes past the grid\n", it, (long long)wg), 1;
        for (int lane = 0; lane < 256; ++lane) {
            const int li = lane & (CONTRACT_LANES - 1), lj = lane >> 4;
            for (int r = 0; r < rb; ++r)
                for (int q2 = 0; q2 < rb; ++q2) {
                    if (S > 1) {  // the store of the register block: every lane, ragged or not
                        const i64 at = (tl * S + sl) * (i64)(rb * rb * 256) + (i64)(r * rb + q2) * 256 + lane;
                        if (at < 0 || (size_t)at >= npart) return std::printf("problem %d: a partial is stored outside the buffer\n", it), 1;
                        if (stored[(size_t)at]++) return std::printf("problem %d: partial %lld stored twice\n", it, (long long)at), 1;
                    }
                    const i64 i = bi * tile + contract_idx(es, rb, li, r), j = bj * tile + contract_idx(es, rb, lj, q2);
                    if (contract_idx(es, rb, li, r) >= tile || contract_idx(es, rb, lj, q2) >= tile) return std::printf("problem %d: lane index past the tile\n", it), 1;
                    if (i >= c.dims[cp.di] || j >= c.dims[cp.dj]) continue;  // never stored to the destination
                    for (i64 t = t_lo; t < t_hi; ++t) {
                        const i64 q = t / nkc, k0 = (t % nkc) * tk, kn = std::min<i64>(tk, K - k0);
                        i64 qoff = 0, qq = q;
                        for (int d = c.NK + 1; d < c.N; ++d) {
                            qoff += (qq % c.dims[d]) * mul_[d];
                            qq /= c.dims[d];
                        }
                        for (i64 kk = 0; kk < kn; ++kk) {
                            const i64 at = rest + i * mul_[cp.di] + j * mul_[cp.dj] + (k0 + kk) * mul_[c.NK] + qoff;
                            if (at < 0 || at >= c.total) return std::printf("problem %d: visit outside the box\n", it), 1;
                            if (seen[(size_t)at]++) return std::printf("problem %d: element %lld visited twice\n", it, (long long)at), 1;
                        }
                    }
                }
        }
    }
    for (i64 e = 0; e < c.total; ++e)
        if (seen[(size_t)e] != 1) return std::printf("problem %d (%s): element %lld visited %d times\n", it, plan.desc.c_str(), (long long)e, seen[(size_t)e]), 1;
    if (S > 1) {  // k_contract_fold: one lane per (tile, register, lane), the slices in order
        std::vector<unsigned char> out((size_t)c.nout, 0);
        for (i64 wg = 0; wg < cp.grid * rb * rb; ++wg) {
            const int reg = (int)(wg % (rb * rb));
            i64 b = wg / (rb * rb);
            const i64 tl = b, bi = b % cp.nti, bj = (b / cp.nti) % cp.ntj;
            i64 rest = 0, br = b / cp.nti / cp.ntj;  // the other kept dims, decoded as the main kernel does
            for (int d : rdim) {
                rest += (br % c.dims[d]) * mul_[d];
                br /= c.dims[d];
            }
            if (br != 0) return std::printf("problem %d: fold workgroup %lld decodes past the grid\n", it, (long long)wg), 1;
            for (int lane = 0; lane < 256; ++lane) {
                const i64 i = bi * tile + contract_idx(es, rb, lane & (CONTRACT_LANES - 1), reg / rb), j = bj * tile + contract_idx(es, rb, lane >> 4, reg % rb);
                for (i64 sl = 0; sl < S; ++sl) {
                    const i64 at = tl * S * (i64)(rb * rb * 256) + reg * 256 + lane + sl * (i64)(rb * rb * 256);
                    if (at < 0 || (size_t)at >= npart) return std::printf("problem %d: the fold reads outside the buffer\n", it), 1;
                    if (!stored[(size_t)at]) return std::printf("problem %d: the fold reads a partial nobody stored\n", it), 1;
                    if (read[(size_t)at]++) return std::printf("problem %d: partial %lld read twice\n", it, (long long)at), 1;
                }
                // the output this lane's fold is stored to: inside the box exactly once (kept dims are the leading canonical dims, so the
                // box offset is the output's index), and the (i, j) of the main kernel's lane and register block entry that stored the partials
                if (i >= c.dims[cp.di] || j >= c.dims[cp.dj]) continue;
                const i64 o = rest + i * mul_[cp.di] + j * mul_[cp.dj];
                if (o < 0 || o >= c.nout) return std::printf("problem %d: the fold stores outside the outputs\n", it), 1;
                if (out[(size_t)o]++) return std::printf("problem %d: output %lld folded twice\n", it, (long long)o), 1;
            }
        }
        for (i64 o = 0; o < c.nout; ++o)
            if (out[(size_t)o] != 1) return std::printf("problem %d (%s): output %lld folded %d times\n", it, plan.desc.c_str(), (long long)o, out[(size_t)o]), 1;
        for (size_t e = 0; e < npart; ++e)
            if (stored[e] != 1 || read[e] != 1) return std::printf("problem %d (%s): partial %zu stored %d times, read %d times\n", it, plan.desc.c_str(), e, stored[e], read[e]), 1;
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(12345);
    auto pick = [&](i64 lo, i64 hi) { return lo + (i64)(rng() % (uint64_t)(hi - lo + 1)); };
    const int dts[] = {SMR_F32, SMR_F64, SMR_C64};
    options().contract = 2;
    long planned = 0, big = 0, nsplit = 0, nclamped = 0, tile_seen[3] = {0, 0, 0};
    for (int it = 0; it < 300; ++it) {
        // box (m, n, [batch], k, [k2]); input 1 varies along m, input 2 along n, both along batch and the reduced dims
        // (one shape in fifty is large enough for the 64 x 64 tiles)
        const bool large = it % 50 == 7, batch = !large && it % 3 == 1, two = !large && it % 4 == 2;
        const i64 m = large ? pick(2000, 2100) : pick(2, 150), n = large ? pick(1100, 1400) : pick(2, 150), k = large ? pick(2, 6) : pick(2, 70);
        std::vector<i64> dims = {m, n};
        if (batch) dims.push_back(pick(2, 4));
        const int nk = (int)dims.size();
        dims.push_back(k);
        if (two) dims.push_back(pick(2, 3));
        const int N = (int)dims.size(), dt = dts[it % 3];
        smr_problem p;
        std::memset(&p, 0, sizeof p);
        static const uint8_t mul[] = {SMR_OP_ARG, 1, SMR_OP_ARG, 2, SMR_OP_MUL, 0};
        p.N = N;
        p.M = 3;
        p.fprog = mul;
        p.fprog_len = 3;
        p.redop = SMR_RED_ADD;
        i64 acc[3] = {1, 1, 1};
        for (int d = 0; d < N; ++d) {
            p.dims[d] = dims[d];
            const bool varies[3] = {d < nk, d != 1, d != 0};
            for (int o = 0; o < 3; ++o) {
                p.ops[o].strides[d] = varies[o] ? acc[o] : 0;
                if (varies[o]) acc[o] *= dims[d] + 1;  // padded: dims do not fuse
            }
        }
        for (int o = 0; o < 3; ++o) {
            p.ops[o].base = (char*)0x7e0000000000ull + ((i64)o << 36);
            p.ops[o].dtype = dt;
        }
        Plan plan;
        if (make_plan(&p, plan) != 0 || plan.family != FAM_CONTRACT) {
            std::printf("problem %d was not planned as a contraction: %s\n", it, plan.desc.c_str());
            return 1;
        }
        ++planned;
        big += plan.contract.rb == 4;
        if (walk(plan, it)) return 1;
        // the same problem with a forced tile and forced slices (one in four: more slices than chunks, clamped)
        const i64 tiles3[] = {16, 32, 64};
        options().contract_tile = tiles3[pick(0, 2)];
        if (large && options().contract_tile == 16) options().contract_tile = 32;  // (the walk is per lane: keep it short)
        options().contract_split = it % 4 == 3 ? 1000 : pick(2, 9);
        Plan sp;
        const int rc = make_plan(&p, sp);
        const i64 asked = options().contract_split, forced = options().contract_tile;
        options().contract_tile = options().contract_split = 0;
        if (rc != 0 || sp.family != FAM_CONTRACT || sp.contract.ti != forced) {
            std::printf("problem %d was not planned on the forced tile: %s\n", it, sp.desc.c_str());
            return 1;
        }
        if (sp.contract.kparts > asked) return std::printf("problem %d: more slices than asked for\n", it), 1;
        nsplit += sp.contract.kparts > 1;
        nclamped += sp.contract.kparts > 1 && asked == 1000;
        for (int t = 0; t < 3; ++t) tile_seen[t] += sp.contract.kparts > 1 && sp.contract.ti == tiles3[t];
        if (walk(sp, it)) return 1;
    }
    std::printf("%ld contraction shapes (%ld with 64 x 64 tiles): every box element visited exactly once\n", planned, big);
    std::printf("%ld of them split with a forced tile (16 x 16: %ld, 32 x 32: %ld, 64 x 64: %ld; %ld with the slices clamped to the chunks): "
                "no empty slice, every box element visited once, every partial stored once inside the buffer and read once by the fold, every output folded once\n",
                nsplit, tile_seen[0], tile_seen[1], tile_seen[2], nclamped);
    return big > 0 && tile_seen[0] > 10 && tile_seen[1] > 10 && tile_seen[2] > 10 && nclamped > 10 ? 0 : 1;
}
