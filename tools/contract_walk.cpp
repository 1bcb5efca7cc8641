// contract_walk.cpp -- CPU check of FAM_CONTRACT's work decomposition: for a few hundred random contraction shapes it plans the problem
// (the planner itself is linked in), then walks every workgroup, lane, register and chunk exactly as smr_k_contract.hip does -- the
// blockIdx.x decode, the lane's register -> tile index map (contract_idx of smr_internal.h, the kernel's own), the chunk walk over (q, k) bounded by the true extent -- and
// checks that every (i, j, rest, q, k) of the box is visited exactly once, by exactly one (workgroup, lane, register), and that no
// visit falls outside the box.  No GPU, no library.  Build and run under AddressSanitizer + UBSan: make -C strided.jl_amd/csrc contract_walk
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

int main() {
    std::mt19937_64 rng(12345);
    auto pick = [&](i64 lo, i64 hi) { return lo + (i64)(rng() % (uint64_t)(hi - lo + 1)); };
    const int dts[] = {SMR_F32, SMR_F64, SMR_C64};
    options().contract = 2;
    long planned = 0, big = 0;
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
        const Canon& c = plan.c;
        const ContractPlan& cp = plan.contract;
        big += cp.rb == 4;
        const int es = dtype_size(c.ct), rb = cp.rb, tile = CONTRACT_LANES * rb, tk = contract_tk(es, rb);
        if (cp.ti != tile || cp.tj != tile || cp.tk != tk) return std::printf("problem %d: tile numbers\n", it), 1;
        const i64 K = c.dims[c.NK], Q = c.total / c.nout / K, nkc = (K + tk - 1) / tk;
        std::vector<unsigned char> seen((size_t)c.total, 0);  // canonical box, dim 0 fastest
        i64 mul_[MAXN], s = 1;
        for (int d = 0; d < c.N; ++d) {
            mul_[d] = s;
            s *= c.dims[d];
        }
        std::vector<int> rdim;
        for (int d = 0; d < c.NK; ++d)
            if (d != cp.di && d != cp.dj) rdim.push_back(d);
        for (i64 wg = 0; wg < cp.grid; ++wg) {
            i64 b = wg;
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
                        const i64 i = bi * tile + contract_idx(es, rb, li, r), j = bj * tile + contract_idx(es, rb, lj, q2);
                        if (contract_idx(es, rb, li, r) >= tile || contract_idx(es, rb, lj, q2) >= tile) return std::printf("problem %d: lane index past the tile\n", it), 1;
                        if (i >= c.dims[cp.di] || j >= c.dims[cp.dj]) continue;  // never stored
                        for (i64 t = 0; t < Q * nkc; ++t) {
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
    }
    std::printf("%ld contraction shapes (%ld with 64 x 64 tiles): every box element visited exactly once\n", planned, big);
    return big > 0 ? 0 : 1;
}
