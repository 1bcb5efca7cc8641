// smr_plan_contract.cpp -- planner of FAM_CONTRACT (smr_k_contract.hip): the shape rules, the "contract" option's gate, the tile
// geometry, and the vector width one execution uses (contract_vec).
//
// The shape: a reduction of f(in1, in2) whose two inputs vary along DIFFERENT kept dims -- the box of the reference's generic
// __mul! (src/linalg.jl:130-162): C2 = (m, n, 1), A2 = (m, 1, k), B2 = (1, n, k).  Every element of in1 is used n times and every
// element of in2 m times, so REDUCE_PART (one use per load) runs it at a few per cent of the vector ALUs; this family stages a
// TI x TK tile of in1 and a TJ x TK tile of in2 in LDS once per chunk and keeps an RB x RB block of outputs per lane in registers
// (RB = 4, 2 or 1: 64 x 64, 32 x 32 or 16 x 16 tiles, by the number of workgroups they give).
#include "smr_contract.h"
#include "smr_plan.h"

namespace smr {

// The tiled kept dim of input `k` (the other input `o` does not vary along it): the largest extent, unit stride breaking ties.
static int pick_tile_dim(const Canon& c, int k, int o) {
    int best = -1;
    for (int d = 0; d < c.NK; ++d) {
        if (c.strides[k][d] == 0 || c.strides[o][d] != 0) continue;
        if (best < 0 || c.dims[d] > c.dims[best] || (c.dims[d] == c.dims[best] && std::llabs(c.strides[k][d]) == 1 && std::llabs(c.strides[k][best]) != 1))
            best = d;
    }
    return best;
}

// contract = 1: is the problem large enough for the family to win?  Measured with tools/contract_cases.py, CONTRACT against
// REDUCE_PART (profiles/contract_cases.txt; the thresholds are quoted there).  The family has no split along the reduced range: a
// launch with fewer workgroups than keep the device busy loses to REDUCE_PART's split forms, so the gate asks for enough output
// tiles, for tiles that are mostly full, and for a reduced length that amortises staging.
static bool contract_gate(const Canon& c, const ContractPlan& cp) {
    // Thresholds (profiles/contract_cases.txt, MI355X, 256 CUs):
    //   tile extents >= 32 along both tiled dims;
    //   output tiles >= 256 (of the tile plan_contract chose): a workgroup per CU.  Every measured row with 256 and more wins, from
    //     1.16x ((1000, 1000, 16) Float32) and 1.4x (256^3) to 3.6 - 5.3x (1024^3); rows with 42 - 144 tiles win 1.01 - 1.4x or tie,
    //     (64, 64, 4096) with 16 tiles loses 4x: left to REDUCE_PART, whose split forms cut the reduced range;
    //   extent of the inner reduced dim (the one walked in chunks) >= 16: (1000, 1000, 16) still wins; below, every chunk is a few
    //     rows between two barriers and staging is not amortised, however long the outer reduced index (not measured: left alone);
    //   op = +: min-plus (f = a + b, op = min, runtime-compiled) loses at every size measured (256^3 0.56x, 512^3 0.45x, 1024^3
    //     0.71x): Julia's NaN-aware min is ten instructions per pair and the family's gain is in the loads -- left to REDUCE_PART;
    //   no interpreted f: with jit = 0 every f but the natively compiled product of same-typed operands runs in the interpreter,
    //     whose kernels of this family need scratch memory (they leave direct dispatch) and were never timed against REDUCE_PART.
    //     (A runtime compiler that turns out to be missing at launch is not known here: that launch interprets.)
    if (c.redop != SMR_RED_ADD) return false;
    if (!options().jit && (c.mixed || c.fkind != FK_MUL2)) return false;
    if (c.dims[cp.di] < 32 || c.dims[cp.dj] < 32) return false;
    if (c.dims[c.NK] < 16) return false;
    // a split plan (option "contract_split") runs grid * kparts workgroups: those keep the device busy
    if (cp.grid * cp.kparts < 256) return false;
    return true;
}

// Sets the tile-dependent fields of `cp` for register block rb; unsplit.
static void contract_set_plan_tile(const Canon& c, ContractPlan& cp, int rb, i64 rest) {
    const int es = dtype_size(c.ct);
    cp.rb = rb;
    cp.ti = cp.tj = CONTRACT_LANES * rb;
    cp.tk = contract_tk(es, rb);
    cp.nti = (c.dims[cp.di] + cp.ti - 1) / cp.ti;
    cp.ntj = (c.dims[cp.dj] + cp.tj - 1) / cp.tj;
    cp.nrest = rest;
    cp.grid = cp.nti * cp.ntj * rest;
    cp.lds_bytes = contract_lds(es, rb);
    cp.kparts = 1;
    cp.cps = 0;
    cp.scratch_bytes = 0;
}

// chunks of the walk over (q, k) with the plan's tile
static i64 contract_nchunks(const Canon& c, const ContractPlan& cp) {
    const i64 K = c.dims[c.NK], Q = c.total / c.nout / K;
    return Q * ((K + cp.tk - 1) / cp.tk);
}

// Cuts the chunk walk of `cp` (its tile set) into at most `want` slices: clamped to the chunks, then cps = ceil(nchunks / S) and
// S = ceil(nchunks / cps), so no slice is empty.  One slice, partials beyond 2^31 bytes or a grid beyond 2^31 - 1: left unsplit.
static void contract_cut(const Canon& c, ContractPlan& cp, i64 want) {
    i64 cps = 0;
    const i64 S = contract_slices(contract_nchunks(c, cp), want, cps);
    if (S < 2) return;
    const long double bytes = (long double)cp.grid * (long double)S * (long double)(cp.ti * cp.tj) * (long double)dtype_size(c.ct);
    if (bytes > 2147483648.0L || (long double)cp.grid * (long double)S > 2147483647.0L) return;
    cp.kparts = (int)S;
    cp.cps = cps;
    cp.scratch_bytes = (size_t)bytes;
}

// contract_split = 1: the tile and the number of slices of a problem whose unsplit plan has fewer than 256 workgroups.  Of the tiles
// allowed (`rbs`, largest first) the largest whose tiles * S can reach the family's workgroup thresholds (512 for 64 x 64, else 256, as
// plan_contract) with S inside the three bounds below; S is then what brings the launch to 512 workgroups, or the bound.  Where no
// tile reaches its threshold, the tile whose bounds allow the most workgroups, if that is at least two slices; else the problem is not
// split (false).  Measured with tools/contract_split_cases.py (profiles/contract_split.txt, MI355X; us per launch, the rows as that
// file has them -- "c" is the rule's own plan; the first rule started from slices of 4 chunks, a quarter of the input bytes and the
// thresholds alone):
//   slices of at least 2 chunks (the prologue of the double buffer is one exposed fetch and barrier per slice): (64, 64, 4096)
//     Float32 on 16 x 16 tiles: 4 chunks per slice (S16) 11.9, 2 chunks (c) 11.8, 1 chunk (S64) 13.8; (256, 256, 4096) Float32 forced
//     onto 32 x 32 tiles: 4 chunks (S16) 29.5, 2 chunks (S32) 30.6, 1 chunk (S64) 35.3;
//   S <= 64: the largest value measured, and the best one wherever it is what brings a row to its workgroups ((32, 32, 1048576)
//     Float32: 64 slices (c) 315.7 against 32 slices 614.3); beyond 64: not measured;
//   the partials' round trip, 2 * scratch_bytes, at most HALF the bytes the inputs move, (dims[di] + dims[dj]) * K * Q * es: at one half
//     the split still gains ((128, 128, 16384) Float64, 32 x 32 tiles: 64 slices 41.6 against 32 slices (c) 47.3; (64, 64, 4096)
//     Float32, 16 x 16: 32 slices (c) 11.8 against 16 slices 11.9), at the whole of it no longer ((64, 64, 4096) ComplexF64, 16 x 16:
//     64 slices 19.0 against 32 slices (c) 18.6);
//   512 workgroups: past a tile's threshold more slices keep gaining up to about two workgroups per CU -- (64, 64, 4096) on 16 x 16
//     tiles, 256 / 512 / 1024 workgroups (S16 / c / S64): Float32 11.9 / 11.8 / 13.8, Float64 14.9 / 14.1 / 16.2, ComplexF64 24.8 /
//     18.6 / 19.0; (128, 128, 16384) Float32 on 32 x 32 tiles 36.4 / 32.1 / 34.1 (Float64 and ComplexF64 gain another 12 % at 1024:
//     47.3 -> 41.6, 108.7 -> 96.1 -- left alone: one target for every type);
//   the larger tile first: (64, 64, 65536) Float32 32 x 32 with 256 workgroups (c) 41.1 against 16 x 16 with 1024 workgroups 55.6
//     (Float64 80.3 against 87.8; ComplexF64 the other way round, 162.6 against 133.1: the choice is not type-dependent here).
static bool contract_split_rule(const Canon& c, ContractPlan& cp, const int* rbs, int nrb, i64 rest) {
    // (the constants and the three bounds live in smr_contract.h: the group planner reads the same rule over a whole group)
    constexpr i64 TARGET = CONTRACT_SPLIT_TARGET;
    const int es = dtype_size(c.ct);
    const i64 K = c.dims[c.NK], Q = c.total / c.nout / K;
    int best_rb = 0;
    i64 best_s = 0, best_wgs = 0;
    for (int n = 0; n < nrb; ++n) {
        ContractPlan t = cp;
        contract_set_plan_tile(c, t, rbs[n], rest);
        const i64 smax = contract_split_smax(es, c.dims[cp.di], c.dims[cp.dj], K, Q, contract_nchunks(c, t), t.grid, t.ti);
        if (smax < 2) continue;
        const i64 thr = rbs[n] == 4 ? 512 : 256;
        if (t.grid * smax >= thr) {
            best_rb = rbs[n];
            best_s = std::max<i64>(2, std::min<i64>(smax, (TARGET + t.grid - 1) / t.grid));
            break;
        }
        if (t.grid * smax > best_wgs) {
            best_wgs = t.grid * smax;
            best_rb = rbs[n];
            best_s = smax;
        }
    }
    if (!best_rb) return false;
    ContractPlan t = cp;
    contract_set_plan_tile(c, t, best_rb, rest);
    contract_cut(c, t, best_s);
    if (t.kparts < 2) return false;
    cp = t;
    return true;
}

// The shape rules alone, without the "contract" option and its gate: is `c` an outer-product reduction this family's tile body can
// run, and along which kept dims is it tiled?  plan_contract asks it for a single call, the group planner (smr_plan_group.cpp) for every
// member of a contraction group.
bool contract_shape(const Canon& c, int& di, int& dj) {
    if (c.redop == SMR_RED_NONE || c.M != 3 || c.bitcopy) return false;
    if (c.NK < 2 || c.N - c.NK < 1) return false;
    // no repeated operand: identical inputs were deduplicated (M would be 2); an input that is the destination's own buffer would be
    // read by one workgroup while another stores into it
    for (int k = 1; k < 3; ++k)
        if (c.base[k] == c.base[0]) return false;
    if (c.strides[1][c.NK] == 0 || c.strides[2][c.NK] == 0) return false;
    di = pick_tile_dim(c, 1, 2);
    dj = pick_tile_dim(c, 2, 1);
    return di >= 0 && dj >= 0;
}

bool plan_contract(const Canon& c, ContractPlan& cp) {
    const Options& o = options();
    if (o.contract == 0 || !contract_shape(c, cp.di, cp.dj)) return false;
    const int es = dtype_size(c.ct);
    // 64 x 64 tiles (4 x 4 outputs per lane) when they fill the device twice over, else 32 x 32 (2 x 2) when those give a workgroup per
    // CU, else 16 x 16 (one output per lane: no reuse in registers, but 256^3 is 256 workgroups instead of 64 on a quarter of the CUs)
    // (the 256 is measured, profiles/contract_cases.txt; the 512 is not: the 64 x 64 kernel was timed against REDUCE_PART only, never
    // against 32 x 32 tiles on the same problem -- two workgroups per CU is where its two waves per SIMD are all resident)
    i64 rest = 1;
    for (int d = 0; d < c.NK; ++d)
        if (d != cp.di && d != cp.dj) rest *= c.dims[d];
    auto tiles = [&](int rb) {
        const i64 t = CONTRACT_LANES * rb;
        return ((c.dims[cp.di] + t - 1) / t) * ((c.dims[cp.dj] + t - 1) / t) * rest;
    };
    const int want = o.contract_tile ? (int)(o.contract_tile / CONTRACT_LANES) : (tiles(4) >= 512 ? 4 : (tiles(2) >= 256 ? 2 : 1));
    // the LDS is static: a budget below the tile's takes the next smaller tile that fits, or refuses the family (a tile forced by
    // "contract_tile" is not exchanged for a smaller one: it fits or the family is refused)
    const i64 cap = std::min<i64>(o.max_lds_bytes, 65536);
    int rb0 = 0;
    for (int rb = want; rb >= 1 && !rb0; rb >>= 1) {
        if ((i64)contract_lds(es, rb) <= cap) rb0 = rb;
        if (o.contract_tile) break;
    }
    if (!rb0) return false;
    contract_set_plan_tile(c, cp, rb0, rest);
    if (cp.grid > 0x7fffffffLL) return false;
    // the split form (opt-in: another accumulation order): forced slices on the tile chosen above, or the rule, which only looks at
    // launches with fewer workgroups than CUs and picks tile and slices together (a forced tile stays)
    if (o.contract_split >= 2) {
        contract_cut(c, cp, o.contract_split);
    } else if (o.contract_split == 1 && cp.grid < 256) {
        int rbs[3], nrb = 0;
        for (int rb = 4; rb >= 1; rb >>= 1)
            if (o.contract_tile ? rb == rb0 : (i64)contract_lds(es, rb) <= cap) rbs[nrb++] = rb;
        contract_split_rule(c, cp, rbs, nrb, rest);
    }
    return o.contract >= 2 || contract_gate(c, cp);
}

// Whole tiles load 16-byte vectors when BOTH inputs allow it: along its unit-stride axis (the tiled dim or the inner reduced dim NK)
// every other stride is a multiple of the vector, the base is 16-byte aligned, and -- vectors along NK -- the reduced extent is a
// whole number of vectors.  Ragged tiles always load element by element (clamped, never guarded).
int contract_vec(const Plan& plan, void* const* bases) { return contract_vec_of(plan.c, plan.contract.di, plan.contract.dj, bases); }

int contract_vec_of(const Canon& c, int di, int dj, void* const* bases) {
    const int es = dtype_size(c.ct);
    const int v = (c.mixed || es >= 16) ? 1 : 16 / es;
    if (v == 1) return 1;
    for (int k = 1; k < 3; ++k) {
        const int dt = k == 1 ? di : dj;
        int ax = -1;
        if (c.strides[k][dt] == 1) ax = dt;
        else if (c.strides[k][c.NK] == 1) ax = c.NK;
        if (ax < 0) return 1;
        if (ax == c.NK && c.dims[c.NK] % v) return 1;
        const uintptr_t b = (uintptr_t)(bases ? bases[c.orig[k]] : c.base[k]) + (uintptr_t)(c.offsets[k] * (i64)c.esize[k]);
        if (b % 16) return 1;
        for (int d = 0; d < c.N; ++d)
            if (d != ax && c.strides[k][d] % v) return 1;
    }
    return v;
}

}  // namespace smr
