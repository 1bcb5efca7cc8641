// smr_plan.h -- private to the planner (smr_plan.cpp selects the family, smr_plan_<family>.cpp plan it): the family planners, the
// predicates they share and the helpers that build the XCD-aware work lists of TILED and ORBIT.
#pragma once

#include <algorithm>
#include <array>
#include <cstdlib>
#include <vector>

#include "smr_internal.h"

namespace smr {

// the family planners make_plan calls
bool plan_tiles(const Canon& c, TilePlan& t);                      // smr_plan_tiled.cpp
bool short_dim0_transposition(const Canon& c, int k, int es);     //   (such inputs are staged like transposed ones)
bool plan_orbit(const Canon& c, OrbitPlan& o);                     // smr_plan_orbit.cpp; builds the orbit lists: call it once per plan
bool plan_flat(const Canon& c, FlatPlan& f);                       // smr_plan_flat.cpp
bool plan_flatb(const Canon& c, FlatBPlan& f);
bool plan_flat2(const Canon& c, Flat2Plan& f);
void plan_reduce_all(const Canon& c, ReducePlan& rp);              // smr_plan_reduce.cpp
void plan_reduce_part(const Canon& c, ReducePlan& rp);
// complete reductions, single calls and the members of a reduction group (smr_plan_group.cpp) alike:
constexpr i64 REDUCE_ALL_PER_BLOCK = 256 * 16;  // box elements per workgroup before a second workgroup is taken; also the vector body's floor
constexpr i64 REDUCE_FOLD_MAX = 64;             // most partials of ONE arrival counter folded inside the launch (its arrivals serialise)
// does a complete reduction take the vector body?  Same-typed operands, a 16-byte vector of more than one element, canonical rank 1,
// a whole number of vectors, at least REDUCE_ALL_PER_BLOCK elements, every input broadcast or unit-stride from a 16-byte aligned
// address (`bases`: the call's base pointers, nullptr: the plan's)
bool reduce_all_vector(const Canon& c, void* const* bases);
// partial reductions, the general form: the lanes that cooperate on one destination element (a power of two, 1 .. 256; `red` reduced
// elements per output) -- plan_part_general's rule, which the members of a partial reduction group (smr_plan_group.cpp) take as well
int reduce_part_general_lanes(const Canon& c, i64 red);
bool plan_contract(const Canon& c, ContractPlan& cp);             // smr_plan_contract.cpp (shape rules + the "contract" option's gate)
// predicates shared by the family planners (smr_plan.cpp)
int elem_bytes(const Canon& c);                      // bytes per element as the kernels move them
int ceil_log2(i64 v);                                // 0 for v <= 1
i64 even_cut(i64 want, i64 n);                       // chunks an index range of n is cut into when about `want` are asked for
bool unit_or_bcast(const Canon& c, int d, int k0);   // every operand k >= k0 unit-stride or broadcast along dim d?
bool inputs_run_along(const Canon& c, int d);        // ... every input, and at least one of them unit-stride

// ---- work lists ------------------------------------------------------------------------------------------------------------
constexpr int NXCD = 8;                      // MI355X: eight XCDs with private L2s; workgroup b is dispatched to XCD b mod 8
constexpr uint32_t IDLE_TILE = 0xffffffffu;  // a work-list entry without work

// One contiguous run of the list per XCD: entry i of n (each `row` words) goes to position (i % cs) * NXCD + i / cs, cs =
// ceil(n / NXCD), so that workgroup NXCD * slot + x executes entry slot of run x; the positions left over hold `idle` in every word.
template <class T>
void deal_per_xcd(const T* list, size_t n, size_t row, std::vector<T>& out, T idle) {
    const size_t cs = (n + NXCD - 1) / NXCD;
    out.assign(cs * NXCD * row, idle);
    for (size_t i = 0; i < n; ++i) std::copy(list + i * row, list + (i + 1) * row, out.begin() + ((i % cs) * NXCD + i / cs) * row);
}

// Mixed radix over extents n[0..N), digit 0 fastest: id = sum coord[d] * mul[d] -- a linear tile id as the kernels decode it.
struct Radix {
    int N = 0;
    i64 n[MAXN], mul[MAXN], count = 1;  // count = product of the extents
    Radix() = default;
    Radix(const i64* extents, int N_) : N(N_) {
        for (int d = 0; d < N; ++d) {
            n[d] = extents[d];
            mul[d] = count;
            count *= n[d];
        }
    }
    void decode(i64 id, i64* coord) const {
        for (int d = 0; d < N; ++d) {
            coord[d] = id % n[d];
            id /= n[d];
        }
    }
    i64 encode(const i64* coord) const {
        i64 id = 0;
        for (int d = 0; d < N; ++d) id += coord[d] * mul[d];
        return id;
    }
};

// A grid of tiles cut into cells of edge[d] tiles along dim d (the last cell of a dim may be shorter): TILED's super-tiles and blocks,
// ORBIT's super-cells.  `cells` numbers the cells.
struct CellGrid {
    Radix cells;
    i64 grid[MAXN], edge[MAXN];
    CellGrid(const i64* grid_, const i64* edge_, int N) {
        i64 nc[MAXN];
        for (int d = 0; d < N; ++d) {
            grid[d] = grid_[d];
            edge[d] = edge_[d];
            nc[d] = (grid[d] + edge[d] - 1) / edge[d];
        }
        cells = Radix(nc, N);
    }
    // fn(coord) for the coordinate of every tile of one cell, in natural order (dim 0 fastest)
    template <class F>
    void for_each_in_cell(i64 cell, F&& fn) const {
        i64 lo[MAXN], n[MAXN], t[MAXN], cnt = 1;
        cells.decode(cell, lo);
        for (int d = 0; d < cells.N; ++d) {
            lo[d] *= edge[d];
            n[d] = std::min(edge[d], grid[d] - lo[d]);
            cnt *= n[d];
        }
        const Radix box(n, cells.N);
        for (i64 q = 0; q < cnt; ++q) {
            box.decode(q, t);
            for (int d = 0; d < cells.N; ++d) t[d] += lo[d];
            fn((const i64*)t);
        }
    }
};

// The image of tile coordinate t under the dim permutation g, (g . t)[g[d]] = t[d], as a linear id with multipliers mul
inline i64 image_of(const i64* t, const int* g, const i64* mul, int N) {
    i64 id = 0;
    for (int d = 0; d < N; ++d) id += t[d] * mul[g[d]];
    return id;
}

// Do operands j and k begin at the same address?
inline bool same_buffer(const Canon& c, int j, int k) {
    return (char*)c.base[j] + c.offsets[j] * c.esize[j] == (char*)c.base[k] + c.offsets[k] * c.esize[k];
}
// Are the strides of operand k a permutation of operand j's (over dims of equal extent)?  pi[d] = the dim along which j has the
// stride k has along d; prefer_fixed_points: a dim along which both have the same stride maps to itself.
inline bool stride_permutation(const Canon& c, int j, int k, int* pi, bool prefer_fixed_points) {
    bool used[MAXN] = {false};
    for (int d = 0; d < c.N; ++d) {
        int hit = -1;
        if (prefer_fixed_points && c.strides[j][d] == c.strides[k][d] && !used[d]) hit = d;
        for (int e = 0; e < c.N && hit < 0; ++e)
            if (!used[e] && c.strides[j][e] == c.strides[k][d] && c.dims[e] == c.dims[d]) hit = e;
        if (hit < 0) return false;
        used[hit] = true;
        pi[d] = hit;
    }
    return true;
}

}  // namespace smr
