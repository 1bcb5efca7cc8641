// smr_plan_group.cpp -- the group planner (smr_group.h: plan_group).  Host arithmetic only, no HIP runtime call: like every planner
// file it links into tools/plan_dump.cpp, which pins the device tables of a corpus of groups.  One loop over the members: each is
// canonicalised like a single call, checked against member 0 (one kernel instantiation, one f; under SMR_GROUP_MEMBER_SCALARS the
// values of f's constants are the member's own, a row of a third table; a contraction group takes them under SMR_GROUP_CONTRACT_SCALARS)
// and given its descriptor; its operands' byte ranges are the
// independence check's input and the footprint of a group recorded in a sequence.  What differs between the kinds are plain functions
// called from that loop: a map member takes one of the kernel's two bodies and its workgroups at once, a contraction its workgroups
// once the whole group has decided the tile, a complete reduction (SMR_GROUP_REDUCE) its body, its workgroups and -- with more than
// one -- its run of partial slots and its arrival counter, a partial reduction (SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART) its lanes per
// destination element and its workgroups.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "smr_contract.h"
#include "smr_group.h"
#include "smr_plan.h"

namespace smr {

i64& group_contract_tile() { static i64 v = 0; return v; }
i64& group_contract_split() { static i64 v = 0; return v; }

namespace {

typedef std::vector<std::pair<uintptr_t, uintptr_t>> Spans;  // (smr_sched.h)

std::string member_tag(int i) { return "smr_group_create: member " + std::to_string(i); }

// does member `c` run the same kernel instantiation with the same functor as member 0 (`r`)?  Empty = yes, else what differs.
// `own_scalars` (SMR_GROUP_MEMBER_SCALARS; SMR_GROUP_CONTRACT_SCALARS on a contraction group): the values of f's constants may differ,
// nothing else.
std::string mismatch(const Canon& r, const Canon& c, bool own_scalars) {
    if (c.bitcopy != r.bitcopy || (!c.bitcopy && c.ct != r.ct)) return "computes in another class than member 0";
    if (c.mixed != r.mixed) return "differs from member 0 in whether operand types are converted";
    if (c.M != r.M) return "has another number of distinct operands than member 0 (" + std::to_string(c.M) + " != " + std::to_string(r.M) + ")";
    for (int k = 0; k < c.M; ++k) {
        if (c.dtype[k] != r.dtype[k]) return "operand " + std::to_string(c.orig[k]) + " has another dtype than in member 0";
        if (c.conj[k] != r.conj[k]) return "operand " + std::to_string(c.orig[k]) + " has another conj flag than in member 0";
    }
    const ProgD &p = c.prog, &q = r.prog;
    if (p.len != q.len || p.nconst != q.nconst || std::memcmp(p.code, q.code, (size_t)(2 * p.len)) != 0 ||
        (!own_scalars && std::memcmp(p.consts, q.consts, sizeof(double) * (size_t)(2 * p.nconst)) != 0))
        return own_scalars ? "has another f-program than member 0 (only the values of its constants may differ)" : "has another f (program or constants) than member 0";
    // recognition (smr_canon.cpp) looks at the program's structure, FK_EXPR5 also at a constant's value: one launch runs ONE functor
    if (own_scalars && c.fkind != r.fkind) return "is recognised as another functor than member 0";
    if (r.redop != SMR_RED_NONE) {  // a contraction or a reduction group: one op and one initop code as well; beta (initarg) is the member's own
        if (c.redop != r.redop) return "reduces with another op than member 0";
        if (c.initop != r.initop) return "has another kind of initop than member 0 (only its argument, beta, may differ)";
    }
    return std::string();
}

// does the launch run a natively compiled functor that keeps constants in fields (with_functor, smr_dispatch.h)?  Its per-member
// row is Canon::fc; every other f with constants is a program (runtime-compiled or interpreted) and its row is ProgD::consts.
bool native_with_consts(const Canon& c) {
    if (c.bitcopy || c.mixed || !(GROUP_FMASK & fbit(c.fkind))) return false;
    const int k = c.fkind;
    return k == FK_SCALE || k == FK_AXPY || k == FK_AXPBY || (k == FK_SYM && c.ct != SMR_I64) || (k == FK_EXPR5 && (c.ct == SMR_F32 || c.ct == SMR_F64));
}

// picks the body of one member and fills its descriptor; returns its number of workgroups
i64 plan_member(const Canon& c, GroupMemberD& m) {
    std::memset(&m, 0, sizeof m);
    m.N = c.N;
    m.total = (uint32_t)c.total;
    for (int k = 0; k < c.M; ++k) {
        m.base[k] = (char*)c.base[k] + c.offsets[k] * (i64)c.esize[k];
        for (int d = 0; d < c.N; ++d) m.strides[k][d] = c.strides[k][d];
    }
    for (int d = 0; d < MAXN; ++d) m.dims[d] = d < c.N ? (uint32_t)c.dims[d] : 1u;
    {   // 256 in the mixed radix of the dims (what does not fit is beyond the box and never reached)
        i64 rem = 256;
        for (int d = 0; d < c.N; ++d) {
            m.step[d] = (uint32_t)(rem % c.dims[d]);
            rem /= c.dims[d];
        }
    }
    // inputs whose unit-stride dim is another one than the destination's fastest dim (canonical dim 0)
    int ntransposed = 0, kt = 0, q = 0;
    for (int k = 1; k < c.M; ++k) {
        const i64 s0 = c.strides[k][0] < 0 ? -c.strides[k][0] : c.strides[k][0];
        if (s0 <= 1) continue;  // unit-stride or broadcast along dim 0
        for (int d = 1; d < c.N; ++d)
            if (c.strides[k][d] == 1 || c.strides[k][d] == -1) {
                ++ntransposed;
                kt = k;
                q = d;
                break;
            }
    }
    if (ntransposed == 1 && c.dims[0] >= GROUP_TMIN && c.dims[q] >= GROUP_TMIN) {
        m.form = GROUP_FORM_TRANSPOSING;
        m.kt = kt;
        m.q = q;
        m.tbase = m.base[kt];
        m.tsp = c.strides[kt][0];
        m.tsq = c.strides[kt][q];
        m.tdtype = c.dtype[kt];
        m.tconj = c.conj[kt];
        for (int k = 0; k < c.M; ++k) m.qstride[k] = c.strides[k][q];
        m.ntp = (uint32_t)((c.dims[0] + GROUP_TILE - 1) / GROUP_TILE);
        m.ntq = (uint32_t)((c.dims[q] + GROUP_TILE - 1) / GROUP_TILE);
        i64 wgs = (i64)m.ntp * m.ntq;
        for (int d = 1; d < c.N; ++d)
            if (d != q) wgs *= c.dims[d];
        return wgs;
    }
    m.form = GROUP_FORM_LINEAR;
    return (c.total + GROUP_CHUNK - 1) / GROUP_CHUNK;
}

// Independence: no member's destination range may meet a range of ANOTHER member.  One sweep over the ranges sorted by their
// start: a range meets an earlier one iff that one ends behind its start, so the two furthest-reaching ends seen so far (of
// different members) decide -- among all ranges for a destination, among the destinations for an input.
struct Range {
    uintptr_t lo, hi;
    int member;
    bool write;
};
struct Reach {  // the furthest ends seen so far, of two different members
    uintptr_t hi[2] = {0, 0};
    int member[2] = {-1, -1};
    void add(uintptr_t h, int mem) {
        if (mem == member[0]) hi[0] = std::max(hi[0], h);
        else if (member[0] < 0 || h > hi[0]) {
            if (member[0] >= 0) { hi[1] = hi[0]; member[1] = member[0]; }
            hi[0] = h;
            member[0] = mem;
        } else if (mem == member[1]) hi[1] = std::max(hi[1], h);
        else if (member[1] < 0 || h > hi[1]) { hi[1] = h; member[1] = mem; }
    }
    // a member other than `mem` whose range ends behind `lo`, or -1
    int meets(uintptr_t lo, int mem) const {
        for (int i = 0; i < 2; ++i)
            if (member[i] >= 0 && member[i] != mem && hi[i] > lo) return member[i];
        return -1;
    }
};

int check_independent(std::vector<Range>& rs) {
    std::sort(rs.begin(), rs.end(), [](const Range& a, const Range& b) { return a.lo != b.lo ? a.lo < b.lo : a.member < b.member; });
    Reach all, writes;
    for (const Range& r : rs) {
        const int other = (r.write ? all : writes).meets(r.lo, r.member);
        if (other >= 0) {
            const int wm = r.write ? r.member : other, om = r.write ? other : r.member;
            return set_error(SMR_EUNSUPPORTED, member_tag(std::max(wm, om)) + ": the destination's byte range of member " + std::to_string(wm) +
                                                   " meets a byte range of member " + std::to_string(om) +
                                                   " (pass SMR_GROUP_INDEPENDENT if no element is shared, e.g. interleaved blocks of one parent)");
        }
        all.add(r.hi, r.member);
        if (r.write) writes.add(r.hi, r.member);
    }
    return SMR_OK;
}

// the union of `rs` as sorted ranges, overlapping and adjacent ones merged (a 128-member group hands a sequence's scheduler a
// handful of ranges, not 256)
Spans merged(Spans rs) {
    std::sort(rs.begin(), rs.end());
    Spans out;
    for (const auto& r : rs) {
        if (r.second <= r.first) continue;
        if (!out.empty() && r.first <= out.back().second) out.back().second = std::max(out.back().second, r.second);
        else out.push_back(r);
    }
    return out;
}

// workgroups [first_wg[i], first_wg[i] + wgs) go to member i: the one place the group's grid grows
int assign_workgroups(GroupPlan& g, int i, i64 wgs) {
    const i64 grid = (i64)g.first_wg[(size_t)i] + wgs;
    if (grid > 0x7fffffffLL) return set_error(SMR_EUNSUPPORTED, member_tag(i) + ": the group needs more than 2^31 - 1 workgroups");
    g.first_wg[(size_t)i + 1] = (uint32_t)grid;
    return SMR_OK;
}

// ---- map groups ------------------------------------------------------------------------------------------------------------------
// member i: under SMR_GROUP_MEMBER_SCALARS its row of the constant table (what its own canonicalisation handed the functor), its body
int map_member(GroupPlan& g, int i, const Canon& c, bool own_scalars) {
    GroupMapPlan& mp = g.map;
    if (own_scalars) {
        const bool native_row = native_with_consts(g.c);
        if (i == 0) mp.W = native_row ? 4 : (c.bitcopy ? 0 : 2 * c.prog.nconst);
        const double* row = native_row ? c.fc : c.prog.consts;
        mp.consts.insert(mp.consts.end(), row, row + mp.W);
    }
    const i64 wgs = plan_member(c, mp.members[(size_t)i]);
    (mp.members[(size_t)i].form ? mp.ntrans : mp.nlinear) += 1;
    return assign_workgroups(g, i, wgs);
}

// bit-equal rows (-0.0 differs from 0.0), or none: the group is the one the call without the flag plans, no third table
void map_finish(GroupMapPlan& mp, int count) {
    const size_t row = sizeof(double) * (size_t)mp.W;
    for (int i = 1; i < count && !mp.varc; ++i) mp.varc = row && std::memcmp(mp.consts.data(), mp.consts.data() + (size_t)i * mp.W, row) != 0;
    if (!mp.varc) {
        std::vector<double>().swap(mp.consts);
        mp.W = 0;
    }
}

const char* independent_tag(uint32_t flags) { return (flags & SMR_GROUP_INDEPENDENT) ? " independent=asserted" : ""; }

void map_describe(GroupPlan& g, uint32_t flags) {
    static const char* names[FK_COUNT] = {"prog", "ident", "add2", "add3", "add4", "scale", "sym", "axpy", "axpby", "abs2", "mul2", "expr5"};
    const Canon& c = g.c;
    // what launch_group_ct() does: with_prog (runtime compilation first) for a mixed group and for an f without a native functor.
    // FK_PROG has a bit in GROUP_FMASK like every kind, so the mask alone does not tell
    const int fk = (!c.mixed && (GROUP_FMASK & fbit(c.fkind))) ? c.fkind : FK_PROG;
    g.jit = options().jit && !c.bitcopy && fk == FK_PROG;
    char buf[256];
    std::snprintf(buf, sizeof buf, "family=group members=%zu grid=%u linear=%d transposing=%d f=%s jit=%d bytes=%lld%s%s", g.rank.size(), g.first_wg.back(),
                  g.map.nlinear, g.map.ntrans, c.bitcopy ? "bitcopy" : names[fk], g.jit ? 1 : 0, (long long)g.algbytes, independent_tag(flags),
                  (flags & SMR_GROUP_MEMBER_SCALARS) ? (g.map.varc ? " scalars=member" : " scalars=shared") : "");
    g.desc = buf;
}

// ---- contraction groups ------------------------------------------------------------------------------------------------------
// the descriptor of a member tiled along di / dj (the tile-dependent fields are set again by contract_finish)
void contract_member(GroupContractMemberD& m, const Canon& c, int di, int dj) {
    std::memset(&m, 0, sizeof m);
    for (int k = 0; k < 3; ++k) m.base[k] = (char*)c.base[k] + c.offsets[k] * (i64)c.esize[k];
    contract_fill(m, c, di, dj, contract_vec_of(c, di, dj, nullptr), 1);
}

// Every member's tiles, slices and workgroups on tile 16 * rb with want[i] slices asked for member i (the single call's slice
// arithmetic, smr_contract.h: contract_slices; a member left with one slice is an unsplit member), and -- when at least one member
// is split -- the tables of the split form: per member S, cps, tiles and the offset of its partials, and the fold launch's prefix sums
// (rb^2 workgroups per tile of a split member, none for the others).  With no member split the plan is exactly the unsplit one.
int contract_layout(GroupPlan& g, int es, int rb, const std::vector<i64>& want) {
    GroupContractPlan& cp = g.contract;
    const size_t count = cp.members.size();
    const i64 tile2 = (i64)(CONTRACT_LANES * rb) * (CONTRACT_LANES * rb);
    cp.rb = rb;
    cp.split.assign(count, GroupSplitD{0, 0, 1, 0});
    cp.fold_first.assign(count + 1, 0);
    cp.nsplit = cp.max_s = 0;
    g.first_wg.assign(count + 1, 0);
    long double elems = 0;
    i64 fold = 0;
    for (size_t i = 0; i < count; ++i) {
        GroupContractMemberD& m = cp.members[i];
        const i64 tiles = contract_set_tile(m, es, rb);
        GroupSplitD& sp = cp.split[i];
        i64 cps = 0;
        const i64 S = tiles > 0x7fffffffLL ? 1 : contract_slices(m.Q * m.nkc, want[i], cps);
        if (S >= 2 && (i64)g.first_wg[i] + tiles * S > 0x7fffffffLL)
            return set_error(SMR_EINVAL, member_tag((int)i) + ": group_contract_split: the slices need more than 2^31 - 1 workgroups");
        if (int rc = assign_workgroups(g, (int)i, tiles * S)) return rc;
        sp.S = (uint32_t)S;
        sp.cps = cps;
        sp.tiles = (uint32_t)tiles;
        if (S >= 2) {
            sp.part_off = (i64)elems;
            elems += (long double)tiles * (long double)S * (long double)tile2;
            fold += tiles * rb * rb;
            if (elems * es > 2147483648.0L || fold > 0x7fffffffLL)
                return set_error(SMR_EUNSUPPORTED, member_tag((int)i) + ": group_contract_split: the group's partials would exceed the limit of 2^31 bytes");
            ++cp.nsplit;
            cp.max_s = std::max(cp.max_s, (int)S);
        }
        cp.fold_first[i + 1] = (uint32_t)fold;
    }
    if (cp.nsplit == 0) {
        std::vector<GroupSplitD>().swap(cp.split);
        std::vector<uint32_t>().swap(cp.fold_first);
    }
    cp.scratch_bytes = (size_t)(elems * es);
    return SMR_OK;
}

// group_contract_split = 1: the single call's contract_split_rule (smr_plan_contract.cpp; the constants and the three bounds on a
// member's slices are shared with it, smr_contract.h) read over the whole group.  Only for a group whose unsplit plan, on the tile
// `rb` the unsplit rule chose, has fewer than 256 workgroups.  Of the tiles allowed (32 then 16, those whose LDS fits `cap`; cap == 0:
// the tile is forced, only `rb`) the largest on which the members' tiles * smax_i sum to at least 256, else the tile that allows the
// most workgroups; smax_i < 2 counts as one slice, and a tile on which no member can take two slices is no candidate.  With G the
// unsplit grid on that tile every member gets S_i = clamp(ceil(512 / G), 1, smax_i) slices.  False: the group is not split.
// The constants were measured for single calls (profiles/contract_split.txt).  Measured for groups with
// tools/group_contract_split_cases.py (profiles/group_contract_split.txt, MI355X; us per execution of the whole group, the unsplit
// group -> the rule's group; the unsplit group's run-to-run spread is 0.1 - 1 us):
//   every row the rule splits wins: 4 x (32, 32, 4096) Float64 118.66 -> 17.01 (32 x 32 tiles, 64 slices, 256 workgroups); 16 x (32,
//     32, 4096) Float64 121.40 -> 21.56 (32 x 32, 32 slices, 512 workgroups); 16 x (16, 16, 65536) Float32 1083.66 -> 114.32 (32 x 32,
//     32 slices).  No measured row that it splits loses, so no row is excluded and the constants stay the single call's;
//   the larger tile first: 16 x (32, 32, 4096), 32 slices on 32 x 32 tiles 21.01 against 32 slices on 16 x 16 tiles 29.64;
//   the gate (fewer than 256 unsplit workgroups) is conservative: the rows it leaves alone all have a forced form that wins -- 64 x
//     (32, 32, 4096) Float64 122.99 -> 42.75 (S32 / 32 x 32), 16 x (64, 64, 4096) ComplexF64 328.14 -> 89.30, the group of 1000 x (32, 32,
//     32) + 2 x (32, 32, 16384) 1047.25 -> 40.50 (S64 / 32 x 32), 64 x (64, 64, 4096) Float32 with exactly 256 workgroups 117.82 -> 89.64
//     (S8 / 32 x 32).  A gate on the longest member's walk instead of the grid: not designed, not measured.
bool contract_group_rule(const std::vector<GroupContractMemberD>& members, int es, i64 cap, int& rb, std::vector<i64>& want) {
    std::vector<GroupContractMemberD> ms = members;  // (contract_set_tile writes the tile-dependent fields)
    std::vector<i64> smax(ms.size());
    i64 G = 0;  // the unsplit grid on the tile surveyed last
    // every member's most slices on tile 16 * r; returns the sum of tiles * smax, 0 when no member can take two slices
    auto survey = [&](int r) {
        i64 W = 0;
        bool any = false;
        G = 0;
        for (size_t i = 0; i < ms.size(); ++i) {
            GroupContractMemberD& m = ms[i];
            const i64 tiles = contract_set_tile(m, es, r);
            smax[i] = std::max<i64>(1, contract_split_smax(es, m.dims[m.di], m.dims[m.dj], m.K, m.Q, m.Q * m.nkc, tiles, CONTRACT_LANES * r));
            any = any || smax[i] >= 2;
            G += tiles;
            W += tiles * smax[i];
        }
        return any ? W : (i64)0;
    };
    (void)survey(rb);
    if (G >= 256) return false;
    int best = 0;
    i64 best_w = 0;
    for (int r = 2; r >= 1; r >>= 1) {
        if (cap ? (i64)contract_lds(es, r) > cap : r != rb) continue;
        const i64 W = survey(r);
        if (W >= 256) {
            best = r;
            break;
        }
        if (W > best_w) {
            best_w = W;
            best = r;
        }
    }
    if (!best) return false;
    (void)survey(best);
    const i64 s = (CONTRACT_SPLIT_TARGET + G - 1) / G;
    for (size_t i = 0; i < ms.size(); ++i) want[i] = std::max<i64>(1, std::min(s, smax[i]));
    rb = best;
    return true;
}

// the group's tile, then every member's tiles and workgroups
int contract_finish(GroupPlan& g) {
    i64 wgs32 = 0, outputs = 0;  // over the group: workgroups on 32 x 32 tiles, destination elements
    for (const GroupContractMemberD& m : g.contract.members) {
        i64 rest = 1;
        for (int n = 0; n < m.nrd; ++n) rest *= m.dims[m.rdim[n]];
        wgs32 += ((m.dims[m.di] + 31) / 32) * ((m.dims[m.dj] + 31) / 32) * rest;
        outputs += m.dims[m.di] * m.dims[m.dj] * rest;
    }
    // One tile size per group.  The single call's rule, read over the whole group: 32 x 32 (2 x 2 outputs per lane) when the group
    // then still has a workgroup per CU -- 256, the threshold measured for single calls (smr_plan_contract.cpp) -- AND those tiles are
    // at least half full over the group (outputs >= 1/2 * 1024 * tiles): members of 16 or 24 along a dim would otherwise stage and
    // compute mostly padding.  Measured (tools/group_contract_vs_single.py, profiles/group_contract.txt): 64 blocks of 64^3 Float64,
    // every tile of either size full, 32 x 32 7.82 us against 16 x 16 8.15 us -- what this rule picks there.  The half-full condition
    // is NOT measured: that is the only row timed under both tiles, and none has partly filled 32 x 32 tiles.
    const int es = dtype_size(g.c.ct);
    const i64 force = group_contract_tile();
    int rb = force == 32 ? 2 : (force == 16 ? 1 : ((wgs32 >= 256 && 2 * outputs >= 1024 * wgs32) ? 2 : 1));
    // the LDS is static: a budget below the tile's takes 16 x 16, or refuses
    const i64 cap = std::min<i64>(options().max_lds_bytes, 65536);
    while (rb >= 1 && (i64)contract_lds(es, rb) > cap) rb >>= 1;
    if (rb < 1) return set_error(SMR_EUNSUPPORTED, "smr_group_create: the 16 x 16 tile of a contraction group does not fit max_lds_bytes");
    // the split form (opt-in: another accumulation order for the members it splits): forced slices on the tile chosen above, or the
    // group rule, which picks tile and slices together
    const i64 split = group_contract_split();
    std::vector<i64> want(g.contract.members.size(), split >= 2 ? split : 1);  // slices asked for, per member
    if (split == 1) {
        const int rb0 = rb;
        if (contract_group_rule(g.contract.members, es, force ? 0 : cap, rb, want) && contract_layout(g, es, rb, want) == SMR_OK) return SMR_OK;
        rb = rb0;  // not split, or its partials or its grid are beyond the limits: the unsplit plan
        (void)set_error(SMR_OK, std::string());  // (a limit's message is not this call's)
        want.assign(want.size(), 1);
    }
    return contract_layout(g, es, rb, want);
}

// SMR_GROUP_CONTRACT_SCALARS, member i: its row of the constant table, the constants of its own canonicalisation (ProgD::consts; for
// the mul! form that is the pair (re, im) of alpha, which FMul2Scale reads like FScale reads Canon::fc)
void contract_member_consts(GroupContractPlan& cp, int i, const Canon& c) {
    if (i == 0) cp.W = 2 * c.prog.nconst;
    cp.consts.insert(cp.consts.end(), c.prog.consts, c.prog.consts + cp.W);
}

// bit-equal rows, or none: the plan is the unflagged one, no table and today's f path (map_finish).  Otherwise the launch reads the
// member's row; the mul! form on operands of the compute class then runs the natively compiled functor
void contract_consts_finish(GroupPlan& g, int count) {
    GroupContractPlan& cp = g.contract;
    const size_t row = sizeof(double) * (size_t)cp.W;
    for (int i = 1; i < count && !cp.varc; ++i) cp.varc = row && std::memcmp(cp.consts.data(), cp.consts.data() + (size_t)i * cp.W, row) != 0;
    if (!cp.varc) {
        std::vector<double>().swap(cp.consts);
        cp.W = 0;
    }
    cp.mul2scale = cp.varc && !g.c.mixed && prog_is_mul2scale(g.c);
}

void contract_describe(GroupPlan& g, uint32_t flags) {
    static const char* ops[] = {"none", "+", "*", "min", "max", "&", "|"};
    // launch_group_contract_ct(): the product of same-typed operands is native, every other f a program -- but for the mul! form
    // in a group with a row of constants per member (launch_group_contract_varc_ct())
    const bool native = !g.c.mixed && (g.c.fkind == FK_MUL2 || g.contract.mul2scale);
    const int es = dtype_size(g.c.ct), rb = g.contract.rb;
    g.jit = options().jit && !native;
    char buf[256], split[160] = "";
    // the split form: members split, the largest S, the fold launch's grid and the group's partials (grid= is the main launch's)
    if (g.contract.nsplit)
        std::snprintf(split, sizeof split, " split=%d kparts=%d fold=second-launch fold_grid=%u scratch=%zu", g.contract.nsplit, g.contract.max_s,
                      g.contract.fold_first.back(), g.contract.scratch_bytes);
    std::snprintf(buf, sizeof buf, "family=group kind=contract members=%zu grid=%u tile=%d k=%d lds=%zu f=%s op=%s jit=%d bytes=%lld", g.rank.size(), g.first_wg.back(),
                  CONTRACT_LANES * rb, contract_tk(es, rb), contract_lds(es, rb), g.contract.mul2scale ? "mul2scale" : (native ? "mul2" : "prog"), g.c.redop >= 0 && g.c.redop < 7 ? ops[g.c.redop] : "?",
                  g.jit ? 1 : 0, (long long)g.algbytes);
    g.desc = std::string(buf) + split + independent_tag(flags) +
             ((flags & SMR_GROUP_CONTRACT_SCALARS) ? (g.contract.varc ? " scalars=member" : " scalars=shared") : "");
}

// ---- reduction groups ------------------------------------------------------------------------------------------------------------
// member i, a complete reduction: W = min(ceil(total / REDUCE_ALL_PER_BLOCK), REDUCE_FOLD_MAX) workgroups -- what plan_reduce_all gives a
// single call under "reduce_blocks" = REDUCE_FOLD_MAX, the most partials one arrival counter folds inside a launch -- and the body the
// single call would take (reduce_all_vector; the base pointers are fixed, so alignment is decided here).  A member with W > 1 gets the
// next W slots of the group's partials and the next counter.
int reduce_admit(int i, const Canon& c) {
    if (c.nout != 1 || c.NK != 0)
        return set_error(SMR_EUNSUPPORTED, member_tag(i) + " is not a complete reduction: it keeps a dim of extent > 1 (" + std::to_string((long long)c.nout) +
                                               " destination elements); a reduction group (SMR_GROUP_REDUCE) holds complete reductions only");
    if (c.M < 2) return set_error(SMR_EUNSUPPORTED, member_tag(i) + " has no input: a complete reduction in a group reads 1 .. SMR_MAXM - 1 distinct inputs");
    return SMR_OK;
}

int reduce_member(GroupPlan& g, int i, const Canon& c) {
    GroupReducePlan& rp = g.reduce;
    GroupReduceMemberD& m = rp.members[(size_t)i];
    std::memset(&m, 0, sizeof m);
    for (int k = 0; k < c.M; ++k) {
        m.base[k] = (char*)c.base[k] + c.offsets[k] * (i64)c.esize[k];
        for (int d = 0; d < c.N; ++d) m.strides[k][d] = c.strides[k][d];
    }
    for (int d = 0; d < MAXN; ++d) m.dims[d] = d < c.N ? c.dims[d] : 1;
    m.total = c.total;
    m.N = c.N;
    m.beta[0] = c.initarg[0];
    m.beta[1] = c.initarg[1];
    const bool vec = reduce_all_vector(c, nullptr);
    m.form = vec ? GROUP_FORM_REDUCE_VECTOR : GROUP_FORM_REDUCE_STRIDED;
    (vec ? rp.nvec : rp.nstrided) += 1;
    const i64 W = std::max<i64>(1, std::min<i64>((c.total + REDUCE_ALL_PER_BLOCK - 1) / REDUCE_ALL_PER_BLOCK, REDUCE_FOLD_MAX));
    if (W > 1) {
        m.part_off = rp.slots;
        m.counter = rp.npartials;
        rp.slots += W;
        rp.npartials += 1;
    }
    rp.max_in_bytes = std::max(rp.max_in_bytes, (long double)c.total * c.esize[1]);
    return assign_workgroups(g, i, W);
}

void reduce_describe(GroupPlan& g, uint32_t flags) {
    static const char* names[FK_COUNT] = {"prog", "ident", "add2", "add3", "add4", "scale", "sym", "axpy", "axpby", "abs2", "mul2", "expr5"};
    static const char* ops[] = {"none", "+", "*", "min", "max", "&", "|"};
    const Canon& c = g.c;
    GroupReducePlan& rp = g.reduce;
    // launch_group_reduce_ct(): a functor of the mask when the operand types are the compute class's, every other f a program
    const int fk = (!c.mixed && (GROUP_REDUCE_FMASK & fbit(c.fkind))) ? c.fkind : FK_PROG;
    g.jit = options().jit && fk == FK_PROG;
    rp.scratch_bytes = (size_t)rp.slots * (size_t)dtype_size(c.ct) + (size_t)rp.npartials * sizeof(unsigned);
    char buf[320];
    std::snprintf(buf, sizeof buf, "family=group kind=reduce members=%zu grid=%u vec=%d strided=%d f=%s op=%s jit=%d partials=%d scratch=%zu bytes=%lld%s", g.rank.size(),
                  g.first_wg.back(), rp.nvec, rp.nstrided, names[fk], c.redop >= 0 && c.redop < 7 ? ops[c.redop] : "?", g.jit ? 1 : 0, rp.npartials, rp.scratch_bytes,
                  (long long)g.algbytes, independent_tag(flags));
    g.desc = buf;
}

// ---- partial reduction groups ------------------------------------------------------------------------------------------------------
// member i, a reduction that may keep dims: the general form of REDUCE_PART with the reduced range in ONE piece.  TR lanes per
// destination element as plan_part_general gives that canonical problem (reduce_part_general_lanes, smr_plan_reduce.cpp), a workgroup
// owns 256 / TR consecutive destination elements, W = ceil(nout / (256 / TR)).  Never split: no partials, no counters, no scratch.
int reduce_part_admit(int i, const Canon& c) {
    if (c.M < 2) return set_error(SMR_EUNSUPPORTED, member_tag(i) + " has no input: a reduction in a group reads 1 .. SMR_MAXM - 1 distinct inputs");
    return SMR_OK;
}

int reduce_part_member(GroupPlan& g, int i, const Canon& c) {
    GroupReducePartPlan& rp = g.reduce_part;
    GroupReducePartMemberD& m = rp.members[(size_t)i];
    std::memset(&m, 0, sizeof m);
    for (int k = 0; k < c.M; ++k) {
        m.base[k] = (char*)c.base[k] + c.offsets[k] * (i64)c.esize[k];
        for (int d = 0; d < c.N; ++d) m.strides[k][d] = c.strides[k][d];
    }
    for (int d = 0; d < MAXN; ++d) m.dims[d] = d < c.N ? c.dims[d] : 1;
    m.nout = std::max<i64>(1, c.nout);
    m.nred = c.total / m.nout;
    m.N = c.N;
    m.NK = std::min(c.NK, c.N);
    m.beta[0] = c.initarg[0];
    m.beta[1] = c.initarg[1];
    const int tr = reduce_part_general_lanes(c, m.nred);
    while ((1 << m.trlog) < tr) ++m.trlog;
    rp.lanes[m.trlog] += 1;
    const i64 ob = 256 >> m.trlog;
    return assign_workgroups(g, i, (m.nout + ob - 1) / ob);
}

void reduce_part_describe(GroupPlan& g, uint32_t flags) {
    static const char* names[FK_COUNT] = {"prog", "ident", "add2", "add3", "add4", "scale", "sym", "axpy", "axpby", "abs2", "mul2", "expr5"};
    static const char* ops[] = {"none", "+", "*", "min", "max", "&", "|"};
    const Canon& c = g.c;
    // launch_group_reduce_part_ct(): a functor of the mask when the operand types are the compute class's, every other f a program
    const int fk = (!c.mixed && (GROUP_REDUCE_FMASK & fbit(c.fkind))) ? c.fkind : FK_PROG;
    g.jit = options().jit && fk == FK_PROG;
    std::string lanes;  // the distinct lanes per output, ascending, each with its member count
    for (int j = 0; j <= 8; ++j)
        if (g.reduce_part.lanes[j]) lanes += (lanes.empty() ? "" : ",") + std::to_string(1 << j) + ":" + std::to_string(g.reduce_part.lanes[j]);
    char buf[320];
    std::snprintf(buf, sizeof buf, "family=group kind=reduce_part members=%zu grid=%u lanes=%s f=%s op=%s jit=%d bytes=%lld%s", g.rank.size(), g.first_wg.back(),
                  lanes.c_str(), names[fk], c.redop >= 0 && c.redop < 7 ? ops[c.redop] : "?", g.jit ? 1 : 0, (long long)g.algbytes, independent_tag(flags));
    g.desc = buf;
}

}  // namespace

int plan_group(const smr_problem* members, int count, uint32_t flags, GroupPlan& g) {
    const bool contract_scalars = (flags & SMR_GROUP_CONTRACT_SCALARS) != 0;
    const bool own_scalars = (flags & SMR_GROUP_MEMBER_SCALARS) != 0, independent = (flags & SMR_GROUP_INDEPENDENT) != 0;
    const bool reduce = (flags & SMR_GROUP_REDUCE) != 0;        // a reduction group: every member a complete reduction ...
    const bool part = (flags & SMR_GROUP_REDUCE_PART) != 0;     // ... or, with this flag as well, a reduction that may keep dims
    const bool contraction = !reduce && members[0].redop != SMR_RED_NONE;  // else the kind is member 0's
    if (part && !reduce)
        return set_error(SMR_EUNSUPPORTED, "smr_group_create: SMR_GROUP_REDUCE_PART without SMR_GROUP_REDUCE: the flag turns a reduction group into a partial reduction group and is valid only together with it");
    // (SMR_GROUP_CONTRACT_SCALARS first: its refusals name it, whatever else is set; the refusals of flag 2 keep their text)
    if (contract_scalars && reduce)
        return set_error(SMR_EUNSUPPORTED, "smr_group_create: SMR_GROUP_CONTRACT_SCALARS with a reduction group (SMR_GROUP_REDUCE): per-member constants of f are not supported there");
    if (contract_scalars && !contraction)
        return set_error(SMR_EUNSUPPORTED, "smr_group_create: SMR_GROUP_CONTRACT_SCALARS with a map group (member 0 is a map): the flag is for contraction groups, a map group takes SMR_GROUP_MEMBER_SCALARS");
    if (contract_scalars && own_scalars)
        return set_error(SMR_EUNSUPPORTED, "smr_group_create: SMR_GROUP_CONTRACT_SCALARS together with SMR_GROUP_MEMBER_SCALARS: a contraction group takes the former alone");
    if (reduce && own_scalars)
        return set_error(SMR_EUNSUPPORTED, "smr_group_create: SMR_GROUP_MEMBER_SCALARS with a reduction group (SMR_GROUP_REDUCE): per-member constants of f are not supported there");
    if (contraction && own_scalars)
        return set_error(SMR_EUNSUPPORTED, "smr_group_create: SMR_GROUP_MEMBER_SCALARS with a contraction group (member 0 is a reduction): per-member constants of f are not supported there");
    g.kind = part ? GROUP_REDUCE_PART : (reduce ? GROUP_REDUCE : (contraction ? GROUP_CONTRACT : GROUP_MAP));
    g.first_wg.assign((size_t)count + 1, 0);
    g.rank.resize((size_t)count);
    if (part) g.reduce_part.members.resize((size_t)count);
    else if (reduce) g.reduce.members.resize((size_t)count);
    else if (contraction) g.contract.members.resize((size_t)count);
    else g.map.members.resize((size_t)count);
    std::vector<Range> ranges;
    Spans rd, wr;
    for (int i = 0; i < count; ++i) {
        const smr_problem& p = members[i];
        // admit: a map group holds maps only, a contraction group reductions of the contraction shape only, a reduction group
        // complete reductions only, a partial reduction group reductions only
        if (part && p.redop == SMR_RED_NONE)
            return set_error(SMR_EUNSUPPORTED, member_tag(i) + " is a map; a partial reduction group (SMR_GROUP_REDUCE | SMR_GROUP_REDUCE_PART) holds reductions only");
        if (reduce && p.redop == SMR_RED_NONE)
            return set_error(SMR_EUNSUPPORTED, member_tag(i) + " is a map; a reduction group (SMR_GROUP_REDUCE) holds complete reductions only");
        if (!reduce && (p.redop != SMR_RED_NONE) != contraction)
            return set_error(SMR_EUNSUPPORTED, member_tag(i) + (contraction ? " is a map; a contraction group (member 0 is a reduction) holds contractions only"
                                                                             : " is a reduction; a group holds maps only"));
        Canon ci;
        Canon& c = i == 0 ? g.c : ci;
        if (int rc = canonicalise(&p, c)) return set_error(rc, member_tag(i) + ": " + smr_last_error());
        int di = -1, dj = -1;
        if (contraction && !contract_shape(c, di, dj))
            return set_error(SMR_EUNSUPPORTED, member_tag(i) + " is a reduction, but not of the contraction shape: two inputs that vary along different kept dims of "
                                                                "extent > 1 and both along a reduced dim, neither on the destination's buffer; a group holds maps only, or such contractions only");
        if (reduce)
            if (int rc = part ? reduce_part_admit(i, c) : reduce_admit(i, c)) return rc;
        if (i > 0) {
            const std::string why = mismatch(g.c, c, own_scalars || contract_scalars);
            if (!why.empty()) return set_error(SMR_EUNSUPPORTED, member_tag(i) + " " + why);
        }
        if (c.total > 0x7fffffffLL) return set_error(SMR_EUNSUPPORTED, member_tag(i) + " has more than 2^31 - 1 box elements");
        g.rank[(size_t)i] = c.N;
        g.algbytes += c.algbytes;
        // the bounding byte range of every operand: compared for the independence check (skipped under SMR_GROUP_INDEPENDENT) and
        // always kept as the group's footprint, which stays conservative for interleaved members
        for (int k = 0; k < c.M; ++k) {
            Range r{0, 0, i, k == 0};
            operand_span(c, k, c.base[k], r.lo, r.hi);
            (r.write ? wr : rd).emplace_back(r.lo, r.hi);
            // a contraction or a complete reduction accumulates into its destination unless the initop replaces the old value: the footprint then says
            // that it is read (like footprint() in smr_api.cpp for every reduction), so that a recorded group acquires what the
            // sequence wrote there
            if (r.write && (contraction || reduce) && c.initop != SMR_INIT_ZERO && c.initop != SMR_INIT_CONST) rd.emplace_back(r.lo, r.hi);
            if (!independent) ranges.push_back(r);
        }
        // a map member takes its workgroups here; a contraction's depend on the tile, which contract_finish picks for the whole group
        if (reduce) {
            if (int rc = part ? reduce_part_member(g, i, c) : reduce_member(g, i, c)) return rc;
        } else if (contraction) {
            contract_member(g.contract.members[(size_t)i], c, di, dj);
            if (contract_scalars) contract_member_consts(g.contract, i, c);
        }
        else if (int rc = map_member(g, i, c, own_scalars)) return rc;
    }
    if (g.kind == GROUP_MAP) map_finish(g.map, count);
    if (g.kind == GROUP_CONTRACT && contract_scalars) contract_consts_finish(g, count);
    if (g.kind == GROUP_CONTRACT)
        if (int rc = contract_finish(g)) return rc;  // (a reduction group decides nothing over the whole group)
    if (int rc = independent ? SMR_OK : check_independent(ranges)) return rc;
    g.rd = merged(std::move(rd));
    g.wr = merged(std::move(wr));
    if (part) reduce_part_describe(g, flags);
    else if (reduce) reduce_describe(g, flags);
    else if (contraction) contract_describe(g, flags);
    else map_describe(g, flags);
    return SMR_OK;
}

}  // namespace smr
