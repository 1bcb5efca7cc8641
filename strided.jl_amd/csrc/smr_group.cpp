// smr_group.cpp -- grouped launches (include/strided_hip.h: smr_group_*): the group planner and its C ABI.
// A group is K independent small maps that share one functor f and one operand-type signature and differ in rank, dims, strides,
// base pointers and offsets; smr_group_execute runs them as ONE launch of the kernel in smr_k_group.hip.  Planning is host
// arithmetic: every member is canonicalised like a single call, checked against member 0, given one of the kernel's two bodies and
// a contiguous range of workgroups.  Under SMR_GROUP_MEMBER_SCALARS the values of f's constants may differ: every member keeps the
// constants of its own canonicalisation as a row of a third table.  The device tables are uploaded by smr_group_prepare or the first execution.  The planner also
// keeps the byte ranges one execution reads and writes: the footprint of a group recorded in a sequence (smr_seq_add_group).
// A group whose member 0 is a reduction is a CONTRACTION group: every member is an outer-product reduction of FAM_CONTRACT's shape
// (smr_plan_contract.cpp: contract_shape) with one f, one op and one initop code; the launch is the kernel in smr_k_gcontract.hip.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

#include "smr_contract.h"
#include "smr_direct.h"
#include "smr_dispatch.h"
#include "smr_group.h"

namespace smr {

i64& group_max_bytes() {
    // largest member (algorithmic bytes) the Python front still defers into a group.  16 MiB is the 32^4 Float64 row of
    // profiles/group_launch.txt: the largest measured member at which one group of 8 beats the 8 single calls it replaces in the
    // front (it beats a recorded sequence only from K = 32 small members on)
    static i64 v = (i64)16 << 20;
    return v;
}

i64& group_contract_tile() {
    static i64 v = 0;
    return v;
}

namespace {

std::string member_tag(int i) { return "smr_group_create: member " + std::to_string(i); }

// does member `c` run the same kernel instantiation with the same functor as member 0 (`r`)?  Empty = yes, else what differs.
// `own_scalars` (SMR_GROUP_MEMBER_SCALARS): the values of f's constants may differ, nothing else.
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
    return std::string();
}

// does the launch run a natively compiled functor that keeps constants in fields (with_functor, smr_dispatch.h)?  Its per-member
// row is Canon::fc; every other f with constants is a program (runtime-compiled or interpreted) and its row is ProgD::consts.
bool native_with_consts(const Canon& c) {
    if (c.bitcopy || c.mixed || !(GROUP_FMASK & fbit(c.fkind))) return false;
    switch (c.fkind) {
        case FK_SCALE: case FK_AXPY: case FK_AXPBY: return true;
        case FK_SYM: return c.ct != SMR_I64;
        case FK_EXPR5: return c.ct == SMR_F32 || c.ct == SMR_F64;
        default: return false;
    }
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
        m.form = 1;
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
    m.form = 0;
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

int launch_group(const GroupPlan& g, hipStream_t s) {
    if (g.kind == 1) switch (g.c.ct) {
        case SMR_F32: return launch_group_contract_ct<SMR_F32>(g, s);
        case SMR_F64: return launch_group_contract_ct<SMR_F64>(g, s);
        case SMR_C32: return launch_group_contract_ct<SMR_C32>(g, s);
        case SMR_C64: return launch_group_contract_ct<SMR_C64>(g, s);
        case SMR_I64: return launch_group_contract_ct<SMR_I64>(g, s);
        default: return set_error(SMR_EINVAL, "bad compute class");
    }
    switch (g.c.bitcopy ? SMR_F32 : g.c.ct) {
        case SMR_F32: return launch_group_ct<SMR_F32>(g, s);
        case SMR_F64: return launch_group_ct<SMR_F64>(g, s);
        case SMR_C32: return launch_group_ct<SMR_C32>(g, s);
        case SMR_C64: return launch_group_ct<SMR_C64>(g, s);
        case SMR_I64: return launch_group_ct<SMR_I64>(g, s);
    }
    return set_error(SMR_EINVAL, "bad compute class");
}

int ensure_tables(const GroupPlan& g) {
    std::lock_guard<std::mutex> lk(g.build_mu);
    if (!g.d_members) {
        const void* src = g.kind == 1 ? (const void*)g.cmembers.data() : (const void*)g.members.data();
        const size_t bytes = g.kind == 1 ? g.cmembers.size() * sizeof(GroupContractMemberD) : g.members.size() * sizeof(GroupMemberD);
        if (int rc = upload_table(&g.d_members, src, bytes, "group members")) return rc;
    }
    if (!g.d_first) {
        if (int rc = upload_table(&g.d_first, g.first_wg.data(), g.first_wg.size() * sizeof(uint32_t), "group workgroup ranges")) return rc;
    }
    if (g.varc && !g.d_consts) {
        if (int rc = upload_table(&g.d_consts, g.consts.data(), g.consts.size() * sizeof(double), "group member scalars")) return rc;
    }
    return SMR_OK;
}

const char* functor_name(const Canon& c) {
    if (c.bitcopy) return "bitcopy";
    static const char* names[FK_COUNT] = {"prog", "ident", "add2", "add3", "add4", "scale", "sym", "axpy", "axpby", "abs2", "mul2", "expr5"};
    const int k = (!c.mixed && (GROUP_FMASK & fbit(c.fkind))) ? c.fkind : FK_PROG;
    return names[k];
}

// ---- contraction groups ------------------------------------------------------------------------------------------------------
// does reduction member `c` run the kernel instantiation, f, op and initop code of member 0 (`r`)?  Empty = yes.  beta (initarg)
// is the member's own.
std::string contract_mismatch(const Canon& r, const Canon& c) {
    const std::string why = mismatch(r, c, false);
    if (!why.empty()) return why;
    if (c.redop != r.redop) return "reduces with another op than member 0";
    if (c.initop != r.initop) return "has another kind of initop than member 0 (only its argument, beta, may differ)";
    return std::string();
}

const char* redop_name(int op) {
    static const char* names[] = {"none", "+", "*", "min", "max", "&", "|"};
    return op >= 0 && op < 7 ? names[op] : "?";
}

// Plans members[0..count) as one contraction group into `g` (g.c, cmembers, first_wg, rank, rb, algbytes) and collects the operand
// ranges.  Member 0 is known to be a reduction.
int plan_contract_group(const smr_problem* members, int count, uint32_t flags, GroupPlan& g, std::vector<Range>& ranges, Spans& rd, Spans& wr, i64& grid_out) {
    g.kind = 1;
    g.cmembers.resize((size_t)count);
    i64 wgs32 = 0, outputs = 0;
    for (int i = 0; i < count; ++i) {
        const smr_problem& p = members[i];
        if (p.redop == SMR_RED_NONE) return set_error(SMR_EUNSUPPORTED, member_tag(i) + " is a map; a contraction group (member 0 is a reduction) holds contractions only");
        Canon ci;
        Canon& c = i == 0 ? g.c : ci;
        if (int rc = canonicalise(&p, c)) return set_error(rc, member_tag(i) + ": " + smr_last_error());
        int di = -1, dj = -1;
        if (!contract_shape(c, di, dj))
            return set_error(SMR_EUNSUPPORTED, member_tag(i) + " is a reduction, but not of the contraction shape: two inputs that vary along different kept dims of "
                                                                "extent > 1 and both along a reduced dim, neither on the destination's buffer; a group holds maps only, or such contractions only");
        if (i > 0) {
            const std::string why = contract_mismatch(g.c, c);
            if (!why.empty()) return set_error(SMR_EUNSUPPORTED, member_tag(i) + " " + why);
        }
        if (c.total > 0x7fffffffLL) return set_error(SMR_EUNSUPPORTED, member_tag(i) + " has more than 2^31 - 1 box elements");
        GroupContractMemberD& m = g.cmembers[(size_t)i];
        std::memset(&m, 0, sizeof m);
        for (int k = 0; k < 3; ++k) m.base[k] = (char*)c.base[k] + c.offsets[k] * (i64)c.esize[k];
        contract_fill(m, c, di, dj, contract_vec_of(c, di, dj, nullptr), 1);  // (the tile-dependent fields are set again below)
        i64 rest = 1;
        for (int n = 0; n < m.nrd; ++n) rest *= m.dims[m.rdim[n]];
        wgs32 += ((m.dims[di] + 31) / 32) * ((m.dims[dj] + 31) / 32) * rest;
        outputs += c.nout;
        g.rank[(size_t)i] = c.N;
        g.algbytes += c.algbytes;
        for (int k = 0; k < c.M; ++k) {
            Range r;
            operand_span(c, k, c.base[k], r.lo, r.hi);
            r.member = i;
            r.write = k == 0;
            (r.write ? wr : rd).emplace_back(r.lo, r.hi);
            if (!(flags & SMR_GROUP_INDEPENDENT)) ranges.push_back(r);
        }
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
    g.rb = rb;
    i64 grid = 0;
    for (int i = 0; i < count; ++i) {
        grid += contract_set_tile(g.cmembers[(size_t)i], es, rb);
        if (grid > 0x7fffffffLL) return set_error(SMR_EUNSUPPORTED, member_tag(i) + ": the group needs more than 2^31 - 1 workgroups");
        g.first_wg[(size_t)i + 1] = (uint32_t)grid;
    }
    grid_out = grid;
    return SMR_OK;
}

}  // namespace
}  // namespace smr

using namespace smr;

struct smr_group {
    GroupPlan plan;
    void* stream = nullptr;  // of member 0: drained before the tables are freed
};

// ---- hooks for smr_seq.cpp, declared in smr_direct.h (the smr_group struct is private to this file) -----------------------------------
namespace smr {
int seq_execute_group(smr_group* g, hipStream_t s, bool prepare_only) {
    if (prepare_only) return smr_group_prepare(g);
    return smr_group_execute(g, (void*)s);  // while a sequence records, the launch is appended to the recorder instead
}
void seq_footprint_group(smr_group* g, Spans& rd, Spans& wr) {
    rd.insert(rd.end(), g->plan.rd.begin(), g->plan.rd.end());
    wr.insert(wr.end(), g->plan.wr.begin(), g->plan.wr.end());
}
}  // namespace smr

extern "C" {

int smr_group_create(const smr_problem* members, int count, uint32_t flags, smr_group** out) {
    if (!members || !out) return set_error(SMR_EINVAL, "smr_group_create: null argument");
    if (count < 1 || count > 65535) return set_error(SMR_EINVAL, "smr_group_create: count must be 1..65535");
    if (flags & ~(SMR_GROUP_INDEPENDENT | SMR_GROUP_MEMBER_SCALARS)) return set_error(SMR_EINVAL, "smr_group_create: unknown flag");
    smr_group* h = new (std::nothrow) smr_group();
    if (!h) return set_error(SMR_ENOMEM, "out of host memory");
    GroupPlan& g = h->plan;
    g.first_wg.assign((size_t)count + 1, 0);
    g.rank.resize((size_t)count);
    std::vector<Range> ranges;
    Spans rd, wr;
    i64 grid = 0;
    int rc = SMR_OK;
    const bool own_scalars = (flags & SMR_GROUP_MEMBER_SCALARS) != 0;
    bool native_row = false;
    // the kind is member 0's: a reduction opens a contraction group, a map a map group (which refuses every reduction below)
    const bool contraction = members[0].redop != SMR_RED_NONE;
    if (contraction) {
        if (own_scalars) rc = set_error(SMR_EUNSUPPORTED, "smr_group_create: SMR_GROUP_MEMBER_SCALARS with a contraction group (member 0 is a reduction): per-member constants of f are not supported there");
        else rc = plan_contract_group(members, count, flags, g, ranges, rd, wr, grid);
    } else {
        g.members.resize((size_t)count);
    }
    for (int i = 0; i < count && rc == SMR_OK && !contraction; ++i) {
        const smr_problem& p = members[i];
        if (p.redop != SMR_RED_NONE) {
            rc = set_error(SMR_EUNSUPPORTED, member_tag(i) + " is a reduction; a group holds maps only");
            break;
        }
        Canon ci;
        Canon& c = i == 0 ? g.c : ci;
        rc = canonicalise(&p, c);
        if (rc) {
            rc = set_error(rc, member_tag(i) + ": " + smr_last_error());
            break;
        }
        if (i > 0) {
            const std::string why = mismatch(g.c, c, own_scalars);
            if (!why.empty()) {
                rc = set_error(SMR_EUNSUPPORTED, member_tag(i) + " " + why);
                break;
            }
        }
        if (c.total > 0x7fffffffLL) {
            rc = set_error(SMR_EUNSUPPORTED, member_tag(i) + " has more than 2^31 - 1 box elements");
            break;
        }
        if (own_scalars) {  // the member's row of the constant table: what its own canonicalisation handed the functor
            if (i == 0) {
                native_row = native_with_consts(c);
                g.W = native_row ? 4 : (c.bitcopy ? 0 : 2 * c.prog.nconst);
            }
            const double* row = native_row ? c.fc : c.prog.consts;
            g.consts.insert(g.consts.end(), row, row + g.W);
        }
        const i64 wgs = plan_member(c, g.members[(size_t)i]);
        g.rank[(size_t)i] = c.N;
        (g.members[(size_t)i].form ? g.ntrans : g.nlinear) += 1;
        grid += wgs;
        if (grid > 0x7fffffffLL) {
            rc = set_error(SMR_EUNSUPPORTED, member_tag(i) + ": the group needs more than 2^31 - 1 workgroups");
            break;
        }
        g.first_wg[(size_t)i + 1] = (uint32_t)grid;
        g.algbytes += c.algbytes;
        // the bounding byte range of every operand: compared for the independence check (skipped under SMR_GROUP_INDEPENDENT) and
        // always kept as the group's footprint, which stays conservative for interleaved members
        for (int k = 0; k < c.M; ++k) {
            Range r;
            operand_span(c, k, c.base[k], r.lo, r.hi);
            r.member = i;
            r.write = k == 0;
            (r.write ? wr : rd).emplace_back(r.lo, r.hi);
            if (!(flags & SMR_GROUP_INDEPENDENT)) ranges.push_back(r);
        }
    }
    if (rc == SMR_OK && !(flags & SMR_GROUP_INDEPENDENT)) rc = check_independent(ranges);
    if (rc) {
        delete h;
        return rc;
    }
    h->stream = members[0].stream;
    if (own_scalars) {
        // bit-equal rows (-0.0 differs from 0.0): the group is the one the call without the flag plans, no third table
        const size_t row = sizeof(double) * (size_t)g.W;
        for (int i = 1; i < count && !g.varc; ++i) g.varc = row && std::memcmp(g.consts.data(), g.consts.data() + (size_t)i * g.W, row) != 0;
        if (!g.varc) {
            std::vector<double>().swap(g.consts);
            g.W = 0;
        }
    }
    g.rd = merged(std::move(rd));
    g.wr = merged(std::move(wr));
    // what launch_group_ct() does: with_prog (runtime compilation first) for a mixed group and for an f without a native functor.
    // FK_PROG has a bit in GROUP_FMASK like every kind, so the mask alone does not tell
    g.jit = options().jit && !g.c.bitcopy && (g.c.mixed || g.c.fkind == FK_PROG || !(GROUP_FMASK & fbit(g.c.fkind)));
    char buf[256];
    if (contraction) {  // launch_group_contract_ct(): the product of same-typed operands is native, every other f a program
        const bool native = !g.c.mixed && g.c.fkind == FK_MUL2;
        g.jit = options().jit && !native;
        std::snprintf(buf, sizeof buf, "family=group kind=contract members=%d grid=%lld tile=%d k=%d lds=%zu f=%s op=%s jit=%d bytes=%lld%s", count, (long long)grid,
                      CONTRACT_LANES * g.rb, contract_tk(dtype_size(g.c.ct), g.rb), contract_lds(dtype_size(g.c.ct), g.rb), native ? "mul2" : "prog",
                      redop_name(g.c.redop), g.jit ? 1 : 0, (long long)g.algbytes, (flags & SMR_GROUP_INDEPENDENT) ? " independent=asserted" : "");
    } else {
        std::snprintf(buf, sizeof buf, "family=group members=%d grid=%lld linear=%d transposing=%d f=%s jit=%d bytes=%lld%s%s", count, (long long)grid,
                      g.nlinear, g.ntrans, functor_name(g.c), g.jit ? 1 : 0, (long long)g.algbytes, (flags & SMR_GROUP_INDEPENDENT) ? " independent=asserted" : "",
                      own_scalars ? (g.varc ? " scalars=member" : " scalars=shared") : "");
    }
    g.desc = buf;
    *out = h;
    return SMR_OK;
}

int smr_group_prepare(smr_group* g) {
    if (!g) return set_error(SMR_EINVAL, "null group");
    int rc = ensure_device();
    if (rc) return rc;
    rc = ensure_tables(g->plan);
    if (rc) return rc;
    jit_set_prepare(true);
    rc = launch_group(g->plan, (hipStream_t)g->stream);
    jit_set_prepare(false);
    return rc;
}

int smr_group_execute(smr_group* g, void* stream) {
    if (!g) return set_error(SMR_EINVAL, "null group");
    int rc = ensure_device();
    if (rc) return rc;
    rc = ensure_tables(g->plan);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)(stream ? stream : g->stream);
    // the launch goes through HIP: on a library-owned stream it is foreign work (what the library submitted directly completes first,
    // and the stream's next direct launch drains it)
    rc = fence_for_foreign_work(s);
    if (rc) return rc;
    return launch_group(g->plan, s);
}

int smr_group_describe(const smr_group* g, char* buf, size_t buflen) {
    if (!g || !buf || buflen == 0) return set_error(SMR_EINVAL, "null argument");
    std::snprintf(buf, buflen, "%s", g->plan.desc.c_str());
    return SMR_OK;
}

int64_t smr_group_algorithmic_bytes(const smr_group* g) { return g ? g->plan.algbytes : 0; }

int64_t smr_group_layout(const smr_group* g, int64_t* out, size_t cap) {
    if (!g) return 0;
    const GroupPlan& p = g->plan;
    const size_t n = p.rank.size();
    if (out)
        for (size_t i = 0; i < n; ++i) {
            const int64_t v[4] = {p.kind == 1 ? 2 : p.members[i].form, p.first_wg[i], (int64_t)p.first_wg[i + 1] - (int64_t)p.first_wg[i], p.rank[i]};
            for (size_t j = 0; j < 4; ++j)
                if (4 * i + j < cap) out[4 * i + j] = v[j];
        }
    return (int64_t)(4 * n);
}

int smr_group_destroy(smr_group* g) {
    if (!g) return SMR_OK;
    if (g->plan.d_members || g->plan.d_first || g->plan.d_consts) {
        (void)eager_fence_if_active();
        (void)hipDeviceSynchronize();  // a queued launch may still read the tables
        if (g->plan.d_members) (void)hipFree(g->plan.d_members);
        if (g->plan.d_first) (void)hipFree(g->plan.d_first);
        if (g->plan.d_consts) (void)hipFree(g->plan.d_consts);
        (void)hipGetLastError();
    }
    delete g;
    return SMR_OK;
}

}  // extern "C"
