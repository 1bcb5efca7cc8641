// smr_group.cpp -- grouped launches (include/strided_hip.h: smr_group_*): the C ABI and the launch path of a planned group.
// smr_group_create checks its arguments and has the planner (smr_plan_group.cpp: plan_group) fill a GroupPlan; the device tables
// (members, workgroup prefix sums, per-member scalars) are uploaded by smr_group_prepare or the first execution, and
// smr_group_execute runs the group as ONE launch of the kernel of its kind (smr_k_group.hip, smr_k_gcontract.hip, smr_k_greduce.hip,
// smr_k_greduce_part.hip)
// -- a contraction group with split members (option "group_contract_split") as two, through partials the group owns.  A reduction
// group (SMR_GROUP_REDUCE) owns partials and arrival counters too, and folds them inside its one launch.
#include <algorithm>
#include <cstdio>
#include <iterator>
#include <new>

#include "smr_direct.h"
#include "smr_group.h"

namespace smr {

i64& group_max_bytes() {
    // largest member (algorithmic bytes) the Python front still defers into a group.  16 MiB is the 32^4 Float64 row of
    // profiles/group_launch.txt: the largest measured member at which one group of 8 beats the 8 single calls it replaces in the
    // front (it beats a recorded sequence only from K = 32 small members on)
    static i64 v = (i64)16 << 20;
    return v;
}

namespace {

// the launcher of the group's kind in the object of compute class CT (a bit copy, never a contraction, goes through Float32's)
template <int CT>
int launch_group_in(const GroupPlan& g, hipStream_t s) {
    if (g.kind == GROUP_REDUCE_PART) return launch_group_reduce_part_ct<CT>(g, s);
    if (g.kind == GROUP_REDUCE) return launch_group_reduce_ct<CT>(g, s);
    if (g.kind == GROUP_CONTRACT && g.contract.varc)  // per-member constants of f: the bodies that read the member's row
        return g.contract.nsplit ? launch_group_contract_split_varc_ct<CT>(g, s) : launch_group_contract_varc_ct<CT>(g, s);
    if (g.kind == GROUP_CONTRACT) return g.contract.nsplit ? launch_group_contract_split_ct<CT>(g, s) : launch_group_contract_ct<CT>(g, s);
    return launch_group_ct<CT>(g, s);
}

int launch_group(const GroupPlan& g, hipStream_t s) {
    switch (g.c.bitcopy ? SMR_F32 : g.c.ct) {
        case SMR_F32: return launch_group_in<SMR_F32>(g, s);
        case SMR_F64: return launch_group_in<SMR_F64>(g, s);
        case SMR_C32: return launch_group_in<SMR_C32>(g, s);
        case SMR_C64: return launch_group_in<SMR_C64>(g, s);
        case SMR_I64: return launch_group_in<SMR_I64>(g, s);
    }
    return set_error(SMR_EINVAL, "bad compute class");
}

int ensure_tables(const GroupPlan& g) {
    std::lock_guard<std::mutex> lk(g.build_mu);
    const auto upload = [](void** dst, std::pair<const void*, size_t> t, const char* what) { return *dst ? SMR_OK : upload_table(dst, t.first, t.second, what); };
    if (int rc = upload(&g.d_members, g.member_table(), "group members")) return rc;
    if (int rc = upload(&g.d_first, GroupPlan::bytes_of(g.first_wg), "group workgroup ranges")) return rc;
    if (g.map.varc)
        if (int rc = upload(&g.map.d_consts, GroupPlan::bytes_of(g.map.consts), "group member scalars")) return rc;
    if (g.contract.varc)
        if (int rc = upload(&g.contract.d_consts, GroupPlan::bytes_of(g.contract.consts), "group member scalars")) return rc;
    if (g.contract.nsplit) {  // the split form's tables and the group's partials: one buffer per group, every element of which a run
                              // writes (main launch) before it reads it (fold): nothing an earlier run left there is ever read
        if (int rc = upload(&g.contract.d_split, GroupPlan::bytes_of(g.contract.split), "group slices")) return rc;
        if (int rc = upload(&g.contract.d_fold_first, GroupPlan::bytes_of(g.contract.fold_first), "group fold ranges")) return rc;
        if (!g.contract.d_partials) {
            const hipError_t e = hipMalloc(&g.contract.d_partials, g.contract.scratch_bytes);
            if (e != hipSuccess) return hip_error(e, "hipMalloc(group partials)");
        }
    }
    if (g.reduce.npartials) {  // a run of slots and an arrival counter for every member with more than one workgroup.  A run writes a
                               // slot before it reads it; the counters must be ZERO before the first launch (the workgroup that
                               // arrives last leaves its counter at zero for the next one)
        if (!g.reduce.d_partials) {
            const hipError_t e = hipMalloc(&g.reduce.d_partials, (size_t)g.reduce.slots * (size_t)dtype_size(g.c.ct));
            if (e != hipSuccess) return hip_error(e, "hipMalloc(group partials)");
        }
        if (!g.reduce.d_counters) {
            const std::vector<unsigned> zeros((size_t)g.reduce.npartials, 0u);
            if (int rc = upload(&g.reduce.d_counters, GroupPlan::bytes_of(zeros), "group arrival counters")) return rc;
        }
    }
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
    if (flags & ~(SMR_GROUP_INDEPENDENT | SMR_GROUP_MEMBER_SCALARS | SMR_GROUP_REDUCE | SMR_GROUP_CONTRACT_SCALARS | SMR_GROUP_REDUCE_PART)) return set_error(SMR_EINVAL, "smr_group_create: unknown flag");
    smr_group* h = new (std::nothrow) smr_group();
    if (!h) return set_error(SMR_ENOMEM, "out of host memory");
    if (int rc = plan_group(members, count, flags, h->plan)) {
        delete h;
        return rc;
    }
    h->stream = members[0].stream;
    *out = h;
    return SMR_OK;
}

int smr_group_prepare(smr_group* g) {
    if (!g) return set_error(SMR_EINVAL, "null group");
    if (int rc = ensure_device()) return rc;
    if (int rc = ensure_tables(g->plan)) return rc;
    jit_set_prepare(true);
    const int rc = launch_group(g->plan, (hipStream_t)g->stream);
    jit_set_prepare(false);
    return rc;
}

int smr_group_execute(smr_group* g, void* stream) {
    if (!g) return set_error(SMR_EINVAL, "null group");
    if (int rc = ensure_device()) return rc;
    if (int rc = ensure_tables(g->plan)) return rc;
    hipStream_t s = (hipStream_t)(stream ? stream : g->stream);
    // the launch goes through HIP: on a library-owned stream it is foreign work (what the library submitted directly completes first,
    // and the stream's next direct launch drains it)
    if (int rc = fence_for_foreign_work(s)) return rc;
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
            const int64_t v[4] = {p.form(i), p.first_wg[i], (int64_t)p.first_wg[i + 1] - (int64_t)p.first_wg[i], p.rank[i]};
            for (size_t j = 0; j < 4; ++j)
                if (4 * i + j < cap) out[4 * i + j] = v[j];
        }
    return (int64_t)(4 * n);
}

int64_t smr_group_lanes(const smr_group* g, int64_t* out, size_t cap) {
    if (!g || g->plan.kind != GROUP_REDUCE_PART) return 0;
    const std::vector<GroupReducePartMemberD>& ms = g->plan.reduce_part.members;
    if (out)
        for (size_t i = 0; i < ms.size() && i < cap; ++i) out[i] = (int64_t)1 << ms[i].trlog;
    return (int64_t)ms.size();
}

int64_t smr_group_split_layout(const smr_group* g, int64_t* out, size_t cap) {
    if (!g || !g->plan.contract.nsplit) return 0;
    const GroupContractPlan& cp = g->plan.contract;
    const size_t n = cp.split.size();
    if (out)
        for (size_t i = 0; i < n; ++i) {
            const int64_t v[4] = {cp.split[i].S, cp.split[i].cps, cp.fold_first[i], (int64_t)cp.fold_first[i + 1] - (int64_t)cp.fold_first[i]};
            for (size_t j = 0; j < 4; ++j)
                if (4 * i + j < cap) out[4 * i + j] = v[j];
        }
    return (int64_t)(4 * n);
}

int smr_group_destroy(smr_group* g) {
    if (!g) return SMR_OK;
    void* const tables[] = {g->plan.d_members, g->plan.d_first, g->plan.map.d_consts, g->plan.contract.d_split, g->plan.contract.d_fold_first, g->plan.contract.d_partials,
                            g->plan.contract.d_consts, g->plan.reduce.d_partials, g->plan.reduce.d_counters};
    if (std::any_of(std::begin(tables), std::end(tables), [](void* t) { return t != nullptr; })) {
        (void)eager_fence_if_active();
        (void)hipDeviceSynchronize();  // a queued launch may still read the tables
        for (void* t : tables)
            if (t) (void)hipFree(t);
        (void)hipGetLastError();
    }
    delete g;
    return SMR_OK;
}

}  // extern "C"
