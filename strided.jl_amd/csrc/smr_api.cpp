// smr_api.cpp -- the C ABI of libstrided_hip.so (include/strided_hip.h): error reporting,
// device/memory helpers, plan cache, execution dispatch, sharding.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "smr_dispatch.h"
#include "smr_group.h"
#include "smr_orbit_args.h"
#include "smr_tiled_args.h"

namespace smr {

static thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int hip_error(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? SMR_ENOMEM : (e == hipErrorNoDevice ? SMR_ENODEVICE : SMR_EHIP);
}

int upload_table(void** dst, const void* src, size_t bytes, const char* what) {
    void* dptr = nullptr;
    hipError_t e = hipMalloc(&dptr, bytes);
    if (e != hipSuccess) return hip_error(e, ("hipMalloc(" + std::string(what) + ")").c_str());
    e = hipMemcpy(dptr, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dptr);
        return hip_error(e, ("hipMemcpy(" + std::string(what) + ")").c_str());
    }
    *dst = dptr;
    return SMR_OK;
}

int cu_count() {
    static const int ncu = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        (void)hipGetLastError();
        return n;
    }();
    return ncu;
}

// ---- TILED / ORBIT: the arguments of one execution ---------------------------------------------------
// The pure builders (smr_plan_tiled_args.cpp, smr_plan_orbit_args.cpp) compute a form's arguments and tables from the plan; what is
// left lives here, next to upload_table: the plan's cache of built forms, the uploads, and the fields that change from call to call.
template <class A>
static bool cached_form(const Plan::FormCache& cached, A& a) {
    if (cached.args.size() != sizeof a) return false;
    std::memcpy(&a, cached.args.data(), sizeof a);
    return true;
}
template <class A>
static void cache_form(Plan::FormCache& cached, const A& a) {
    cached.args.resize(sizeof a);
    std::memcpy(cached.args.data(), &a, sizeof a);
}
template <class T>
static int upload_once(void** dst, const std::vector<T>& rows, const char* what) {
    return *dst ? SMR_OK : upload_table(dst, rows.data(), rows.size() * sizeof(T), what);
}

template <bool WIDE>
int tiled_launch_args(const Plan& plan, void* const* base, int esize, const TiledVariant& tv, bool wt_store, TiledLaunch<WIDE>& L) {
    const Canon& c = plan.c;
    const TilePlan& t = plan.tile;
    const Options& o = options();
    TiledArgs<WIDE>& a = L.a;
    L.lds = (size_t)t.nstaged * ((size_t)1 << t.tilelog) * esize;
    L.grid = t.ord.empty() ? (unsigned)t.grid : (unsigned)t.ord.size();
    L.pgrid = tv.pgrid;  // the persistent, software-pipelined form (tiled_variant)
    Plan::FormCache& cached = plan.tiled_cache[(WIDE ? 2 : 0) + (tv.V > 1 ? 1 : 0)];
    if (!cached_form(cached, a)) {
        TiledBuild<WIDE> b;
        if (int rc = build_tiled_args<WIDE>(plan, esize, tv, b)) return rc;
        a = b.a;
        if (!jit_dry_run()) {
            if (a.ordmode == 2)
                if (int rc = upload_once(&plan.tiled_order, t.ord, "tile order")) return rc;
            if (int rc = upload_once(&cached.tab, b.rows, "lane table")) return rc;
            a.ordtab = reinterpret_cast<const uint32_t*>(plan.tiled_order);
            a.lanetab = reinterpret_cast<const LaneRow<WIDE>*>(cached.tab);
            cache_form(cached, a);
        }
    }
    for (int k = 0; k < c.M; ++k) a.op[k].base = base[k];
    // non-temporal stores: measured faster or equal whenever a tile writes whole 128-byte lines (32^4 Float64
    // permutedims! 3.36 -> 2.76 us, 128^4 864 -> 818 us, never slower for a consumer kernel that follows);
    // partial lines must meet in L2 first, so short destination runs keep plain stores
    a.nts = (o.nt_store > 0) ? 1 : 0;
    if (o.nt_store < 0) {
        const i64 run = std::min<i64>(c.dims[0], (i64)1 << t.tlog[0]) * c.esize[0];
        a.nts = (c.strides[0][0] == 1 && run >= 128) ? 1 : 0;
    }
    // write-through stores (policy 2): forced, or a launch recorded for a sequence (its packet then needs no release fence).  Only the
    // one-shot vector form: there every store of the kernel is one of the vector stores below.
    if (wt_store && L.pgrid == 0 && (o.nt_store == 2 || want_self_release(plan))) a.nts = 2;
    return SMR_OK;
}
template int tiled_launch_args<false>(const Plan&, void* const*, int, const TiledVariant&, bool, TiledLaunch<false>&);
template int tiled_launch_args<true>(const Plan&, void* const*, int, const TiledVariant&, bool, TiledLaunch<true>&);

int orbit_launch_args(const Plan& plan, void* const* base, int esize, const OrbitVariant& v, bool wt_store, OrbitLaunch& L) {
    const OrbitPlan& o = plan.orbit;
    const Options& opt = options();
    OrbitArgs& a = L.a;
    Plan::FormCache& cached = v.pair ? plan.pair_cache : plan.orbit_cache[v.V > 1 ? 1 : 0];
    if (!cached_form(cached, a)) {
        OrbitBuild b;
        if (int rc = v.pair ? build_pair_args(plan, esize, b) : build_orbit_args(plan, esize, v, b)) return rc;
        a = b.a;
        if (!jit_dry_run()) {
            // the one-orbit form's origin rows serve both of its access widths; the PAIR form's work list is its own
            void** list = v.pair ? &cached.tab : &plan.orbit_list;
            if (int rc = upload_once(list, b.rows, v.pair ? "orbit pair table" : "orbit origins")) return rc;
            a.list = reinterpret_cast<const uint32_t*>(*list);
            cache_form(cached, a);
        }
    }
    a.src = (const char*)base[o.k0];
    a.dst = (char*)base[0];
    if (v.pair) {
        a.nts = opt.nt_store > 0 ? 1 : 0;  // (32- / 64-byte runs: partial lines meet in L2, plain stores -- as in the one-orbit form)
        L.block = 256;
        L.lds = 8 * ((size_t)esize << 8);
    } else {
        // automatic: only tiles that write whole 128-byte lines (symmetrise 4000^2: 40.2 -> 38.5 us); the 32-/64-byte
        // runs of the 4-D orbits rely on line partners meeting in L2 and get slower (4.8 -> 6.3 us at 32^4)
        a.nts = (opt.nt_store > 0 || (opt.nt_store < 0 && plan.c.strides[0][0] == 1 && (esize << o.lg[0]) >= 128)) ? 1 : 0;
        L.block = 1u << a.ntlog;
        L.lds = (size_t)v.ng * ((size_t)esize << o.tilelog);
    }
    // write-through stores: forced (nt_store = 2), or a launch recorded for a sequence that fits the caches several times over
    // (want_self_release): its packet then needs no release fence
    if (wt_store && (opt.nt_store == 2 || want_self_release(plan))) a.nts = 2;
    L.grid = (unsigned)a.nlist;
    if (v.pipe && !v.pair) {
        // as many workgroups as the machine holds at once, a multiple of 8 so that a workgroup stays on its XCD's run
        const unsigned cap = (unsigned)cu_count() * (unsigned)std::max<size_t>(1, (160 * 1024) / L.lds) / 8u * 8u;
        if (cap >= 8) L.grid = std::min<unsigned>(L.grid, cap);
        if (opt.orbit_wgs >= 8) L.grid = std::min<unsigned>(L.grid, (unsigned)opt.orbit_wgs / 8u * 8u);
    }
    return SMR_OK;
}

// ---- per-type dispatch ---------------------------------------------------------------------------
#define SMR_DISPATCH_CT(fn)                                                   \
    switch (plan.c.bitcopy ? SMR_F32 : plan.c.ct) {                           \
        case SMR_F32: return fn##_ct<SMR_F32>(plan, bases, s);                \
        case SMR_F64: return fn##_ct<SMR_F64>(plan, bases, s);                \
        case SMR_C32: return fn##_ct<SMR_C32>(plan, bases, s);                \
        case SMR_C64: return fn##_ct<SMR_C64>(plan, bases, s);                \
        case SMR_I64: return fn##_ct<SMR_I64>(plan, bases, s);                \
    }                                                                         \
    return set_error(SMR_EINVAL, "bad compute class");

int launch_generic_map(const Plan& plan, void* const* bases, hipStream_t s) { SMR_DISPATCH_CT(launch_generic_map) }
int launch_stream_map(const Plan& plan, void* const* bases, hipStream_t s) { SMR_DISPATCH_CT(launch_stream_map) }
int launch_tiled_map(const Plan& plan, void* const* bases, hipStream_t s) { SMR_DISPATCH_CT(launch_tiled_map) }
int launch_reduce_all(const Plan& plan, void* const* bases, hipStream_t s) { SMR_DISPATCH_CT(launch_reduce_all) }
int launch_reduce_part(const Plan& plan, void* const* bases, hipStream_t s) { SMR_DISPATCH_CT(launch_reduce_part) }
int launch_orbit_map(const Plan& plan, void* const* bases, hipStream_t s) { SMR_DISPATCH_CT(launch_orbit_map) }
int launch_flat_map(const Plan& plan, void* const* bases, hipStream_t s) { SMR_DISPATCH_CT(launch_flat_map) }
int launch_contract(const Plan& plan, void* const* bases, hipStream_t s) { SMR_DISPATCH_CT(launch_contract) }

// ---- overlap windows and library-owned streams --------------------------------------------------------------------------
// smr_overlap_begin / _end nest per stream.  HIP ignores the any-order dispatch flag on gfx9 (profiles/r04_overlap.txt), so a window
// does not change how launches that go through HIP are ordered.  Independent launches overlap where the library dispatches itself:
// library-owned streams (smr_stream_create, registered here for good) and recorded sequences (smr_seq.cpp).
namespace {
struct Span {
    uintptr_t lo, hi;
};
struct Window {
    int depth = 0;       // nesting of smr_overlap_begin
    bool owned = false;  // smr_stream_create: permanently registered
};
struct Windows {
    std::mutex mu;
    std::unordered_map<void*, Window> map;
};
Windows& windows() {
    static Windows* w = new Windows();
    return *w;
}

// byte ranges one execution of `plan` reads and writes (every operand's bounding range; the plan's own partials)
void footprint(const Plan& plan, void* const* bases, std::vector<Span>& rd, std::vector<Span>& wr) {
    const Canon& c = plan.c;
    for (int k = 0; k < c.M; ++k) {
        Span sp;
        operand_span(c, k, bases ? bases[c.orig[k]] : c.base[k], sp.lo, sp.hi);
        if (k == 0) {
            wr.push_back(sp);
            if (c.redop != SMR_RED_NONE) rd.push_back(sp);  // reductions accumulate into the destination
        } else {
            rd.push_back(sp);
        }
    }
    if (plan.scratch) {
        const Span sp{(uintptr_t)plan.scratch, (uintptr_t)plan.scratch + plan.counter_off + RED_COUNTERS * sizeof(unsigned)};
        wr.push_back(sp);
        rd.push_back(sp);
    }
}

bool stream_is_owned(hipStream_t s) {
    Windows& W = windows();
    std::lock_guard<std::mutex> g(W.mu);
    if (W.map.empty()) return false;
    auto it = W.map.find((void*)s);
    return it != W.map.end() && it->second.owned;
}

// on a library-owned stream, what the library submitted directly completes before whatever follows on the stream through HIP ...
int window_fence(hipStream_t s) {
    if (!stream_is_owned(s) || !eager_available(s)) return SMR_OK;
    const int rc = eager_fence_all();
    eager_note_hip_work(s);  // ... and that HIP work completes before the next direct launch ON THIS STREAM
    return rc;
}
}  // namespace

// for the other translation units (smr_comm.cpp: the RCCL collective is foreign work on the stream)
int fence_for_foreign_work(hipStream_t s) { return window_fence(s); }

static std::atomic<long> g_launches{0};
void count_launch() { g_launches.fetch_add(1, std::memory_order_relaxed); }

static int execute_family(const Plan& plan, void* const* bases, hipStream_t s);

static int execute(const Plan& plan, void* const* bases, hipStream_t s) {
    if (!jit_no_launch() && !recorder()) {
        // a library-owned stream: the library submits the launch itself (smr_eager.cpp: eager direct dispatch), on the hardware queue its
        // data dependencies select -- independent executions run concurrently, host cost ~1 us instead of HIP's 3.6-4 us
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (options().eager_direct && stream_is_owned(s) && eager_available(s) &&
            (hipStreamIsCapturing(s, &capturing) != hipSuccess || capturing == hipStreamCaptureStatusNone)) {  // (a capture records HIP launches)
            std::vector<Span> rd, wr;
            footprint(plan, bases, rd, wr);
            std::vector<RecLaunch> rec;
            // self-released launches (write-through stores, no release fence on the packet: smr_seq.cpp) while what this stream has
            // been writing lately fits the caches
            set_recorder(&rec, options().eager_self_release != 0 && !wr.empty() && eager_recent_writes_fit(wr[0].lo, wr[0].hi), true);
            int rc = execute_family(plan, bases, s);
            set_recorder(nullptr);
            if (rc) return rc;
            if (!__atomic_exchange_n(&plan.eager_seen, true, __ATOMIC_RELAXED)) eager_request_sys_acquire(s);  // (two threads may execute one plan)
            std::vector<std::pair<uintptr_t, uintptr_t>> r2, w2;
            for (const Span& x : rd) r2.emplace_back(x.lo, x.hi);
            for (const Span& x : wr) w2.emplace_back(x.lo, x.hi);
            rc = rec.empty() ? SMR_EUNSUPPORTED : eager_submit(plan, rec, r2, w2, s);
            if (rc != SMR_EUNSUPPORTED) return rc;
            // this execution goes through HIP (a kernel that needs scratch memory, ...): everything submitted directly comes first
            if (int rc3 = eager_fence_all()) return rc3;
            eager_note_hip_work(s);
        }
    }
    return execute_family(plan, bases, s);
}

static int execute_family(const Plan& plan, void* const* bases, hipStream_t s) {
    switch (plan.family) {
        case FAM_GENERIC: return launch_generic_map(plan, bases, s);
        case FAM_STREAM: return launch_stream_map(plan, bases, s);
        case FAM_TILED: {
            std::lock_guard<std::mutex> g(*plan.build_mu);
            return launch_tiled_map(plan, bases, s);
        }
        case FAM_ORBIT: {
            std::lock_guard<std::mutex> g(*plan.build_mu);
            return launch_orbit_map(plan, bases, s);
        }
        case FAM_FLAT: return launch_flat_map(plan, bases, s);
        case FAM_REDUCE_ALL: return launch_reduce_all(plan, bases, s);
        case FAM_REDUCE_PART: return launch_reduce_part(plan, bases, s);
        case FAM_CONTRACT: return launch_contract(plan, bases, s);
    }
    return set_error(SMR_EINVAL, "plan has no kernel family");
}

unsigned long long* stamp_next(size_t waves) {
    Options& o = options();
    if (!o.stamp_base || o.stamp_used + (i64)(2 * waves) > o.stamp_cap) return nullptr;
    unsigned long long* p = reinterpret_cast<unsigned long long*>((uintptr_t)o.stamp_base) + o.stamp_used;
    o.stamp_used += (i64)(2 * waves);
    return p;
}

static bool g_device_checked = false;
int ensure_device() {
    if (g_device_checked) return SMR_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return set_error(SMR_ENODEVICE, "libstrided_hip: no HIP device available (the HIP kernels are the only compute path; there is no CPU fallback)");
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
            if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
                return set_error(SMR_ENODEVICE, std::string("libstrided_hip is built for gfx950 only, found ") + prop.gcnArchName);
        }
    }
    g_device_checked = true;
    return SMR_OK;
}

}  // namespace smr

using namespace smr;

struct smr_plan {
    Plan plan;
    int nops = 0;  // M of the originating problem (length of a `bases` rebinding array)
    void* stream = nullptr;
    void* obase[SMR_MAXM] = {nullptr};  // the base pointers the plan was created with (aliasing pattern)
    // plans with reduction scratch (partials + arrival counters) must not run twice at once: executions on different streams are
    // chained through an event
    std::mutex scratch_mu;
    bool ran = false;
    hipStream_t last_stream = nullptr;
    hipEvent_t order_ev = nullptr;
};

// Executes a plan that may own reduction scratch.  The one-launch fold (smr_k_reduce.hip: arrive_last) relies on the arrival
// counters being zero when a launch starts and on the partials belonging to ONE execution at a time:
//   * an execution on another stream than the previous one first waits (on the device) for that one -- two streams never run
//     the same plan's launches concurrently (skipped while either stream is being captured: a capture cannot wait for foreign work;
//     captured graphs replay in the order their streams impose);
//   * an execution that failed to launch leaves nothing half-done on the device, but the counters are re-zeroed on the stream all the
//     same, so that no earlier, aborted launch can leave a later one waiting for arrivals that never come.
static int execute_owned(smr_plan* h, void* const* bases, hipStream_t s) {
    if (!h->plan.scratch || jit_no_launch() || recorder()) return execute(h->plan, bases, s);
    std::lock_guard<std::mutex> g(h->scratch_mu);
    if (h->ran && h->last_stream != s) {
        hipStreamCaptureStatus c1 = hipStreamCaptureStatusNone, c2 = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &c1);
        (void)hipStreamIsCapturing(h->last_stream, &c2);
        // launches the library submitted itself (a library-owned stream) are not HIP work: no event covers them, and the direct queues do
        // not honour hipStreamWaitEvent.  With such a stream on either side the previous execution is waited for on the host.
        if (c1 == hipStreamCaptureStatusNone && c2 == hipStreamCaptureStatusNone && (stream_is_owned(s) || stream_is_owned(h->last_stream))) {
            (void)eager_fence_if_active();
            (void)hipStreamSynchronize(h->last_stream);
        }
        if (c1 == hipStreamCaptureStatusNone && c2 == hipStreamCaptureStatusNone) {
            if (!h->order_ev) (void)hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming);
            if (h->order_ev && hipEventRecord(h->order_ev, h->last_stream) == hipSuccess) (void)hipStreamWaitEvent(s, h->order_ev, 0);
        }
        (void)hipGetLastError();
    }
    const int rc = execute(h->plan, bases, s);
    h->ran = true;
    h->last_stream = s;
    if (rc != SMR_OK) {
        (void)hipGetLastError();
        (void)hipMemsetAsync((char*)h->plan.scratch + h->plan.counter_off, 0, RED_COUNTERS * sizeof(unsigned), s);
        (void)hipGetLastError();
    }
    return rc;
}

static int plan_build(const smr_problem* p, smr_plan** out) {
    if (!p || !out) return set_error(SMR_EINVAL, "null argument");
    smr_plan* h = new (std::nothrow) smr_plan();
    if (!h) return set_error(SMR_ENOMEM, "out of host memory");
    int rc = make_plan(p, h->plan);
    if (rc) {
        delete h;
        return rc;
    }
    h->nops = p->M;
    h->stream = p->stream;
    for (int k = 0; k < p->M; ++k) h->obase[k] = p->ops[k].base;
    *out = h;
    return SMR_OK;
}

// reduction partials are allocated on first execution (planning itself needs no device)
static int ensure_scratch(smr_plan* h) {
    std::lock_guard<std::mutex> g(*h->plan.build_mu);
    const size_t need = h->plan.family == FAM_CONTRACT ? h->plan.contract.scratch_bytes : h->plan.red.scratch_bytes;  // (at most one of the two)
    if (h->plan.scratch || need == 0) return SMR_OK;
    const size_t coff = (need + 255) & ~(size_t)255;
    void* buf = nullptr;
    hipError_t e = hipMalloc(&buf, coff + RED_COUNTERS * sizeof(unsigned));
    if (e != hipSuccess) return hip_error(e, "hipMalloc(reduction partials)");
    e = hipMemset((char*)buf + coff, 0, RED_COUNTERS * sizeof(unsigned));  // the kernels leave the counters at zero
    if (e != hipSuccess) {
        (void)hipFree(buf);
        return hip_error(e, "hipMemset(reduction counters)");
    }
    h->plan.counter_off = coff;
    h->plan.scratch = buf;
    return SMR_OK;
}

static void plan_free(smr_plan* h) {
    if (!h) return;
    (void)eager_fence_if_active();  // launches submitted directly may still read the plan's tables
    if (h->plan.scratch) (void)hipFree(h->plan.scratch);
    for (void** p : h->plan.dev_tables())
        if (*p) {
            (void)hipFree(*p);
            *p = nullptr;
        }
    if (h->order_ev) (void)hipEventDestroy(h->order_ev);
    delete h;
}

// ---- hooks for smr_seq.cpp, declared in smr_direct.h (the smr_plan struct is private to this file) --------------------------------------
namespace smr {
int seq_execute_plan(smr_plan* plan, void* const* bases, hipStream_t s, bool prepare_only) {
    if (prepare_only) return smr_plan_prepare(plan);
    return smr_plan_execute(plan, bases, (void*)s);
}
void seq_footprint(smr_plan* plan, void* const* bases, std::vector<std::pair<uintptr_t, uintptr_t>>& rd, std::vector<std::pair<uintptr_t, uintptr_t>>& wr) {
    std::vector<Span> r, w;
    footprint(plan->plan, bases, r, w);
    for (const Span& x : r) rd.emplace_back(x.lo, x.hi);
    for (const Span& x : w) wr.emplace_back(x.lo, x.hi);
}
int seq_nops(smr_plan* plan) { return plan->nops; }
bool seq_stream_is_owned(hipStream_t s) { return stream_is_owned(s); }
}  // namespace smr

// ---- plan cache for the one-shot entry point ---------------------------------------------------------
// Plans are held by shared_ptr: a thread that found a plan keeps it alive while it executes, eviction only
// drops the cache's reference (the last owner frees the device tables -- after draining the plan's stream,
// outside the cache lock).  The key describes the problem's SHAPE, not its addresses: operands are
// identified by alias class (which operands share a base pointer) and 256-byte alignment, and the
// actual base pointers are bound at launch -- a loop over freshly allocated arrays hits one entry.
namespace {
struct PlanDeleter {
    void operator()(smr_plan* h) const {
        if (!h) return;
        const auto tabs = h->plan.dev_tables();
        if (h->plan.scratch || std::any_of(tabs.begin(), tabs.end(), [](void** p) { return *p != nullptr; })) {
            (void)window_fence((hipStream_t)h->stream);
            (void)hipStreamSynchronize((hipStream_t)h->stream);  // queued kernels may still read the tables
        }
        plan_free(h);
    }
};
typedef std::shared_ptr<smr_plan> PlanRef;

struct Cache {
    std::mutex mu;
    std::list<std::pair<std::string, PlanRef>> lru;
    std::unordered_map<std::string, std::list<std::pair<std::string, PlanRef>>::iterator> map;
    static constexpr size_t CAP = 512;
    ~Cache() {}
};
Cache& cache() {
    static Cache* c = new Cache();  // intentionally leaked: no HIP calls at process exit
    return *c;
}

std::string signature(const smr_problem* p) {
    std::string s;
    auto put = [&](const void* d, size_t n) { s.append((const char*)d, n); };
    put(&p->N, sizeof p->N);
    put(&p->M, sizeof p->M);
    put(p->dims, sizeof(int64_t) * (size_t)p->N);
    for (int k = 0; k < p->M; ++k) {
        // alias class = first operand with the same base; byte distance to it (views of one buffer may sit
        // at different offsets); alignment of the base itself
        int32_t cls = k;
        for (int j = 0; j < k; ++j)
            if (p->ops[j].base == p->ops[k].base) {
                cls = j;
                break;
            }
        const uint32_t align = (uint32_t)((uintptr_t)p->ops[k].base & 255u);
        // address class = first operand whose FIRST ELEMENT sits at the same address: the ORBIT / tile-order planners
        // recognise "views of one buffer" by that address, whatever the base pointers are
        int32_t acls = k;
        const char* ak = (const char*)p->ops[k].base + p->ops[k].offset * (int64_t)dtype_size(p->ops[k].dtype);
        for (int j = 0; j < k; ++j)
            if ((const char*)p->ops[j].base + p->ops[j].offset * (int64_t)dtype_size(p->ops[j].dtype) == ak) {
                acls = j;
                break;
            }
        put(&acls, sizeof acls);
        put(&cls, sizeof cls);
        put(&align, sizeof align);
        put(&p->ops[k].offset, sizeof(int64_t));
        put(p->ops[k].strides, sizeof(int64_t) * (size_t)p->N);
        put(&p->ops[k].dtype, sizeof(int32_t));
        put(&p->ops[k].conj, sizeof(int32_t));
    }
    put(&p->fprog_len, sizeof(int32_t));
    if (p->fprog && p->fprog_len > 0) put(p->fprog, (size_t)(2 * p->fprog_len));
    put(&p->nconsts, sizeof(int32_t));
    if (p->fconsts && p->nconsts > 0) put(p->fconsts, sizeof(double) * (size_t)(2 * p->nconsts));
    put(&p->redop, sizeof(int32_t));
    put(&p->initop, sizeof(int32_t));
    put(p->initarg, sizeof p->initarg);
    put(&p->stream, sizeof(void*));
    return s;
}

void cache_clear_locked(Cache& c, std::vector<PlanRef>& dropped) {
    for (auto& kv : c.lru) dropped.push_back(std::move(kv.second));
    c.lru.clear();
    c.map.clear();
}

// ---- options (smr_set_option / smr_get_option; include/strided_hip.h describes them) -------------------------------------
// Every option that plans depend on, by family.  The stamp buffer, tile_lg0..7 and the read-only counters are handled
// by name in the two functions.
struct OptionField {
    const char* name;
    i64 Options::*field;
};
const OptionField OPTION_FIELDS[] = {
    {"force_family", &Options::force_family},
    {"jit", &Options::jit},
    {"max_lds_bytes", &Options::max_lds_bytes},
    // TILED
    {"tile_log2", &Options::tile_log2},
    {"tile_order", &Options::tile_order},
    {"tile_block", &Options::tile_block},
    {"tile_block_xcd", &Options::tile_block_xcd},
    {"tiled_vec", &Options::tiled_vec},
    {"tiled_uavec", &Options::tiled_uavec},
    {"tiled_edge_first", &Options::tiled_edge_first},
    {"tiled_persist", &Options::tiled_persist},
    {"tiled_persist_wpc", &Options::tiled_persist_wpc},
    {"tiled_persist_min", &Options::tiled_persist_min},
    {"tiled_xpose", &Options::tiled_xpose},
    {"tiled_gorder", &Options::tiled_gorder},
    // ORBIT
    {"orbit", &Options::orbit},
    {"orbit_lg", &Options::orbit_lg},
    {"orbit_min", &Options::orbit_min},
    {"orbit_few", &Options::orbit_few},
    {"orbit_minrun", &Options::orbit_minrun},
    {"orbit_group", &Options::orbit_group},
    {"orbit_pipe", &Options::orbit_pipe},
    {"orbit_wgs", &Options::orbit_wgs},
    {"orbit_pair", &Options::orbit_pair},
    {"orbit_pack", &Options::orbit_pack},
    // FLAT
    {"flat", &Options::flat},
    {"flat_wide", &Options::flat_wide},
    {"flat2", &Options::flat2},
    {"contract", &Options::contract},
    {"contract_split", &Options::contract_split},
    {"contract_tile", &Options::contract_tile},
    {"flat2_pair", &Options::flat2_pair},
    {"flat2_bytes", &Options::flat2_bytes},
    {"flat2_lead_bytes", &Options::flat2_lead_bytes},
    {"flat2_long", &Options::flat2_long},
    {"flatb", &Options::flatb},
    // STREAM
    {"stream_ua", &Options::stream_ua},
    {"stream_pack_rows", &Options::stream_pack_rows},
    {"nt_store", &Options::nt_store},
    {"nt_stream_min", &Options::nt_stream_min},
    // reductions
    {"reduce_blocks", &Options::reduce_blocks},
    {"reduce_part_wgs", &Options::reduce_part_wgs},
    {"reduce_part_kind", &Options::reduce_part_kind},
    {"reduce_single", &Options::reduce_single},
    {"reduce_row_floor", &Options::reduce_row_floor},
    {"reduce_row_dense", &Options::reduce_row_dense},
    {"reduce_col_txlog", &Options::reduce_col_txlog},
    {"reduce_col_exact", &Options::reduce_col_exact},
    {"reduce_col_narrow", &Options::reduce_col_narrow},
    {"nt_load", &Options::nt_load},
    // dispatch on library-owned streams and in sequences
    {"eager_direct", &Options::eager_direct},
    {"eager_self_release", &Options::eager_self_release},
    {"seq_self_release", &Options::seq_self_release},
    {"self_release_max_bytes", &Options::self_release_max_bytes},
    {"self_release_max_total", &Options::self_release_max_total},
    // sharding
    {"allreduce_f64", &Options::allreduce_f64},
};

i64 Options::*option_field(const std::string& n) {
    for (const OptionField& f : OPTION_FIELDS)
        if (n == f.name) return f.field;
    return nullptr;
}

// "tile_lg0" .. "tile_lg7": the canonical dim, else -1
int tile_lg_dim(const std::string& n) {
    return n.size() == 8 && n.rfind("tile_lg", 0) == 0 && n[7] >= '0' && n[7] <= '7' ? n[7] - '0' : -1;
}
}  // namespace

extern "C" {

int smr_abi_version(void) { return SMR_ABI_VERSION; }

const char* smr_last_error(void) { return g_last_error.c_str(); }

int smr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int smr_init(int device) {
    int n = smr_device_count();
    if (n <= 0) return set_error(SMR_ENODEVICE, "smr_init: no HIP device");
    if (device < 0 || device >= n) return set_error(SMR_EINVAL, "smr_init: device index out of range");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_error(e, "hipSetDevice");
    g_device_checked = false;
    return ensure_device();
}

int smr_shutdown(void) {
    Cache& c = cache();
    std::vector<PlanRef> dropped;
    {
        std::lock_guard<std::mutex> g(c.mu);
        cache_clear_locked(c, dropped);
    }
    dropped.clear();  // frees outside the lock
    return SMR_OK;
}

int smr_malloc(size_t bytes, void** out) {
    if (!out) return set_error(SMR_EINVAL, "null out");
    int rc = ensure_device();
    if (rc) return rc;
    hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    return e == hipSuccess ? SMR_OK : hip_error(e, "hipMalloc");
}
int smr_free(void* p) {
    const int rc = eager_fence_if_active();  // hipFree waits for HIP's queues only
    hipError_t e = hipFree(p);
    if (e != hipSuccess) return hip_error(e, "hipFree");
    return rc;
}
int smr_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
    if (int rc = window_fence((hipStream_t)stream)) return rc;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    return e == hipSuccess ? SMR_OK : hip_error(e, "hipMemcpyAsync(h2d)");
}
int smr_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
    if (int rc = window_fence((hipStream_t)stream)) return rc;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream);
    return e == hipSuccess ? SMR_OK : hip_error(e, "hipMemcpyAsync(d2h)");
}
int smr_stream_sync(void* stream) {
    int rc = window_fence((hipStream_t)stream);
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? SMR_OK : hip_error(e, "hipStreamSynchronize");
}

int smr_overlap_begin(void* stream) {
    int rc = ensure_device();
    if (rc) return rc;
    Windows& W = windows();
    std::lock_guard<std::mutex> g(W.mu);
    ++W.map[stream].depth;
    return SMR_OK;
}

int smr_overlap_end(void* stream) {
    Windows& W = windows();
    std::lock_guard<std::mutex> g(W.mu);
    auto it = W.map.find(stream);
    if (it == W.map.end() || it->second.depth == 0) return set_error(SMR_EINVAL, "smr_overlap_end without smr_overlap_begin on this stream");
    if (--it->second.depth == 0 && !it->second.owned) W.map.erase(it);
    return SMR_OK;
}

int smr_overlap_fence(void* stream) { return window_fence((hipStream_t)stream); }

int smr_stream_create(void** out) {
    if (!out) return set_error(SMR_EINVAL, "null out");
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_error(e, "hipStreamCreateWithFlags");
    Windows& W = windows();
    std::lock_guard<std::mutex> g(W.mu);
    W.map[(void*)s].owned = true;
    *out = (void*)s;
    return SMR_OK;
}

int smr_stream_destroy(void* stream) {
    if (!stream) return set_error(SMR_EINVAL, "null stream");
    {
        Windows& W = windows();
        std::lock_guard<std::mutex> g(W.mu);
        auto it = W.map.find(stream);
        if (it == W.map.end() || !it->second.owned) return set_error(SMR_EINVAL, "smr_stream_destroy: not a stream made by smr_stream_create");
        W.map.erase(it);
    }
    (void)eager_fence_if_active();
    eager_forget_stream((hipStream_t)stream);
    {   // cached one-shot plans remember the stream they were created on and drain it when they are dropped: none may outlive this one
        // (round 4: a later smr_set_option -- which clears the cache -- synchronised a destroyed stream and crashed)
        Cache& c = cache();
        std::vector<PlanRef> dropped;
        {
            std::lock_guard<std::mutex> g(c.mu);
            cache_clear_locked(c, dropped);
        }
        dropped.clear();
    }
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamDestroy((hipStream_t)stream);
    return e == hipSuccess ? SMR_OK : hip_error(e, "hipStreamDestroy");
}

int smr_plan_create(const smr_problem* problem, smr_plan** out) {
    // planning is pure host arithmetic; the device is only required to execute (or to
    // allocate reduction scratch)
    return plan_build(problem, out);
}

int smr_plan_execute(smr_plan* plan, void* const* bases, void* stream) {
    if (!plan) return set_error(SMR_EINVAL, "null plan");
    if (bases) {
        // the planner merged operands that were the same view of one buffer and co-located views that shared a
        // buffer: a rebinding must keep exactly that aliasing pattern
        for (int k = 0; k < plan->nops; ++k)
            for (int j = 0; j < k; ++j)
                if ((plan->obase[j] == plan->obase[k]) != (bases[j] == bases[k]))
                    return set_error(SMR_EINVAL, "smr_plan_execute: the rebound base pointers change which operands share a buffer; create a new plan");
    }
    int rc = ensure_device();
    if (rc) return rc;
    rc = ensure_scratch(plan);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)(stream ? stream : plan->stream);
    return execute_owned(plan, bases, s);
}

int smr_plan_prepare(smr_plan* plan) {
    if (!plan) return set_error(SMR_EINVAL, "null plan");
    int rc = ensure_device();
    if (rc) return rc;
    rc = ensure_scratch(plan);
    if (rc) return rc;
    jit_set_prepare(true);
    rc = execute(plan->plan, nullptr, (hipStream_t)plan->stream);
    jit_set_prepare(false);
    return rc;
}

int smr_plan_destroy(smr_plan* plan) {
    plan_free(plan);
    return SMR_OK;
}

int smr_plan_describe(const smr_plan* plan, char* buf, size_t buflen) {
    if (!plan || !buf || buflen == 0) return set_error(SMR_EINVAL, "null argument");
    std::snprintf(buf, buflen, "%s", plan->plan.desc.c_str());
    return SMR_OK;
}

// the f-program the kernels will run, after canonicalisation (host-only: no device, no launch)
int smr_debug_canon_prog(const smr_problem* problem, uint8_t* code, int cap, int* nwraps, int* compute_class, int32_t* orig) {
    Canon c;
    const int rc = canonicalise(problem, c);
    if (rc) return rc;
    if (nwraps) *nwraps = c.int_wraps;
    if (compute_class) *compute_class = c.bitcopy ? -1 : c.ct;
    if (orig)
        for (int j = 0; j < SMR_MAXM; ++j) orig[j] = j < c.M ? c.orig[j] : -1;
    if (code)
        for (int i = 0; i < 2 * c.prog.len && i < cap; ++i) code[i] = c.prog.code[i];
    return c.prog.len;
}

int64_t smr_plan_algorithmic_bytes(const smr_plan* plan) { return plan ? plan->plan.c.algbytes : 0; }

int smr_mapreduce_scalar(const smr_problem* problem, void* host_result) {
    if (!problem || !host_result) return set_error(SMR_EINVAL, "null argument");
    if (problem->N < 1 || problem->N > SMR_MAXN) return set_error(SMR_EINVAL, "rank out of range");
    for (int i = 0; i < problem->N; ++i)
        if (problem->dims[i] != 1 && problem->ops[0].strides[i] != 0)
            return set_error(SMR_EINVAL, "smr_mapreduce_scalar: the destination must be a single element");
    int rc = smr_mapreduce(problem);
    if (rc) return rc;
    const smr_operand& d = problem->ops[0];
    const size_t es = (size_t)dtype_size(d.dtype);
    rc = window_fence((hipStream_t)problem->stream);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(host_result, (const char*)d.base + d.offset * (int64_t)es, es, hipMemcpyDeviceToHost,
                                  (hipStream_t)problem->stream);
    if (e != hipSuccess) return hip_error(e, "hipMemcpyAsync(scalar result)");
    e = hipStreamSynchronize((hipStream_t)problem->stream);
    return e == hipSuccess ? SMR_OK : hip_error(e, "hipStreamSynchronize");
}

int smr_plan_jit_compile(smr_plan* plan, size_t* code_size) {
    if (!plan) return set_error(SMR_EINVAL, "null plan");
    if (code_size) *code_size = 0;
    if (plan->plan.c.bitcopy) return SMR_OK;
    jit_set_dry_run(true);
    const int rc = execute(plan->plan, nullptr, nullptr);
    const size_t n = jit_dry_code_size();
    jit_set_dry_run(false);
    if (rc == SMR_OK && code_size) *code_size = n;
    return rc;
}

int smr_plan_jit_source(const smr_plan* plan, char* buf, size_t buflen) {
    if (!plan || !buf || buflen == 0) return set_error(SMR_EINVAL, "null argument");
    static const char* names[] = {"float", "double", "smr::c32", "smr::c64"};
    const Canon& c = plan->plan.c;
    std::snprintf(buf, buflen, "%s", jit_functor_source(c, c.ct == SMR_I64 ? "smr::ix64" : names[c.ct & 3]).c_str());
    return SMR_OK;
}

int64_t smr_plan_tile_order(const smr_plan* plan, uint32_t* out, size_t cap) {
    if (!plan || (plan->plan.family != FAM_TILED && plan->plan.family != FAM_ORBIT)) return 0;
    const std::vector<uint32_t>& ord = plan->plan.family == FAM_ORBIT ? plan->plan.orbit.wtile : plan->plan.tile.ord;
    if (out)
        for (size_t i = 0; i < ord.size() && i < cap; ++i) out[i] = ord[i];
    return (int64_t)ord.size();
}

int64_t smr_plan_orbit_pairs(const smr_plan* plan, uint32_t* out, size_t cap) {
    if (!plan || plan->plan.family != FAM_ORBIT || !plan->plan.orbit.pair_ok) return 0;
    const std::vector<uint32_t>& pt = plan->plan.orbit.ptile;
    if (out)
        for (size_t i = 0; i < pt.size() && i < cap; ++i) out[i] = pt[i];
    return (int64_t)pt.size();
}

int64_t smr_plan_flat_runs(const smr_plan* plan, int64_t* out, size_t cap) {
    if (!plan || plan->plan.family != FAM_FLAT || !plan->plan.flat2.on || plan->plan.flatb.on) return 0;
    const Canon& c = plan->plan.c;
    const Flat2Plan& f = plan->plan.flat2;
    std::vector<int64_t> v = {f.kt, f.shared ? 1 : 0, c.N, f.R[0], f.R[1], f.TP[0], f.TP[1], f.p[0], f.p[1]};
    for (int d = 0; d < c.N; ++d) v.push_back(c.dims[d]);
    for (int d = 0; d < c.N; ++d) v.push_back(c.strides[0][d]);
    for (int d = 0; d < c.N; ++d) v.push_back(c.strides[f.kt][d]);
    for (int s = 0; s < 2; ++s)
        for (int d = 0; d < c.N; ++d) v.push_back(f.ingroup[s][d] ? 1 : 0);
    for (int s = 0; s < 2; ++s)
        for (int r = 0; r < f.R[s]; ++r) v.push_back(f.roff[s][r]);
    if (out)
        for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
    return (int64_t)v.size();
}

int64_t smr_plan_flat_side(const smr_plan* plan, int64_t* out, size_t cap) {
    if (!plan || plan->plan.family != FAM_FLAT || plan->plan.flat2.on || plan->plan.flatb.on) return 0;
    const Canon& c = plan->plan.c;
    const FlatPlan& f = plan->plan.flat;
    std::vector<int64_t> v = {f.dir, f.R, f.tplog, f.tqlog, f.p, f.q, f.lshare ? 1 : 0, f.fuse ? 1 : 0, f.kt, c.N};
    for (int d = 0; d < c.N; ++d) v.push_back(c.dims[d]);
    for (int d = 0; d < c.N; ++d) v.push_back(c.strides[0][d]);
    for (int d = 0; d < c.N; ++d) v.push_back(c.strides[f.kt][d]);
    for (int d = 0; d < c.N; ++d) v.push_back(f.ingroup[d] ? 1 : 0);
    for (int r = 0; r < f.R; ++r) v.push_back(f.roff[r]);
    if (out)
        for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
    return (int64_t)v.size();
}

int64_t smr_plan_flat_batched(const smr_plan* plan, int64_t* out, size_t cap) {
    if (!plan || plan->plan.family != FAM_FLAT || !plan->plan.flatb.on) return 0;
    const Canon& c = plan->plan.c;
    const FlatBPlan& f = plan->plan.flatb;
    std::vector<int64_t> v = {f.g, f.P, f.K, c.N};
    for (int d = 0; d < c.N; ++d) v.push_back(c.dims[d]);
    for (int d = 0; d < c.N; ++d) v.push_back(c.strides[0][d]);
    for (int d = 0; d < c.N; ++d) v.push_back(c.strides[1][d]);
    for (int r = 0; r < f.P; ++r) v.push_back(f.srcoff[r]);
    if (out)
        for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
    return (int64_t)v.size();
}

int smr_mapreduce(const smr_problem* problem) {
    if (!problem) return set_error(SMR_EINVAL, "null problem");
    if (problem->N < 1 || problem->N > SMR_MAXN || problem->M < 1 || problem->M > SMR_MAXM)
        return set_error(SMR_EINVAL, "rank / operand count out of range");
    int rc = ensure_device();
    if (rc) return rc;
    Cache& c = cache();
    std::string key = signature(problem);
    PlanRef h, evicted;
    {
        std::lock_guard<std::mutex> g(c.mu);
        auto it = c.map.find(key);
        if (it != c.map.end()) {
            c.lru.splice(c.lru.begin(), c.lru, it->second);
            h = it->second->second;
        }
    }
    if (!h) {
        smr_plan* raw = nullptr;
        rc = plan_build(problem, &raw);
        if (rc) return rc;
        PlanRef fresh(raw, PlanDeleter());
        std::lock_guard<std::mutex> g(c.mu);
        auto it = c.map.find(key);  // another thread may have inserted the same key meanwhile: use its plan
        if (it != c.map.end()) {
            c.lru.splice(c.lru.begin(), c.lru, it->second);
            h = it->second->second;
        } else {
            c.lru.emplace_front(key, fresh);
            c.map[key] = c.lru.begin();
            h = fresh;
            if (c.lru.size() > Cache::CAP) {
                evicted = std::move(c.lru.back().second);  // released after the lock is gone
                c.map.erase(c.lru.back().first);
                c.lru.pop_back();
            }
        }
    }
    evicted.reset();
    rc = ensure_scratch(h.get());
    if (rc) return rc;
    // the plan was built for another set of base pointers with the same aliasing / alignment: bind the
    // caller's at launch
    void* bases[SMR_MAXM];
    for (int k = 0; k < problem->M; ++k) bases[k] = problem->ops[k].base;
    return execute_owned(h.get(), bases, (hipStream_t)problem->stream);
}

int smr_shard(const smr_problem* p, int nshards, int shard, smr_problem* out, int* needs_allreduce) {
    return smr_shard_ex(p, nshards, shard, 0u, out, needs_allreduce, nullptr, nullptr, nullptr);
}

int smr_shard_ex(const smr_problem* p, int nshards, int shard, uint32_t local_ops, smr_problem* out, int* needs_allreduce, int* split_dim,
                 int64_t* start_out, int64_t* stop_out) {
    if (!p || !out) return set_error(SMR_EINVAL, "null argument");
    if (nshards < 1 || shard < 0 || shard >= nshards) return set_error(SMR_EINVAL, "bad shard index");
    if (p->N < 1 || p->N > SMR_MAXN || p->M < 1 || p->M > SMR_MAXM) return set_error(SMR_EINVAL, "bad N/M");
    *out = *p;
    if (needs_allreduce) *needs_allreduce = 0;
    if (split_dim) *split_dim = -1;
    if (start_out) *start_out = 0;
    if (stop_out) *stop_out = 0;
    if (nshards == 1) return SMR_OK;
    // Split dim: the slowest-varying destination dim that is long enough (destination slabs
    // are then disjoint and contiguous-ish); for reductions prefer a kept dim so that no
    // exchange is needed -- the same race-freedom rule as src/mapreduce.jl:172-177.  Only when
    // no kept dim is long enough split a reduced dim and combine partials afterwards, like
    // the reference's complete-reduction branch (:153-170).
    int best = -1;
    int64_t beststride = -1;
    for (int i = 0; i < p->N; ++i) {
        int64_t s = p->ops[0].strides[i] < 0 ? -p->ops[0].strides[i] : p->ops[0].strides[i];
        if (s != 0 && p->dims[i] >= nshards && s > beststride) {
            best = i;
            beststride = s;
        }
    }
    int allred = 0;
    if (best < 0) {
        if (p->redop == SMR_RED_NONE) {
            // tiny map: give everything to shard 0, empty work elsewhere is not expressible
            // (dims >= 1), so fall back to the longest dim
            for (int i = 0; i < p->N; ++i)
                if (best < 0 || p->dims[i] > p->dims[best]) best = i;
            if (p->dims[best] < nshards) return set_error(SMR_EUNSUPPORTED, "box too small to shard");
        } else {
            int64_t bs = -1;
            for (int i = 0; i < p->N; ++i) {
                if (p->ops[0].strides[i] != 0 || p->dims[i] < nshards) continue;
                int64_t s = 0;
                for (int k = 1; k < p->M; ++k) {
                    int64_t v = p->ops[k].strides[i] < 0 ? -p->ops[k].strides[i] : p->ops[k].strides[i];
                    s = std::max(s, v);
                }
                if (s > bs) {
                    bs = s;
                    best = i;
                }
            }
            if (best < 0) return set_error(SMR_EUNSUPPORTED, "box too small to shard");
            allred = 1;
        }
    }
    const int64_t d = p->dims[best];
    const int64_t start = d * shard / nshards, end = d * (shard + 1) / nshards;
    out->dims[best] = end - start;
    // an operand flagged in local_ops is already this shard's slab: its base/offset address box index
    // `start` of the split dim (block-partitioned inputs: nothing is replicated); the others live in the whole
    // parent and get the reference's offset shift (src/mapreduce.jl:217-219)
    for (int k = 0; k < p->M; ++k)
        if (!((local_ops >> k) & 1u)) out->ops[k].offset = p->ops[k].offset + start * p->ops[k].strides[best];
    if (split_dim) *split_dim = best;
    if (start_out) *start_out = start;
    if (stop_out) *stop_out = end;
    if (allred && shard != 0) out->initop = SMR_INIT_NONE;  // initop is applied once, on shard 0
    if (needs_allreduce) *needs_allreduce = allred;
    return SMR_OK;
}

int smr_set_option(const char* name, int64_t value) {
    if (!name) return set_error(SMR_EINVAL, "null option name");
    Options& o = options();
    const std::string n(name);
    if (n == "stamp_base" || n == "stamp_cap" || n == "stamp_used") {  // no plan depends on these: keep the cache
        (n == "stamp_base" ? o.stamp_base : (n == "stamp_cap" ? o.stamp_cap : o.stamp_used)) = value;
        return SMR_OK;
    }
    if (n == "group_max_bytes") {  // read by the front ends only (smr_group.cpp): no plan depends on it either
        if (value < 0) return set_error(SMR_EINVAL, "group_max_bytes must be >= 0");
        group_max_bytes() = value;
        return SMR_OK;
    }
    if (n == "group_contract_tile") {  // read by smr_group_create only: no plan depends on it
        if (value != 0 && value != 16 && value != 32) return set_error(SMR_EINVAL, "group_contract_tile must be 0 (the rule), 16 or 32");
        group_contract_tile() = value;
        return SMR_OK;
    }
    if (n == "group_contract_split") {  // read by smr_group_create only, for contraction groups: no plan depends on it
        if (value < 0 || value > 0x7fffffffLL) return set_error(SMR_EINVAL, "group_contract_split must be 0 (never), 1 (the group rule) or the number of slices to force per member");
        group_contract_split() = value;
        return SMR_OK;
    }
    if (n == "contract_split" && value < 0) return set_error(SMR_EINVAL, "contract_split must be 0 (never), 1 (the rule) or the number of slices to force");
    if (n == "contract_tile" && value != 0 && value != 16 && value != 32 && value != 64) return set_error(SMR_EINVAL, "contract_tile must be 0 (the rule), 16, 32 or 64");
    if (i64 Options::*f = option_field(n)) o.*f = value;
    else if (const int d = tile_lg_dim(n); d >= 0) o.tile_lg[d] = value;
    else return set_error(SMR_EINVAL, "unknown option " + n);
    Cache& c = cache();
    std::vector<PlanRef> dropped;
    {
        std::lock_guard<std::mutex> g(c.mu);
        cache_clear_locked(c, dropped);
    }
    dropped.clear();
    return SMR_OK;
}

int64_t smr_get_option(const char* name) {
    if (!name) return -1;
    const Options& o = options();
    const std::string n(name);
    if (i64 Options::*f = option_field(n)) return o.*f;
    if (const int d = tile_lg_dim(n); d >= 0) return o.tile_lg[d];
    if (n == "stamp_base") return o.stamp_base;
    if (n == "stamp_cap") return o.stamp_cap;
    if (n == "stamp_used") return o.stamp_used;
    if (n == "stamp_build") return SMR_STAMP;
    if (n == "group_max_bytes") return group_max_bytes();
    if (n == "group_contract_tile") return group_contract_tile();
    if (n == "group_contract_split") return group_contract_split();
    // read-only counters
    if (n == "launches") return g_launches.load();
    if (n == "jit_compiles") return jit_stats().compiles;
    if (n == "jit_hits") return jit_stats().hits;
    if (n == "jit_failures") return jit_stats().failures;
    if (n == "jit_compile_ms") return (int64_t)jit_stats().compile_ms;
    if (n == "eager_launches") return eager_stat(0);
    if (n == "eager_free") return eager_stat(1);
    if (n == "eager_same") return eager_stat(2);
    if (n == "eager_cross") return eager_stat(3);
    if (n == "eager_fallback") return eager_stat(4);
    if (n == "eager_kernarg_device") return eager_stat(5);
    if (n == "eager_gpu_only_signals") return eager_stat(6);
    if (n == "eager_arg_hits") return eager_stat(7);
    if (n == "allreduces") return comm_stat(0);
    if (n == "allreduces_inplace") return comm_stat(1);
    return -1;
}

}  // extern "C"
