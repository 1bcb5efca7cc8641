// smr_eager.cpp -- eager direct dispatch on library-owned streams, on the direct queues of smr_direct.cpp.
#include <sched.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <set>

#include "smr_direct.h"

// ---- eager direct dispatch: the launches of a library-owned stream (smr_stream_create) ---------------------------------------------
// A host that routes ALL its device work through this library (the Julia shim) pays HIP's 3.6-4 us of host time per launch for kernels
// that last 2-5 us, and HIP orders every launch behind its predecessor.  On a library-owned stream the library submits the launch
// itself: the launchers run in recording mode (SMR_LAUNCH appends instead of launching), the kernel descriptor comes from the code
// object HIP loaded, the argument block goes into a ring of host-coherent slots, and ONE 64-byte packet + a doorbell go to one of up
// to four HSA queues.  Which queue is decided by the data: the bounding byte ranges of the operands (and the plan's partials) are
// compared with what is still in flight on every queue --
//   * no conflict anywhere  -> the queue with the least in flight: the launch runs CONCURRENTLY with its predecessors;
//   * conflicts on one queue -> that queue (the barrier bit orders it behind them);
//   * conflicts on several   -> one of them, behind a barrier-AND packet that waits for the last packet of each of the others.
// Every packet carries a completion signal from a per-queue ring; a signal that has reached 0 retires its launch's ranges.  Results
// are those of in-order execution on the stream (src/mapreduce.jl:203-223: spawn what is independent, wait where it must).
// The library fences by itself -- waits for every queue -- before anything it does on the stream through HIP (copies, synchronisation,
// sequence replays, the scalar result of a complete reduction), and drains HIP work it queued itself before the next direct launch.
namespace smr {
// Eager path: is the recent write set of this process small enough to stay in the Infinity Cache?  (Write-through stores pay off
// while the destinations are cache-resident and lose on partial lines that go to HBM: profiles/r05_bench_n1.json, cold 4-way sum.)
// A 16-slot direct-mapped table of recently written destinations (base address -> bytes); O(1) per call.
bool eager_recent_writes_fit(uintptr_t dest_lo, uintptr_t dest_hi) {
    static std::mutex mu;
    static uintptr_t key[16] = {};
    static size_t bytes[16] = {}, total = 0;
    std::lock_guard<std::mutex> g(mu);
    const unsigned slot = (unsigned)((dest_lo >> 12) * 0x9E3779B1u >> 28) & 15u;
    if (key[slot] != dest_lo || bytes[slot] != dest_hi - dest_lo) {
        total -= bytes[slot];
        key[slot] = dest_lo;
        bytes[slot] = dest_hi - dest_lo;
        total += bytes[slot];
    }
    return (i64)total <= options().self_release_max_total;
}
namespace {
constexpr int EAGER_Q = 4;          // hardware queues of the eager path (the first EAGER_Q of the device's direct queues)
constexpr int EAGER_SIGS = 256;     // launches in flight per queue
constexpr size_t EAGER_SLOT = 8192; // bytes of argument block per launch (TiledArgs<true> + hidden block fit)
struct Inflight {
    int sig;  // index into EagerQueue::sigs
    Spans rd, wr;
};
struct EagerQueue {
    std::vector<hsa_signal_t> sigs;
    std::vector<unsigned char> dep_user;  // bit k: a barrier-AND packet on queue k names this signal (several queues may name the same tail)
    std::vector<Inflight> inflight;  // oldest first
    unsigned next = 0;               // next signal / argument slot
    int tail = -1;                   // signal index of the last packet submitted when it carries one (-1: it does not, or nothing was submitted since the last fence)
    int unsignaled = 0;              // packets at the tail without a completion signal (0 with tail == -1: the queue is idle as far as we know)
    unsigned char* kargs = nullptr;  // EAGER_SIGS slots of EAGER_SLOT bytes, host-coherent
};
struct Eager {
    EagerQueue q[EAGER_Q];
    bool ready = false, failed = false, fail_reported = false;
    bool kargs_device = false, gpu_only_signals = false;
    // resident argument blocks (device memory only): a bump arena behind the per-queue rings; when it is full everything in flight is
    // waited for and the arena starts over (blocks of an older epoch are stale)
    unsigned char* arena = nullptr;
    size_t arena_bytes = 0, arena_used = 0;
    unsigned long long epoch = 1;
    long n_arg_hits = 0;
    std::set<hipStream_t> hip_pending;  // owned streams on which the library queued HIP work (a copy, a fallback launch) since their last drain:
                                        // a direct launch on stream s waits for s's own HIP work only -- streams are ordered in themselves, not among each other
    unsigned sys_acquire = ~0u; // bit k: the next direct launch on queue k follows work of another agent (a copy, a table upload): acquire at system scope
    std::map<std::string, std::pair<KernelRef, std::shared_ptr<void>>> jit;  // runtime-compiled kernels by entry-point name (module pinned)
    long n_launch = 0, n_free = 0, n_same = 0, n_cross = 0, n_fallback = 0;
};
std::mutex g_eager_mu;
std::map<int, Eager*> g_eager;
Eager& eager_of(int dev) {  // per device, like the direct queues it drives (one process per GPU is the usual case)
    std::lock_guard<std::mutex> g(g_eager_mu);
    Eager*& e = g_eager[dev];
    if (!e) e = new Eager();
    return *e;
}
std::vector<int> eager_devices() {
    std::lock_guard<std::mutex> g(g_eager_mu);
    std::vector<int> v;
    for (auto& kv : g_eager) v.push_back(kv.first);
    return v;
}

// a CPU agent (for hsa_amd_agents_allow_access) and a device-local pool the CPU may be given access to (large BAR)
struct PoolPick {
    Hsa* h;
    hsa_agent_t cpu{};
    bool have_cpu = false;
    hsa_amd_memory_pool_t pool{};
    bool have_pool = false;
};
hsa_status_t pick_cpu(hsa_agent_t a, void* data) {
    PoolPick* p = (PoolPick*)data;
    hsa_device_type_t t;
    if (!p->have_cpu && p->h->agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) == HSA_STATUS_SUCCESS && t == HSA_DEVICE_TYPE_CPU) {
        p->cpu = a;
        p->have_cpu = true;
    }
    return HSA_STATUS_SUCCESS;
}
hsa_status_t pick_pool(hsa_amd_memory_pool_t pool, void* data) {
    PoolPick* p = (PoolPick*)data;
    hsa_amd_segment_t seg;
    uint32_t flags = 0;
    bool alloc = false;
    if (p->h->pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_SEGMENT, &seg) != HSA_STATUS_SUCCESS || seg != HSA_AMD_SEGMENT_GLOBAL) return HSA_STATUS_SUCCESS;
    p->h->pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS, &flags);
    p->h->pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_RUNTIME_ALLOC_ALLOWED, &alloc);
    if (!alloc || !(flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_COARSE_GRAINED)) return HSA_STATUS_SUCCESS;
    hsa_amd_memory_pool_access_t acc = HSA_AMD_MEMORY_POOL_ACCESS_NEVER_ALLOWED;
    if (p->h->agent_pool_get_info(p->cpu, pool, HSA_AMD_AGENT_MEMORY_POOL_INFO_ACCESS, &acc) != HSA_STATUS_SUCCESS || acc == HSA_AMD_MEMORY_POOL_ACCESS_NEVER_ALLOWED)
        return HSA_STATUS_SUCCESS;
    p->pool = pool;
    p->have_pool = true;
    return HSA_STATUS_INFO_BREAK;
}

// Argument blocks: device memory the host writes through the BAR (what HIP itself does on this part: a kernel that fetches its
// arguments from host memory starts a PCIe round trip later), when the device-local pool can be mapped for the CPU; else pinned
// host memory.  $SMR_EAGER_KERNARG = host | device forces one.
unsigned char* eager_kernarg_ring(Direct& d, Eager& e, size_t bytes) {
    Hsa& h = hsa();
    const char* force = std::getenv("SMR_EAGER_KERNARG");
    const bool want_dev = !(force && std::strcmp(force, "host") == 0);
    if (want_dev && h.iterate_pools && h.pool_get_info && h.agent_pool_get_info && h.pool_allocate && h.allow_access) {
        PoolPick pp;
        pp.h = &h;
        h.iterate_agents(pick_cpu, &pp);
        if (pp.have_cpu) h.iterate_pools(d.agent, pick_pool, &pp);
        void* p = nullptr;
        if (pp.have_pool && h.pool_allocate(pp.pool, bytes, 0, &p) == HSA_STATUS_SUCCESS && p) {
            hsa_agent_t both[2] = {pp.cpu, d.agent};
            if (h.allow_access(2, both, nullptr, p) == HSA_STATUS_SUCCESS) {
                e.kargs_device = true;
                return (unsigned char*)p;
            }
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return (unsigned char*)p;
}

int eager_init(Direct& d, Eager& e) {
    if (e.ready) return SMR_OK;
    if (e.failed) return SMR_EUNSUPPORTED;
    Hsa& h = hsa();
    const char* sg = std::getenv("SMR_EAGER_SIGNALS");  // "interrupt": ordinary signals (experiments)
    const bool gpu_only = h.amd_signal_create && !(sg && std::strcmp(sg, "interrupt") == 0);
    e.gpu_only_signals = gpu_only;
    constexpr size_t ARENA = (size_t)16 << 20;
    unsigned char* ring = eager_kernarg_ring(d, e, (size_t)EAGER_Q * EAGER_SIGS * EAGER_SLOT + ARENA);
    if (!ring) {
        e.failed = true;
        return SMR_EUNSUPPORTED;
    }
    if (e.kargs_device) {
        e.arena = ring + (size_t)EAGER_Q * EAGER_SIGS * EAGER_SLOT;
        e.arena_bytes = ARENA;
    }
    for (int k = 0; k < EAGER_Q; ++k) {
        if (direct_queue(d, k) != SMR_OK) {
            e.failed = true;
            return SMR_EUNSUPPORTED;
        }
        EagerQueue& q = e.q[k];
        q.sigs.resize(EAGER_SIGS);
        q.dep_user.assign(EAGER_SIGS, 0);
        for (int i = 0; i < EAGER_SIGS; ++i) {
            // completion signals are polled by the host and consumed by barrier-AND packets: no interrupt, no event mailbox write
            const hsa_status_t st = gpu_only ? h.amd_signal_create(0, 0, nullptr, HSA_AMD_SIGNAL_AMD_GPU_ONLY, &q.sigs[i]) : h.signal_create(0, 0, nullptr, &q.sigs[i]);
            if (st != HSA_STATUS_SUCCESS) {
                e.failed = true;
                return SMR_EUNSUPPORTED;
            }
        }
        q.kargs = ring + (size_t)k * EAGER_SIGS * EAGER_SLOT;
    }
    e.ready = true;
    return SMR_OK;
}

// drop the launches whose completion signal has reached 0 (in submission order: a queue completes in order)
void eager_wait_queue(Eager& e, Direct& d, int k);

// (a queue completes in order: every packet carries the barrier bit; an entry without a signal of its own retires with the next
// signalled one behind it)
void eager_retire(EagerQueue& q) {
    Hsa& h = hsa();
    size_t done = 0;
    for (size_t i = 0; i < q.inflight.size(); ++i) {
        if (q.inflight[i].sig < 0) continue;
        if (h.signal_load(q.sigs[q.inflight[i].sig]) != 0) break;
        done = i + 1;
    }
    if (done) q.inflight.erase(q.inflight.begin(), q.inflight.begin() + (long)done);
}

int eager_take_signal(Eager& e, Direct& d, EagerQueue& q, int self);

// a marker: an empty barrier packet that completes when everything submitted to the queue before it has; returns its signal index
int eager_marker(Eager& e, Direct& d, EagerQueue& q, hsa_queue_t* hq, int self) {
    const int si = eager_take_signal(e, d, q, self);
    hsa_barrier_and_packet_t bp;
    std::memset(&bp, 0, sizeof bp);
    bp.completion_signal = q.sigs[si];
    (void)put_packet(d, hq, &bp, barrier_header(HSA_FENCE_SCOPE_NONE, HSA_FENCE_SCOPE_NONE), 0);
    Inflight f;
    f.sig = si;
    q.inflight.push_back(std::move(f));
    q.tail = si;
    q.unsignaled = 0;
    return si;
}

// (after a failure nothing is waited for any more: the bookkeeping is dropped, the caller learns about it from d.failed)
void eager_wait_queue(Eager& e, Direct& d, int k) {
    EagerQueue& q = e.q[k];
    if (!d.failed.load()) {
        if (q.unsignaled > 0) (void)eager_marker(e, d, q, d.q[k], k);
        if (q.tail >= 0) (void)wait_signal(d, q.sigs[q.tail]);
    }
    q.inflight.clear();
    q.tail = -1;
    q.unsignaled = 0;
}

// the next completion signal of queue `self` (a ring): the packet that used it EAGER_SIGS signalled submissions ago must have completed,
// and a barrier-AND packet of another queue that names it must have passed, before it is re-armed
int eager_take_signal(Eager& e, Direct& d, EagerQueue& q, int self) {
    Hsa& h = hsa();
    const int si = (int)(q.next % EAGER_SIGS);
    ++q.next;
    (void)wait_signal(d, q.sigs[si]);
    if (const unsigned users = q.dep_user[si]) {  // every queue whose barrier-AND packet names it must have consumed that packet
        q.dep_user[si] = 0;
        for (int k = 0; k < EAGER_Q; ++k)
            if (((users >> k) & 1u) && k != self) eager_wait_queue(e, d, k);
    }
    eager_retire(q);
    h.signal_store_relaxed(q.sigs[si], 1);
    return si;
}

bool conflicts(const EagerQueue& q, const Spans& rd, const Spans& wr) {
    for (const Inflight& f : q.inflight)
        if (overlaps(f.wr, wr) || overlaps(f.wr, rd) || overlaps(f.rd, wr)) return true;
    return false;
}


}  // namespace

// smr_api.cpp: the launches of one execution, recorded by the caller; rd / wr = its footprint.  SMR_OK, an error, or
// SMR_EUNSUPPORTED when this execution has to go through HIP (the caller fences and launches normally).
int eager_submit(const Plan& plan, std::vector<RecLaunch>& launches, const std::vector<std::pair<uintptr_t, uintptr_t>>& rd,
                 const std::vector<std::pair<uintptr_t, uintptr_t>>& wr, hipStream_t s) {
    const int dev = device_of(s);  // the stream's device, not the calling thread's current one
    Direct& d = direct_of(dev);
    if (!d.ok) return SMR_EUNSUPPORTED;
    std::lock_guard<std::mutex> g(d.mu);
    Eager& e = eager_of(dev);
    if (eager_init(d, e) != SMR_OK) return SMR_EUNSUPPORTED;
    // a sequence replay still in flight on these queues (asynchronous smr_seq_run) comes first
    for (int k = 0; k < SEQ_MAXQ; ++k)
        if (d.armed[k]) {
            if (!wait_signal(d, d.done[k])) return SMR_EHIP;
            d.armed[k] = false;
        }
    // kernels first: anything that cannot be dispatched directly sends the whole execution through HIP
    std::vector<KernelRef> refs(launches.size());
    for (size_t j = 0; j < launches.size(); ++j) {
        RecLaunch& l = launches[j];
        // runtime-compiled kernels are looked up by name once (the cache pins their module)
        auto it = l.hostfn ? e.jit.end() : e.jit.find(l.kname);
        const bool cached = it != e.jit.end();
        if (cached) refs[j] = it->second.first;
        const bool ok = resolve_launch(d, l, refs[j], nullptr);
        if (!cached && !l.hostfn && refs[j].object) {  // found by name just now, whatever the checks said
            if (e.jit.size() > 512) {  // unpins the modules (looked up again on their next use): nothing in flight may still run their code
                for (int k = 0; k < EAGER_Q; ++k) eager_wait_queue(e, d, k);
                e.jit.clear();
            }
            e.jit[l.kname] = std::make_pair(refs[j], l.keep);
        }
        if (!ok || std::max<size_t>(refs[j].kernarg_size, l.args.size()) > EAGER_SLOT) {
            ++e.n_fallback;
            return SMR_EUNSUPPORTED;
        }
    }
    if (e.hip_pending.count(s)) {  // what the library queued on THIS stream through HIP (a copy, a fallback launch) comes first
        hipError_t he = hipStreamSynchronize(s);
        if (he != hipSuccess) return hip_error(he, "draining the stream before a direct launch");
        e.hip_pending.erase(s);
        e.sys_acquire = ~0u;
    }
    // which queue
    int nconf = 0, conf[EAGER_Q], target = -1;
    for (int k = 0; k < EAGER_Q; ++k) {
        eager_retire(e.q[k]);
        if (conflicts(e.q[k], rd, wr)) conf[nconf++] = k;
    }
    if (nconf == 0) {
        size_t best = (size_t)-1;
        for (int k = 0; k < EAGER_Q; ++k)
            if (e.q[k].inflight.size() < best) {
                best = e.q[k].inflight.size();
                target = k;
            }
        ++e.n_free;
    } else {
        target = conf[0];
        for (int i = 1; i < nconf; ++i)
            if (e.q[conf[i]].inflight.size() > e.q[target].inflight.size()) target = conf[i];
        if (nconf == 1) ++e.n_same;
        else ++e.n_cross;
    }
    EagerQueue& q = e.q[target];
    hsa_queue_t* hq = d.q[target];
    if (nconf > 1) {  // wait (on the device) for the last packet of every other conflicting queue
        hsa_barrier_and_packet_t bp;
        std::memset(&bp, 0, sizeof bp);
        int nd = 0;
        for (int i = 0; i < nconf; ++i)
            if (conf[i] != target) {
                EagerQueue& o = e.q[conf[i]];
                if (o.unsignaled > 0) (void)eager_marker(e, d, o, d.q[conf[i]], conf[i]);  // its last packet carries no signal: a marker behind it does
                if (o.tail >= 0) {
                    bp.dep_signal[nd++] = o.sigs[o.tail];
                    o.dep_user[o.tail] |= (unsigned char)(1u << target);
                }
            }
        if (!put_packet(d, hq, &bp, barrier_header(HSA_FENCE_SCOPE_AGENT, HSA_FENCE_SCOPE_AGENT), 0)) return SMR_EHIP;
    }
    for (size_t j = 0; j < launches.size(); ++j) {
        const RecLaunch& l = launches[j];
        // completion signals are expensive on the device side (the packet processor updates one in host memory before it goes on: a
        // dependent chain with a signal per packet ran at 4.5 us per launch, 2.9 without): with resident argument blocks only every
        // 8th launch of a queue carries one (it retires its predecessors too; fences and cross-queue waits add a marker on demand);
        // with argument blocks in the per-launch ring slots every launch needs its own
        const bool want_sig = !e.arena || q.unsignaled >= 7;
        const int si = want_sig ? eager_take_signal(e, d, q, target) : -1;
        if (d.failed.load()) return SMR_EHIP;
        // the argument block: a resident one when this plan's launch j was issued with these very bytes before (the hot loop of a
        // host program), else a fresh block -- in the arena when there is one (it becomes resident), in the launch's ring slot otherwise
        unsigned char* b = nullptr;
        bool fresh = true;
        if (e.arena) {
            for (Plan::ArgBlock& ab : plan.eager_args)
                if (ab.launch == (int)j && ab.dev_index == dev && ab.epoch == e.epoch && ab.bytes.size() == l.args.size() && std::memcmp(ab.bytes.data(), l.args.data(), l.args.size()) == 0) {
                    b = (unsigned char*)ab.dev;
                    fresh = false;
                    ++e.n_arg_hits;
                    break;
                }
            if (!b) {
                const size_t need = (std::max<size_t>(refs[j].kernarg_size, l.args.size()) + 255) & ~(size_t)255;
                if (e.arena_used + need > e.arena_bytes) {  // start over: nothing in flight may still read an old block
                    for (int k = 0; k < EAGER_Q; ++k) eager_wait_queue(e, d, k);
                    e.arena_used = 0;
                    ++e.epoch;
                }
                b = e.arena + e.arena_used;
                e.arena_used += need;
                if (plan.eager_args.size() >= 8) plan.eager_args.erase(plan.eager_args.begin());  // a few rebinding patterns per plan
                Plan::ArgBlock ab;
                ab.launch = (int)j;
                ab.bytes = l.args;
                ab.dev = b;
                ab.dev_index = dev;
                ab.epoch = e.epoch;
                plan.eager_args.push_back(std::move(ab));
            }
        } else {
            b = q.kargs + (size_t)si * EAGER_SLOT;
        }
        if (fresh) {
            // explicit arguments, then the hidden ones at the offsets the code object's metadata names (block counts, group sizes,
            // grid dims, dynamic LDS size); staged in host memory: the block itself may be device memory behind the BAR
            std::vector<unsigned char> img(std::max<size_t>(refs[j].kernarg_size, l.args.size()), 0);
            fill_kernarg_image(refs[j], l, l.grid, img.data(), img.size());
            std::memcpy(b, img.data(), img.size());
            if (e.kargs_device) {  // posted writes through the BAR: a read of the last byte written returns only after they have landed
                const size_t used = std::max<size_t>(l.args.size(), refs[j].kernarg_size);
                __atomic_thread_fence(__ATOMIC_SEQ_CST);
                volatile unsigned char sink = ((volatile unsigned char*)b)[used ? used - 1 : 0];
                (void)sink;
            }
        }
        hsa_kernel_dispatch_packet_t pk = dispatch_packet(refs[j], l.grid, l.block, l.lds, b);
        pk.completion_signal = si >= 0 ? q.sigs[si] : hsa_signal_t{0};
        // agent-scope fences like HIP's between kernels (the argument block is host-coherent memory, never cached in L2); the first
        // launch after a copy acquires at system scope
        // (a self-released launch -- write-through stores, acknowledged before its waves end -- leaves nothing dirty in an L2: no release)
        if (!put_packet(d, hq, &pk,
                        header_of(true, ((e.sys_acquire >> target) & 1u) ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT, l.self_released ? HSA_FENCE_SCOPE_NONE : HSA_FENCE_SCOPE_AGENT),
                        pk.setup))
            return SMR_EHIP;
        e.sys_acquire &= ~(1u << target);
        Inflight f;
        f.sig = si;
        if (j + 1 == launches.size()) {  // the execution's ranges retire with its LAST launch
            f.rd = rd;
            f.wr = wr;
        }
        q.inflight.push_back(std::move(f));
        q.tail = si;
        q.unsignaled = si >= 0 ? 0 : q.unsignaled + 1;
        ++e.n_launch;
        count_launch();
    }
    return SMR_OK;
}

// everything submitted directly -- on every device this process drove that way -- has completed when this returns (host wait).
// SMR_OK, or SMR_EHIP when a device's direct path failed (now or earlier, reported once): its results are then undefined.
int eager_fence_all() {
    int rc = SMR_OK;
    for (int dev : direct_devices()) {
        Direct& d = direct_of(dev);
        std::lock_guard<std::mutex> g(d.mu);
        Eager& e = eager_of(dev);
        const bool was_failed = d.failed.load();
        if (e.ready)
            for (int k = 0; k < EAGER_Q; ++k) eager_wait_queue(e, d, k);
        (void)wait_all(d);  // a sequence replay submitted asynchronously (smr_seq_run) shares the queues
        if (d.failed.load() && !(was_failed && e.fail_reported)) {
            e.fail_reported = true;
            {
                std::string fw;
                {
                    std::lock_guard<std::mutex> g(d.why_mu);
                    fw = d.fail_why;
                }
                rc = set_error(SMR_EHIP, "direct dispatch: " + (fw.empty() ? std::string("the HSA queue reported an error") : fw));
            }
        }
    }
    return rc;
}
void eager_note_hip_work(hipStream_t s) {
    const int dev = device_of(s);
    Direct& d = direct_of(dev);
    if (!d.ok) return;
    std::lock_guard<std::mutex> g(d.mu);
    eager_of(dev).hip_pending.insert(s);
}
void eager_forget_stream(hipStream_t s) {  // the stream is being destroyed (its handle may be reused)
    for (int dev : eager_devices()) {
        Direct& d = direct_of(dev);
        std::lock_guard<std::mutex> g(d.mu);
        eager_of(dev).hip_pending.erase(s);
    }
}
void eager_request_sys_acquire(hipStream_t s) {  // device memory was written behind the queues' backs (a table upload by hipMemcpy)
    const int dev = device_of(s);
    Direct& d = direct_of(dev);
    if (!d.ok) return;
    std::lock_guard<std::mutex> g(d.mu);
    eager_of(dev).sys_acquire = ~0u;
}
long eager_stat(int which) {
    const int dev = current_device();
    Direct& d = direct_of(dev);
    std::lock_guard<std::mutex> g(d.mu);  // (the counters are written under the same lock)
    Eager& e = eager_of(dev);
    switch (which) {
        case 0: return e.n_launch;
        case 1: return e.n_free;
        case 2: return e.n_same;
        case 3: return e.n_cross;
        case 5: return e.kargs_device ? 1 : 0;
        case 7: return e.n_arg_hits;
        case 6: return e.gpu_only_signals ? 1 : 0;
        default: return e.n_fallback;
    }
}
bool eager_hip_pending(int dev, hipStream_t s) { return eager_of(dev).hip_pending.count(s) != 0; }
void eager_hip_drained(int dev, hipStream_t s) { eager_of(dev).hip_pending.erase(s); }
bool eager_available(hipStream_t s) { return direct_of(device_of(s)).ok; }
// for paths that must not create the direct queues as a side effect (freeing memory, destroying plans)
int eager_fence_if_active() {
    if (direct_devices().empty()) return SMR_OK;
    return eager_fence_all();
}
}  // namespace smr
