// smr_seq.cpp -- recorded sequences of plan and group executions, replayed as hand-built AQL packets on the library's own HSA queue.
//
// Why.  The reference runs independent pieces of work as concurrent tasks and waits only where it must (src/mapreduce.jl:203-223).
// On MI355X the unit is the LAUNCH, and a stream-ordered launch of 16 MiB is a span of 1.6-3.2 us plus a 1.6-1.9 us boundary (drain,
// write-back, next dispatch) even when its successor touches none of its data.  What round 4 measured (profiles/r04_overlap.txt):
//   * HIP accepts hipExtAnyOrderLaunch but ignores it on gfx9 (hip_ext.h says so; the device stamps confirm it): through HIP every
//     packet of a stream carries the AQL barrier bit;
//   * two HIP streams do overlap the two kernels of the bench step (8.6 -> 6.2 us per step) -- when two host threads feed them: HIP's
//     eager launch path costs 3.6-4 us of host time per launch, one thread cannot feed two queues;
//   * a hipGraph with two branches is executed node by node through that same eager path (8.2-8.8 us per step), only single-chain
//     graphs get the batched submission.
// So the library submits its own packets: a sequence is recorded ONCE (every launch's kernel object, grid and kernarg block, resident
// in device memory), a dependency analysis (byte ranges read / written: footprint() in smr_api.cpp) decides per launch whether
// its packet carries the barrier bit, and a replay is N x 64-byte stores into the queue rings plus a doorbell per queue -- ~0.1 us of
// host time per launch, no host thread in the loop.  Independent launches go to DIFFERENT hardware queues (one per dependency
// component): inside one queue the packet processor runs consecutive dispatches one after the other on their agent-scope fences even
// with the barrier bit clear (measured with device stamps, profiles/r04_overlap.txt); two queues do overlap.
//
// Kernel objects come from the code objects HIP itself has loaded: host stub -> kernel name (hipKernelNameRefByPtr) -> "<name>.kd" looked
// up in the process's HSA executables (loader extension 1.03: hsa_ven_amd_loader_iterate_executables).  Nothing is loaded twice.
// Ordering against the caller's HIP stream: smr_seq_run waits (on the host) for `stream` to drain when it is busy, and makes it wait for
// the replay with hipStreamWaitValue64 on the completion signal's value -- "as if the sequence had been launched in order on stream".
// The direct-dispatch layer underneath is smr_direct.cpp; what goes to which queue, cut how, ordered and fenced how, is decided by
// schedule() (smr_sched.cpp), which needs no device.
#include <sched.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "smr_direct.h"

using namespace smr;

// ---- the sequence object ----------------------------------------------------------------------------------------------------------
struct SeqItem {  // one recorded execution: of a plan (with optional rebinding of base pointers) or of a group (`plan` is null)
    smr_plan* plan;
    smr_group* group;
    bool has_bases;
    void* bases[SMR_MAXM];
};
struct SeqPacket {
    hsa_kernel_dispatch_packet_t pk;  // header / completion signal filled in at replay
    bool barrier;
    bool acquire;  // the launch reads bytes some launch of the sequence writes (read-after-write, accumulation, in-place update)
    bool self_released;  // every store of the launch is written through and acknowledged before the kernel ends: no release fence needed
};
struct smr_seq {
    std::vector<SeqItem> items;
    bool built = false;
    bool aql = false;           // every launch is a precompiled kernel without scratch: replayed as AQL packets
    std::string why_not_aql;
    std::vector<SeqPacket> packets[SEQ_MAXQ];  // one replay's packets, per hardware queue
    int nq = 0;                 // queues in use (= dependency components of the recorded list, at most max_queues)
    int max_queues = 4;         // measured: beyond 4 queues of its own a process is time-multiplexed by the hardware scheduler (6 queues: 6.0 -> 11.1 us per step)
    int slices = -1;            // a component that is ONE independent-workgroup launch is cut into this many block ranges, one queue each;
                                // -1 (default): automatic, only the heaviest chain is cut (schedule(), step 3b); 1: never
    std::map<int, int> comp_slices;  // "slices:<c>": block ranges of component c alone (asymmetric: only the long chain is cut)
    int nsliced = 0;            // components that were
    int ncomp = 0;
    void* d_kernargs = nullptr;
    std::vector<std::shared_ptr<void>> keep;  // runtime-compiled programs the packets name
    int64_t runs = 0;
    int n_any = 0, n_barrier = 0, n_acquire = 0, n_self_released = 0;
    // Fences of the packets INSIDE a replay (the first packet on a queue always acquires, the last always releases, at system scope).
    //   acquire: -1 = by need (default): agent scope on a launch that reads bytes which some launch of the sequence WRITES -- a
    //            read-after-write, a reduction accumulating into its destination, an in-place map -- and none on a launch whose
    //            inputs nobody in the sequence writes: an acquire invalidates every XCD's L2, i.e. it throws away the read-only
    //            inputs the next replay (and whatever runs concurrently on the other queues) would have hit there, and it is only
    //            needed to observe another workgroup's writes.  0 none / 1 agent / 2 system force one scope (experiments).
    //   release: 1 agent (default; the next writer of the same bytes may sit on another XCD: write-after-write needs the
    //            write-back), 0 none (experiment: NOT safe in general), 2 system.
    int acq_mid = -1, rel_mid = 1;
    // Scope of a replay's FIRST acquire on every queue: -1 (default) = by the memory the sequence reads -- agent scope when every
    // operand it reads lives in device-local memory of this GPU (hipMalloc): what an acquire has to do is drop THIS device's stale
    // cache lines, and for local memory the agent-scope invalidate drops all of them, whoever wrote the new data (a DMA copy, the
    // host through the BAR, a kernel of a peer device write to memory, not into these L2s; tests/test_gpu_round5.py replays after a
    // DMA upload); system scope as soon as an operand is host memory (pinned, zero-copy) or managed, or its type cannot be told.
    // Measured: the system-scope acquire costs a replay 6-7 us (profiles/r05_seq_fixed_cost.txt).  0 / 1 / 2 force a scope.
    // The LAST release stays at system scope (default 2): measured no cheaper at agent scope.
    int rel_self = 0;  // release scope of self-released launches' packets inside a replay: 0 none (default), 1 = like the others (experiment)
    int acq_first = -1, rel_last = 2;
    int acq_first_auto = 2;  // what -1 resolved to at build time
    bool all_ordered = false;   // experiment: every packet carries the barrier bit
    bool inflight = false;      // a replay was submitted and nobody waited for it yet
    int device = -1;            // the device the sequence was built for (its plans' tables and the kernarg blocks live there)
    int async_mode = -1;        // smr_seq_run returns after the doorbells: -1 automatic (see smr_seq_run), 0 never (wait inside), 1 always
    bool held = false;          // the last replay put a holding kernel on the caller's stream
};


namespace {
// a kernel on the caller's stream that holds the stream back until the replay's completion signals (host memory) read zero: makes
// smr_seq_run asynchronous on devices without hipStreamWaitValue64.  Bounded: after ~`limit` ticks of the 100 MHz device clock it
// gives up and raises *gave_up (the host reports it from smr_seq_wait).
__global__ void k_seq_hold(const volatile long long* const* sigs, int n, unsigned long long limit, unsigned* gave_up) {
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    for (int k = 0; k < n; ++k)
        while (__hip_atomic_load((const long long*)sigs[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) {
            __builtin_amdgcn_s_sleep(64);
            if (wall_clock64() - t0 > limit) {
                __hip_atomic_store(gave_up, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return;
            }
        }
}

// ---- building: record, resolve, schedule(), kernarg blocks, packets ------------------------------------------------------------------
struct Rec {
    std::vector<RecLaunch> launches;
    std::vector<KernelRef> refs;
    std::vector<size_t> offs;  // of launch j's first kernarg block in d_kernargs (a sliced launch has one block per slice, back to back)
    size_t blocksize(size_t j) const { return (std::max<size_t>(refs[j].kernarg_size, launches[j].args.size()) + 255) & ~(size_t)255; }
};
void* const* bases_of(const SeqItem& it) { return it.has_bases ? it.bases : nullptr; }
// an item executes (or, prepare_only: builds whatever its first execution would build) as what it is
int seq_execute_item(const SeqItem& it, hipStream_t s, bool prepare_only) {
    return it.group ? seq_execute_group(it.group, s, prepare_only) : seq_execute_plan(it.plan, bases_of(it), s, prepare_only);
}

// the footprints of the recorded executions, as the scheduler wants them (launch facts are added by seq_record)
std::vector<SchedExec> seq_footprints(smr_seq* q) {
    std::vector<SchedExec> ex(q->items.size());
    for (size_t i = 0; i < ex.size(); ++i) {
        const SeqItem& it = q->items[i];
        if (it.group) seq_footprint_group(it.group, ex[i].rd, ex[i].wr);
        else seq_footprint(it.plan, bases_of(it), ex[i].rd, ex[i].wr);
        ex[i].same_as = (int)i;
        for (size_t j = 0; j < i && ex[i].same_as == (int)i; ++j) {
            const SeqItem& o = q->items[j];
            if (o.plan == it.plan && o.group == it.group && o.has_bases == it.has_bases && !(it.has_bases && std::memcmp(it.bases, o.bases, sizeof it.bases) != 0)) ex[i].same_as = (int)j;
        }
    }
    return ex;
}
SchedKnobs seq_knobs(const smr_seq* q) {
    SchedKnobs k;
    k.max_queues = std::max(1, std::min(q->max_queues, SEQ_MAXQ));
    k.slices = q->slices;
    k.comp_slices = q->comp_slices;
    k.all_ordered = q->all_ordered;
    k.self_release_max_total = options().self_release_max_total;
    return k;
}

// 1. + 2. record every launch of every item (tables uploaded / scratch allocated by a prepare pass first); launches may be
// self-released only while everything the sequence touches stays in the caches (schedule(): cache_resident)
int seq_record(smr_seq* q, std::vector<Rec>& recs, std::vector<SchedExec>& ex) {
    for (const SeqItem& it : q->items)
        if (int rc = seq_execute_item(it, nullptr, true)) return rc;
    ex = seq_footprints(q);
    const bool allow_self = schedule(ex, seq_knobs(q)).cache_resident;
    for (size_t i = 0; i < q->items.size(); ++i) {
        set_recorder(&recs[i].launches, allow_self);
        int rc = seq_execute_item(q->items[i], nullptr, false);
        set_recorder(nullptr);
        if (rc) return rc;
        if (recs[i].launches.empty()) return set_error(SMR_EINVAL, "smr_seq: an item recorded no launch");
        const RecLaunch& l0 = recs[i].launches[0];
        ex[i].nlaunch = (int)recs[i].launches.size();
        ex[i].grid = l0.grid;
        ex[i].sliceable = l0.slice_kind != 0;
        ex[i].all_self = true;
        for (const RecLaunch& l : recs[i].launches) ex[i].all_self = ex[i].all_self && l.self_released;
        // a split contraction group: the partials' launch (sliceable) and the fold, which needs all of it
        ex[i].fold_after = q->items[i].group != nullptr && ex[i].nlaunch == 2 && ex[i].sliceable;
    }
    return SMR_OK;
}

// 3. resolve kernels (the device's kernel map and queues are shared with the eager path: the caller holds d.mu).  false: some launch
// cannot be dispatched directly (q->why_not_aql says which): the sequence replays through HIP
bool seq_resolve(smr_seq* q, Direct& d, std::vector<Rec>& recs) {
    for (Rec& r : recs)
        for (const RecLaunch& l : r.launches) {
            if (l.keep) q->keep.push_back(l.keep);
            KernelRef k;
            if (!resolve_launch(d, l, k, &q->why_not_aql)) return false;
            r.refs.push_back(k);
        }
    return true;
}

// 6. kernarg blocks (explicit arguments + the code-object-v5 hidden block), one resident copy in device memory; a sliced launch
//    has one block per slice (its block-offset field / list pointer patched)
int seq_kernargs(smr_seq* q, std::vector<Rec>& recs, const Schedule& sc) {
    size_t total = 0;
    for (size_t i = 0; i < recs.size(); ++i)
        for (size_t j = 0; j < recs[i].launches.size(); ++j) {
            recs[i].offs.push_back(total);
            total += recs[i].blocksize(j) * (size_t)sc.nslices[i];
        }
    std::vector<unsigned char> host(total, 0);
    for (size_t i = 0; i < recs.size(); ++i)
        for (size_t j = 0; j < recs[i].launches.size(); ++j) {
            const RecLaunch& l = recs[i].launches[j];
            const int ns = sc.nslices[i];
            for (int s2 = 0; s2 < ns; ++s2) {
                unsigned lo = 0, hi = l.grid;
                if (ns > 1 && l.slice_kind != 0) slice_range(l.grid, ns, s2, lo, hi);  // (a launch that is not cut -- a fold behind a cut launch -- keeps its grid in every block)
                unsigned char* b = host.data() + recs[i].offs[j] + (size_t)s2 * recs[i].blocksize(j);
                // the hidden arguments carry this slice's block count
                fill_kernarg_image(recs[i].refs[j], l, hi - lo, b, recs[i].blocksize(j));
                if (ns > 1 && l.slice_kind == 1) {  // a 32-bit "first block" field inside the argument block
                    uint32_t v;
                    std::memcpy(&v, b + l.slice_off, 4);
                    v += lo;
                    std::memcpy(b + l.slice_off, &v, 4);
                } else if (ns > 1 && l.slice_kind == 2) {  // a pointer to a per-workgroup table: advanced by `lo` rows
                    uint64_t v;
                    std::memcpy(&v, b + l.slice_off, 8);
                    v += (uint64_t)lo * l.slice_row;
                    std::memcpy(b + l.slice_off, &v, 8);
                }
#if SMR_STAMP
                // stamp build: the last explicit argument is the launch's stamp region (16 bytes per wave, indexed by the slice-relative
                // blockIdx.x): every slice gets its own part of it
                if (ns > 1 && l.args.size() >= 8) {
                    uint64_t sp = 0;
                    std::memcpy(&sp, b + l.args.size() - 8, 8);
                    if (sp) {
                        sp += (uint64_t)lo * ((l.block + 63) / 64) * 16;
                        std::memcpy(b + l.args.size() - 8, &sp, 8);
                    }
                }
#endif
            }
        }
    if (q->d_kernargs) (void)hipFree(q->d_kernargs);
    q->d_kernargs = nullptr;
    hipError_t e = hipMalloc(&q->d_kernargs, total ? total : 256);
    if (e != hipSuccess) return hip_error(e, "hipMalloc(sequence kernargs)");
    e = hipMemcpy(q->d_kernargs, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_error(e, "hipMemcpy(sequence kernargs)");
    return SMR_OK;
}

// 7. where the memory the sequence READS lives (first acquire: see smr_seq::acq_first)
int seq_first_acquire_scope(const std::vector<SchedExec>& ex, int device) {
    for (const SchedExec& r : ex)
        for (const auto& x : r.rd) {
            hipPointerAttribute_t at;
            std::memset(&at, 0, sizeof at);
            const bool local = x.second > x.first && hipPointerGetAttributes(&at, (const void*)x.first) == hipSuccess && at.type == hipMemoryTypeDevice &&
                               !at.isManaged && at.device == device;
            if (!local) {
                (void)hipGetLastError();
                return HSA_FENCE_SCOPE_SYSTEM;
            }
        }
    return HSA_FENCE_SCOPE_AGENT;
}

int seq_build(smr_seq* q) {
    for (auto& v : q->packets) v.clear();
    q->keep.clear();
    q->aql = false;
    q->n_any = q->n_barrier = q->n_acquire = q->n_self_released = 0;
    q->nq = 0;
    q->nsliced = 0;
    q->device = current_device();  // the plans' tables are uploaded (prepare pass below) on the calling thread's device
    Direct& d = direct_of(q->device);
    if (!d.ok) {
        std::lock_guard<std::mutex> g(d.why_mu);
        q->why_not_aql = d.why;
    }
    std::vector<Rec> recs(q->items.size());
    std::vector<SchedExec> ex;
    if (int rc = seq_record(q, recs, ex)) return rc;
    std::unique_lock<std::mutex> dlock(d.mu);
    const bool aql = d.ok && seq_resolve(q, d, recs);
    dlock.unlock();
    q->aql = aql;
    q->built = true;
    if (!aql) return SMR_OK;
    const Schedule sc = schedule(ex, seq_knobs(q));
    q->ncomp = sc.ncomp;
    q->nsliced = sc.nsliced;
    dlock.lock();
    for (int k = 0; k < sc.nq; ++k)
        if (int rc = direct_queue(d, k)) return rc;
    dlock.unlock();
    q->nq = sc.nq;
    if (int rc = seq_kernargs(q, recs, sc)) return rc;
    q->acq_first_auto = seq_first_acquire_scope(ex, q->device);
    // 8. the schedule's entries as packets (header / completion signal filled in at replay)
    for (int k = 0; k < sc.nq; ++k)
        for (const SchedEntry& e : sc.queues[k]) {
            const Rec& r = recs[e.exec];
            const RecLaunch& l = r.launches[e.launch];
            const unsigned nblocks = (sc.nslices[e.exec] > 1 && e.launch == 0) ? e.hi - e.lo : l.grid;  // (only a first launch is ever cut)
            if (nblocks == 0) continue;  // an empty launch
            SeqPacket sp;
            std::memset(&sp, 0, sizeof sp);
            sp.barrier = e.barrier;
            sp.acquire = e.acquire;
            sp.self_released = l.self_released;
            if (sp.self_released) ++q->n_self_released;
            (sp.barrier ? q->n_barrier : q->n_any)++;
            if (sp.acquire) ++q->n_acquire;
            sp.pk = dispatch_packet(r.refs[e.launch], nblocks, l.block, l.lds, (char*)q->d_kernargs + r.offs[e.launch] + (size_t)e.slice * r.blocksize(e.launch));
            q->packets[k].push_back(sp);
        }
    return SMR_OK;
}

// writes `reps` replays into the rings; the last packet on every queue signals that queue's d.done
int seq_submit(smr_seq* q, Direct& d, int reps) {
    Hsa& h = hsa();
    const int acq_mid = q->acq_mid, rel_mid = q->rel_mid;
    uint64_t written[SEQ_MAXQ] = {}, totalp[SEQ_MAXQ] = {};
    int open_queues = 0;
    for (int k = 0; k < q->nq; ++k) {
        totalp[k] = (uint64_t)q->packets[k].size() * (uint64_t)reps;
        d.armed[k] = totalp[k] > 0;
        if (totalp[k]) {
            h.signal_store_relaxed(d.done[k], 1);
            ++open_queues;
        }
    }
    d.t_submit = now_s();
    // the limit is on the ABSENCE OF PROGRESS, as in wait_signal: a replay longer than the rings (16384 packets per queue) that runs
    // for minutes keeps draining and keeps being fed -- the clock restarts with every packet written (it used to run
    // from t_submit, so a legitimate replay of more than SMR_DIRECT_TIMEOUT_MS was declared dead while its rings were full)
    double t_progress = d.t_submit;
    unsigned idle_rounds = 0;
    while (open_queues > 0) {
        // every ring full (the replay is longer than the rings: the packet processor has to catch up): spin briefly, then yield; bounded
        if (++idle_rounds > 64) {
            if (idle_rounds < 1024) __builtin_ia32_pause();
            else sched_yield();
            if ((idle_rounds & 1023) == 0 && (d.failed.load() || now_s() - t_progress > direct_timeout_s())) {
                direct_fail(d, "the hardware queues stopped consuming packets during a replay");
                return SMR_EHIP;
            }
        }
        for (int k = 0; k < q->nq; ++k) {
            if (written[k] >= totalp[k]) continue;
            hsa_queue_t* hq = d.q[k];
            const uint32_t mask = hq->size - 1;
            const size_t np = q->packets[k].size();
            // as many packets as the ring has room for, at most 256 per visit so that every queue is fed early
            const uint64_t widx = h.add_write_index(hq, 0);
            const uint64_t room = hq->size - (widx - h.load_read_index(hq));
            if (room == 0) continue;  // the packet processor is behind: visit the other queues, come back
            const uint64_t nthis = std::min<uint64_t>({room, totalp[k] - written[k], (uint64_t)256});
            const uint64_t base = h.add_write_index(hq, nthis);
            for (uint64_t t = 0; t < nthis; ++t) {
                const uint64_t g = written[k] + t;
                const SeqPacket& sp = q->packets[k][g % np];
                hsa_kernel_dispatch_packet_t* slot = (hsa_kernel_dispatch_packet_t*)hq->base_address + ((base + t) & mask);
                const bool first = g == 0, last = g + 1 == totalp[k];
                hsa_kernel_dispatch_packet_t pk = sp.pk;
                pk.completion_signal = last ? d.done[k] : hsa_signal_t{0};
                // body first, header last (release): the packet processor owns the slot once the header is valid
                std::memcpy((char*)slot + 4, (const char*)&pk + 4, sizeof pk - 4);
                const int acq = acq_mid >= 0 ? acq_mid : (sp.acquire ? HSA_FENCE_SCOPE_AGENT : HSA_FENCE_SCOPE_NONE);
                // release: the last packet on a queue at system scope; inside the replay agent scope -- none for a self-released
                // launch (its stores were written through and acknowledged before it ended: nothing is dirty in an L2)
                const int rel = (sp.self_released && q->rel_self == 0) ? HSA_FENCE_SCOPE_NONE : rel_mid;
                const uint16_t hdr = header_of(sp.barrier || first, first ? (q->acq_first >= 0 ? q->acq_first : q->acq_first_auto) : acq, last ? q->rel_last : rel);
                __atomic_store_n((uint32_t*)slot, (uint32_t)hdr | ((uint32_t)pk.setup << 16), __ATOMIC_RELEASE);
            }
            h.signal_store_screlease(hq->doorbell_signal, (hsa_signal_value_t)(base + nthis - 1));
            idle_rounds = 0;
            t_progress = now_s();
            written[k] += nthis;
            if (written[k] >= totalp[k]) --open_queues;
        }
    }
    return SMR_OK;
}

// the holding kernel's view of the completion signals (device-visible host memory, one block per device, made on first use)
struct HoldBlock {
    const volatile long long** sigs = nullptr;  // [SEQ_MAXQ]
    unsigned* gave_up = nullptr;
};
HoldBlock* hold_block(Direct& d) {
    static std::mutex mu;
    static std::map<int, HoldBlock> all;
    std::lock_guard<std::mutex> g(mu);
    HoldBlock& hb = all[d.dev];
    if (!hb.sigs) {
        void* p = nullptr;
        if (hipHostMalloc(&p, 256, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        std::memset(p, 0, 256);
        hb.sigs = (const volatile long long**)p;
        hb.gave_up = (unsigned*)((char*)p + 128);
    }
    return &hb;
}
}  // namespace

extern "C" {

int smr_seq_create(smr_seq** out) {
    if (!out) return set_error(SMR_EINVAL, "null out");
    *out = new (std::nothrow) smr_seq();
    return *out ? SMR_OK : set_error(SMR_ENOMEM, "out of host memory");
}

int smr_seq_add(smr_seq* q, smr_plan* plan, void* const* bases) {
    if (!q || !plan) return set_error(SMR_EINVAL, "null argument");
    if (q->inflight) return set_error(SMR_EINVAL, "smr_seq_add: a replay is in flight (smr_seq_wait first)");
    SeqItem it;
    std::memset(&it, 0, sizeof it);
    it.plan = plan;
    it.has_bases = bases != nullptr;
    if (bases)
        for (int k = 0; k < seq_nops(plan); ++k) it.bases[k] = bases[k];
    q->items.push_back(it);
    q->built = false;
    return SMR_OK;
}

int smr_seq_add_group(smr_seq* q, smr_group* group) {
    if (!q || !group) return set_error(SMR_EINVAL, "null argument");
    if (q->inflight) return set_error(SMR_EINVAL, "smr_seq_add_group: a replay is in flight (smr_seq_wait first)");
    SeqItem it;
    std::memset(&it, 0, sizeof it);
    it.group = group;
    q->items.push_back(it);
    q->built = false;
    return SMR_OK;
}

int smr_seq_run(smr_seq* q, int reps, void* stream) {
    if (!q || reps < 1) return set_error(SMR_EINVAL, "smr_seq_run: null sequence or reps < 1");
    if (q->items.empty()) return set_error(SMR_EINVAL, "smr_seq_run: empty sequence");
    hipStream_t s = (hipStream_t)stream;
    if (!q->built) {
        int rc = seq_build(q);
        if (rc) return rc;
    }
    if (q->aql && device_of(s) != q->device) return set_error(SMR_EINVAL, "smr_seq_run: the stream belongs to another device than the one the sequence was built on");
    if (q->aql && !direct_of(q->device).ok) {  // the direct path failed after the sequence was built: from now on through HIP
        q->aql = false;
        q->why_not_aql = direct_of(q->device).why;
    }
    if (!q->aql) {  // HIP path: the same launches, in order on the caller's stream
        for (int r = 0; r < reps; ++r)
            for (SeqItem& it : q->items) {
                int rc = seq_execute_item(it, s, false);
                if (rc) return rc;
            }
        ++q->runs;
        return SMR_OK;
    }
    Direct& d = direct_of(q->device);
    if (int rc = eager_fence_all()) return rc;  // launches a library-owned stream submitted directly share these queues: they come first
    std::lock_guard<std::mutex> g(d.mu);
    // the previous replay on these queues must have completed before the completion signals are re-armed
    if (int rc = wait_all(d)) return rc;
    // whatever the caller queued on `stream` before comes first (a library-owned stream holds HIP work only when the library put it
    // there: a copy, a fallback launch -- tracked per stream; nothing pending = nothing to ask HIP about)
    hipError_t e = hipSuccess;
    const bool owned_idle = seq_stream_is_owned(s) && !eager_hip_pending(q->device, s);
    if (!owned_idle) {
        e = hipStreamQuery(s);
        if (e == hipErrorNotReady) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_error(e, "smr_seq_run: draining the caller's stream");
        eager_hip_drained(q->device, s);
    }
    int rc = seq_submit(q, d, reps);
    if (rc) return rc;
    q->inflight = true;
    q->held = false;
    ++q->runs;
    // ... and whatever is queued on `stream` afterwards comes last.  The call returns as soon as the doorbells are rung (the reference's
    // @spawn returns at once and `wait` is separate, src/mapreduce.jl:214-223); what keeps later work on `stream` behind the replay:
    //   * a library-owned stream (smr_stream_create): nothing -- all its work goes through this library, which waits for the replay
    //     before anything it submits or does on the stream (eager_submit, the fences in smr_api.cpp);
    //   * a HIP stream: hipStreamWaitValue64 on the completion signals where the device supports it ($SMR_SEQ_STREAM_WAIT=1),
    //     otherwise a one-wave holding kernel on the stream that polls the signals (k_seq_hold; bounded).
    // "async" = 0 restores the blocking call; smr_seq_wait is the host-side wait in every mode.
    const bool owned = seq_stream_is_owned(s);
    if (q->async_mode == 0) {
        rc = wait_all(d);
        q->inflight = false;
        return rc;
    }
    if (owned) return SMR_OK;
    if (d.wait_value_ok) {
        e = hipSuccess;
        for (int k = 0; k < q->nq && e == hipSuccess; ++k)
            if (d.armed[k]) e = hipStreamWaitValue64(s, (void*)d.done_ptr[k], 0, hipStreamWaitValueEq, 0xFFFFFFFFFFFFFFFFull);
        if (e == hipSuccess) return SMR_OK;
        (void)hipGetLastError();
        d.wait_value_ok = false;
    }
    HoldBlock* hb = hold_block(d);
    int n = 0;
    if (hb)
        for (int k = 0; k < q->nq; ++k)
            if (d.armed[k] && d.done_ptr[k]) hb->sigs[n++] = (const volatile long long*)d.done_ptr[k];
    bool all_have_ptr = hb != nullptr;
    for (int k = 0; k < q->nq; ++k)
        if (d.armed[k] && !d.done_ptr[k]) all_have_ptr = false;
    if (all_have_ptr && n > 0) {
        (void)hipGetLastError();
        // 100 MHz device clock: the kernel's own limit in ticks -- a backstop far above the host's no-progress limit (a host that
        // declares the path failed zeroes the signals, which releases the kernel: direct_fail)
        const unsigned long long limit = (unsigned long long)(std::max(direct_timeout_s() * 20.0, 600.0) * 1e8);
        hipLaunchKernelGGL(k_seq_hold, dim3(1), dim3(64), 0, s, (const volatile long long* const*)hb->sigs, n, limit, hb->gave_up);
        if (hipGetLastError() == hipSuccess) {
            q->held = true;
            return SMR_OK;
        }
    }
    rc = wait_all(d);  // no way to hold the stream back: block here
    q->inflight = false;
    return rc;
}

int smr_seq_wait(smr_seq* q) {
    if (!q) return set_error(SMR_EINVAL, "null sequence");
    if (!q->aql || !q->inflight) return SMR_OK;
    Direct& d = direct_of(q->device);
    int rc;
    {
        std::lock_guard<std::mutex> g(d.mu);
        rc = wait_all(d);
    }
    q->inflight = false;
    if (rc == SMR_OK && q->held) {
        HoldBlock* hb = hold_block(d);
        if (hb && __atomic_load_n(hb->gave_up, __ATOMIC_RELAXED)) {
            __atomic_store_n(hb->gave_up, 0u, __ATOMIC_RELAXED);
            rc = set_error(SMR_EHIP, "smr_seq: the holding kernel on the caller's stream gave up before the replay completed");
        }
    }
    return rc;
}

int smr_seq_info(smr_seq* q, char* buf, size_t buflen) {
    if (!q || !buf || !buflen) return set_error(SMR_EINVAL, "null argument");
    if (!q->built) {
        int rc = seq_build(q);
        if (rc) return rc;
    }
    int ngroups = 0;
    for (const SeqItem& it : q->items) ngroups += it.group != nullptr;
    if (q->aql) {
        const Direct& d = direct_of(q->device);
        size_t np = 0;
        for (const auto& v : q->packets) np += v.size();
        const int first = q->acq_first >= 0 ? q->acq_first : q->acq_first_auto;
        std::snprintf(buf, buflen, "backend=aql items=%zu groups=%d packets=%zu components=%d sliced=%d queues=%d ordered=%d unordered=%d acquire=%s(%d of %zu packets) first_acquire=%s release=%d self_released=%d kernarg_layout=%s agent=%s stream_wait=%s last_replay_us=%.3f",
                      q->items.size(), ngroups, np, q->ncomp, q->nsliced, q->nq, q->n_barrier, q->n_any, q->acq_mid < 0 ? "by-need" : (q->acq_mid == 0 ? "none" : (q->acq_mid == 1 ? "agent" : "system")),
                      q->n_acquire, np, first == 2 ? "system" : (first == 1 ? "agent" : "none"), q->rel_mid, q->n_self_released, layout_source(d), d.agent_by_pci ? "pci-address" : "only-gpu",
                      q->async_mode == 0 ? "host(blocking)" : (d.wait_value_ok ? "hipStreamWaitValue64" : "holding-kernel|owned-stream"), d.last_us);
    }
    else
        std::snprintf(buf, buflen, "backend=hip items=%zu groups=%d (%s)", q->items.size(), ngroups, q->why_not_aql.c_str());
    return SMR_OK;
}

// Host-only view of the dependency analysis (no device needed: footprints are arithmetic on the plans' strides and base pointers):
// comp[i] = dependency component of recorded execution i.  Returns the number of components, or a negative status.
int smr_seq_components(smr_seq* q, int32_t* comp, size_t cap) {
    if (!q) return set_error(SMR_EINVAL, "null sequence");
    const Schedule sc = schedule(seq_footprints(q), seq_knobs(q));
    if (comp)
        for (size_t i = 0; i < sc.comp.size() && i < cap; ++i) comp[i] = sc.comp[i];
    return sc.ncomp;
}

// Host-only view of the fence analysis (no device needed): acquire[i] = 1 when recorded execution i reads bytes some execution of the
// sequence writes (its packets acquire inside a replay; all others do not), *footprint = bytes of the union of every range the
// sequence touches, *cache_resident = 1 when that is within "self_release_max_total" (launches may then be self-released).
int smr_seq_fences(smr_seq* q, int32_t* acquire, size_t cap, int64_t* footprint, int32_t* cache_resident) {
    if (!q) return set_error(SMR_EINVAL, "null sequence");
    const Schedule sc = schedule(seq_footprints(q), seq_knobs(q));
    if (acquire)
        for (size_t i = 0; i < sc.acquire.size() && i < cap; ++i) acquire[i] = sc.acquire[i];
    if (footprint) *footprint = sc.footprint_bytes;
    if (cache_resident) *cache_resident = sc.cache_resident ? 1 : 0;
    return (int)sc.acquire.size();
}

// Host-only view of the whole scheduler on synthetic executions (tests/test_seq_schedule.py); the layout is in include/strided_hip.h.
int smr_debug_seq_schedule(int nexec, const int32_t* nspans, const int64_t* spans, const int32_t* launches, const int64_t* knobs, const int32_t* comp_slices,
                           int32_t* per_exec, int32_t* totals, int64_t* footprint, int32_t* packets, int packet_cap) {
    if (nexec < 0 || !nspans || !spans || !launches || !knobs) return set_error(SMR_EINVAL, "smr_debug_seq_schedule: null argument");
    std::vector<SchedExec> ex((size_t)nexec);
    for (int i = 0; i < nexec; ++i) {
        for (int k = 0; k < nspans[2 * i] + nspans[2 * i + 1]; ++k, spans += 2)
            (k < nspans[2 * i] ? ex[i].rd : ex[i].wr).push_back({(uintptr_t)spans[0], (uintptr_t)spans[1]});
        const int32_t* l = launches + 5 * i;
        ex[i].nlaunch = l[0];
        ex[i].grid = (unsigned)l[1];
        ex[i].sliceable = l[2] != 0;
        ex[i].fold_after = (l[2] & 2) != 0;  // (bit 1: a two-launch execution whose second launch folds the whole first one)
        ex[i].all_self = l[3] != 0;
        ex[i].same_as = l[4];
    }
    SchedKnobs kn;
    kn.max_queues = (int)knobs[0];
    kn.slices = (int)knobs[1];
    kn.all_ordered = knobs[2] != 0;
    kn.self_release_max_total = knobs[3];
    for (int64_t c = 0; comp_slices && c < knobs[4]; ++c) kn.comp_slices[comp_slices[2 * c]] = comp_slices[2 * c + 1];
    const Schedule sc = schedule(ex, kn);
    for (int i = 0; per_exec && i < nexec; ++i) {
        const int32_t row[4] = {sc.comp[i], sc.acquire[i], sc.queue[i], sc.nslices[i]};
        std::memcpy(per_exec + 4 * i, row, sizeof row);
    }
    if (totals) {
        totals[0] = sc.ncomp;
        totals[1] = sc.nsliced;
        totals[2] = sc.nq;
        totals[3] = sc.cache_resident ? 1 : 0;
    }
    if (footprint) *footprint = sc.footprint_bytes;
    int n = 0;
    for (int k = 0; k < sc.nq; ++k)
        for (const SchedEntry& e : sc.queues[k]) {
            if (packets && n < packet_cap) {
                const int32_t row[8] = {k, e.exec, e.launch, e.slice, (int32_t)e.lo, (int32_t)e.hi, e.barrier ? 1 : 0, e.acquire ? 1 : 0};
                std::memcpy(packets + 8 * n, row, sizeof row);
            }
            ++n;
        }
    return n;
}

int smr_seq_set(smr_seq* q, const char* name, int64_t value) {
    if (!q || !name) return set_error(SMR_EINVAL, "null argument");
    // {name, member, lo, hi, rebuilds}: a setting that changes the packets ("rebuilds") is refused while a replay is in flight
    static const struct {
        const char* name;
        int smr_seq::*member;
        int lo, hi;
        bool rebuilds;
    } table[] = {
        {"acquire", &smr_seq::acq_mid, -1, 2, false},
        {"release", &smr_seq::rel_mid, 0, 2, false},
        {"release_self", &smr_seq::rel_self, 0, 1, false},
        {"first_acquire", &smr_seq::acq_first, -1, 2, false},
        {"last_release", &smr_seq::rel_last, 0, 2, false},
        {"async", &smr_seq::async_mode, -1, 1, false},
        {"queues", &smr_seq::max_queues, 1, SEQ_MAXQ, true},  // hardware queues a replay may spread over
    };
    if (std::strcmp(name, "fence_scope") == 0 && value >= 0 && value <= 2) {  // both fences of every inner packet at one scope
        q->acq_mid = q->rel_mid = (int)value;
        return SMR_OK;
    }
    for (const auto& t : table)
        if (std::strcmp(name, t.name) == 0 && value >= t.lo && value <= t.hi && !(t.rebuilds && q->inflight)) {
            q->*t.member = (int)value;
            if (t.rebuilds) q->built = false;
            return SMR_OK;
        }
    if (q->inflight) return set_error(SMR_EINVAL, "smr_seq_set: a replay is in flight (smr_seq_wait first)");
    if (std::strcmp(name, "order") == 0) {  // experiments: 0 = every packet ordered, 1 = dependency-aware (default)
        q->all_ordered = value == 0;
        q->built = false;
        return SMR_OK;
    }
    if (std::strcmp(name, "slices") == 0 && (value == -1 || (value >= 1 && value <= SEQ_MAXQ))) {  // block ranges per single-launch component (-1: automatic)
        q->slices = (int)value;
        q->comp_slices.clear();
        q->built = false;
        return SMR_OK;
    }
    if (std::strncmp(name, "slices:", 7) == 0 && value >= 1 && value <= SEQ_MAXQ) {  // ... of component <c> alone (numbered by first appearance)
        char* end = nullptr;
        const long c = std::strtol(name + 7, &end, 10);
        if (end == name + 7 || *end || c < 0 || c > 4096) return set_error(SMR_EINVAL, "smr_seq_set: slices:<component>");
        q->comp_slices[(int)c] = (int)value;
        q->built = false;
        return SMR_OK;
    }
    return set_error(SMR_EINVAL, "smr_seq_set: unknown name");
}

int smr_seq_destroy(smr_seq* q) {
    if (!q) return SMR_OK;
    (void)smr_seq_wait(q);
    if (q->d_kernargs) (void)hipFree(q->d_kernargs);
    delete q;
    return SMR_OK;
}

}  // extern "C"
