// smr_sched.h -- the replay scheduler of recorded sequences (smr_seq.cpp) as one pure function: byte ranges and a few facts per launch
// in; components, queues, block-range slices, barrier bits and acquire flags out.  Plain host C++ (no HIP, no HSA, no options()): the
// sequence builder, the host-only views smr_seq_components / smr_seq_fences and the CPU test (smr_debug_seq_schedule) all run this code.
#pragma once
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace smr {

typedef std::vector<std::pair<uintptr_t, uintptr_t>> Spans;  // byte ranges [first, second)
bool overlaps(const Spans& v, const std::pair<uintptr_t, uintptr_t>& x);
bool overlaps(const Spans& v, const Spans& w);

// one recorded execution of a plan
struct SchedExec {
    Spans rd, wr;             // the bytes it reads / writes (footprint() in smr_api.cpp)
    int nlaunch = 0;          // launches it recorded (0: footprints only -- enough for comp, acquire and the footprint)
    unsigned grid = 0;        // workgroups of its first launch
    bool sliceable = false;   // the first launch's workgroups are independent (RecLaunch::slice_kind != 0)
    bool all_self = false;    // every launch of it is self-released
    int same_as = 0;          // index of the first execution with the same plan and the same base pointers, else its own index
    bool fold_after = false;  // nlaunch == 2 and the second launch only needs the WHOLE first one to have completed (a split contraction
                              // group: partials, then the fold): the first launch may be cut into block ranges on the item's own queue
};
struct SchedKnobs {
    int max_queues = 4;               // hardware queues a replay may spread over (>= 1)
    int slices = -1;                  // block ranges per single-launch component: -1 automatic, 1 never
    std::map<int, int> comp_slices;   // ... of component c alone
    bool all_ordered = false;         // every packet carries the barrier bit
    int64_t self_release_max_total = 0;  // option "self_release_max_total": cache_resident = footprint_bytes <= this
};
// one packet of a replay.  [lo, hi) = its workgroups: the slice's block range when the launch is cut, else the whole launch -- known
// to the scheduler for launch 0 only (hi = SchedExec::grid); a later launch of an execution is never cut and has lo = hi = 0.
// A `fold_after` execution that is cut has its ranges back to back on ONE queue (the first with the execution's barrier bit, the
// others free: the packet processor takes packets in order, so none starts before the first was let through) and then its second
// launch with the barrier bit: it starts when every range has completed.  No order across queues is needed for it.
struct SchedEntry {
    int exec, launch, slice;
    unsigned lo, hi;
    bool barrier, acquire;
};
struct Schedule {
    std::vector<int> comp, acquire, queue, nslices;  // per execution: component, reads what the sequence writes, first queue, slices
    std::vector<int> same_queue;   // per execution: 1 = its slices are block ranges on ONE queue (a cut `fold_after` execution)
    int ncomp = 0, nsliced = 0, nq = 0;
    int64_t footprint_bytes = 0;   // union of every range the sequence touches
    bool cache_resident = false;
    std::vector<std::vector<SchedEntry>> queues;  // nq lists, in submission order, empty slices dropped
};

int components_of(const std::vector<Spans>& rd, const std::vector<Spans>& wr, std::vector<int>& comp);
void slice_range(unsigned grid, int ns, int s, unsigned& lo, unsigned& hi);
Schedule schedule(const std::vector<SchedExec>& ex, const SchedKnobs& knobs);

}  // namespace smr
