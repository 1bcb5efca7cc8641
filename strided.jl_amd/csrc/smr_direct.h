// smr_direct.h -- direct dispatch: the HSA runtime HIP already loaded, the per-device hardware queues of the library's own, kernel
// descriptors and kernarg layouts from the code objects HIP loaded, hand-built AQL packets and bounded waits (smr_direct.cpp).  Shared by
// eager dispatch on library-owned streams (smr_eager.cpp) and recorded sequences (smr_seq.cpp); internal to those three files.
#pragma once
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <hsa/hsa_ven_amd_loader.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "smr_internal.h"
#include "smr_kmeta.h"
#include "smr_sched.h"

namespace smr {

// smr_api.cpp
int seq_execute_plan(smr_plan* plan, void* const* bases, hipStream_t s, bool prepare_only);
void seq_footprint(smr_plan* plan, void* const* bases, std::vector<std::pair<uintptr_t, uintptr_t>>& rd, std::vector<std::pair<uintptr_t, uintptr_t>>& wr);
int seq_nops(smr_plan* plan);
// smr_group.cpp: a recorded group execution (one launch; the footprint is the merged byte ranges of all members, kept by the planner)
int seq_execute_group(smr_group* group, hipStream_t s, bool prepare_only);
void seq_footprint_group(smr_group* group, Spans& rd, Spans& wr);
bool seq_stream_is_owned(hipStream_t s);

// ---- the HSA runtime HIP already loaded (never a second copy) ------------------------------------------------------------------
struct Hsa {
    void* lib = nullptr;
    decltype(&hsa_init) init = nullptr;
    decltype(&hsa_iterate_agents) iterate_agents = nullptr;
    decltype(&hsa_agent_get_info) agent_get_info = nullptr;
    decltype(&hsa_queue_create) queue_create = nullptr;
    decltype(&hsa_queue_destroy) queue_destroy = nullptr;
    decltype(&hsa_queue_load_read_index_scacquire) load_read_index = nullptr;
    decltype(&hsa_queue_add_write_index_relaxed) add_write_index = nullptr;
    decltype(&hsa_signal_create) signal_create = nullptr;
    decltype(&hsa_signal_destroy) signal_destroy = nullptr;
    decltype(&hsa_signal_store_relaxed) signal_store_relaxed = nullptr;
    decltype(&hsa_signal_store_screlease) signal_store_screlease = nullptr;
    decltype(&hsa_signal_load_scacquire) signal_load = nullptr;
    decltype(&hsa_signal_wait_scacquire) signal_wait = nullptr;
    decltype(&hsa_amd_signal_value_pointer) signal_value_pointer = nullptr;
    decltype(&hsa_system_get_major_extension_table) get_ext_table = nullptr;
    decltype(&hsa_executable_get_symbol_by_name) get_symbol_by_name = nullptr;
    decltype(&hsa_executable_symbol_get_info) symbol_get_info = nullptr;
    decltype(&hsa_status_string) status_string = nullptr;
    // optional (eager dispatch): signals without an interrupt, argument blocks in device memory written through the BAR
    decltype(&hsa_amd_signal_create) amd_signal_create = nullptr;
    decltype(&hsa_amd_agent_iterate_memory_pools) iterate_pools = nullptr;
    decltype(&hsa_amd_memory_pool_get_info) pool_get_info = nullptr;
    decltype(&hsa_amd_agent_memory_pool_get_info) agent_pool_get_info = nullptr;
    decltype(&hsa_amd_memory_pool_allocate) pool_allocate = nullptr;
    decltype(&hsa_amd_agents_allow_access) allow_access = nullptr;
    hsa_ven_amd_loader_1_03_pfn_t loader;
    bool ok = false;
    std::string why;
};
Hsa& hsa();

// ---- per-device direct queue --------------------------------------------------------------------------------------------------
constexpr int SEQ_MAXQ = 8;
struct KernelRef {
    uint64_t object = 0;
    uint32_t kernarg_size = 0, group_static = 0, private_size = 0;
    std::string name;
    KernargLayout layout;        // where the hidden arguments live: from the code object's metadata, else the code-object-v5 rule
    bool from_metadata = false;
};
struct Direct {
    int dev = 0;
    hsa_agent_t agent{};
    // A queue error (the HSA callback) or a wait that ran out of time marks the device's direct path as failed: every wait returns,
    // the call that noticed returns SMR_EHIP, and later executions go through HIP (direct().ok is false from then on).
    std::atomic<bool> failed{false};
    std::string fail_why;
    std::mutex why_mu;                  // guards `why` / `fail_why` (written by whichever thread sees the failure, read by smr_seq_info and the planners of other threads: ADVICE r5)
    // kernarg layouts by code object (storage base address of the loaded image) and kernel-descriptor symbol
    std::map<uint64_t, std::map<std::string, KernargLayout>> code_objects;
    int n_meta = 0, n_v5 = 0;    // kernels resolved with a layout from metadata / from the v5 rule
    bool agent_by_pci = false;   // the HSA agent was found by the HIP device's PCI address (false: the only GPU agent there is)
    bool probe_ok = false;       // the self-test launch saw the blockDim / gridDim / LDS it was given
    bool probe_meta = false;     // ... with a layout read from metadata
    // SEQ_MAXQ hardware queues of the library's own (created on first use): launches that belong to different dependency
    // components of a sequence go to different queues, where neither the barrier bit nor the acquire / release fences of one
    // chain hold up the other (inside ONE queue the packet processor serialises consecutive dispatches on their fences even
    // when the barrier bit is clear: profiles/r04_overlap.txt)
    hsa_queue_t* q[SEQ_MAXQ] = {};
    hsa_signal_t done[SEQ_MAXQ] = {};   // completion signal of the last packet a replay put on queue k
    volatile int64_t* done_ptr[SEQ_MAXQ] = {};
    bool armed[SEQ_MAXQ] = {};          // done[k] belongs to a replay nobody waited for yet
    double t_submit = 0, last_us = 0;   // host clock at the first doorbell of the replay in flight; doorbell -> completion observed
    std::mutex mu;                      // one replay is written at a time
    std::map<const void*, KernelRef> kernels;
    bool wait_value_ok = false;
    bool ok = false;
    std::string why;
};

double now_s();
double direct_timeout_s();
void direct_fail(Direct& d, const std::string& why);
bool wait_signal(Direct& d, hsa_signal_t sig);
int wait_all(Direct& d);
int direct_queue(Direct& d, int k);
int current_device();
int device_of(hipStream_t s);
Direct& direct_of(int dev);
Direct& direct();
std::vector<int> direct_devices();  // the devices whose direct path was asked for so far (nothing is created)
int resolve_name(Direct& d, const std::string& name, KernelRef& out);
int resolve_kernel(Direct& d, const void* hostfn, KernelRef& out);
bool kernarg_layout_of(const KernelRef& k, size_t explicit_bytes, KernargLayout& L);
bool resolve_launch(Direct& d, const RecLaunch& l, KernelRef& k, std::string* why);
void fill_kernarg_image(const KernelRef& k, const RecLaunch& l, unsigned grid_blocks, unsigned char* dst, size_t dst_bytes);
hsa_kernel_dispatch_packet_t dispatch_packet(const KernelRef& k, unsigned grid_blocks, unsigned block, size_t lds, void* kernargs);
uint16_t header_of(bool barrier, int acq, int rel);
uint16_t barrier_header(int acq, int rel);
bool put_packet(Direct& d, hsa_queue_t* hq, const void* body64, uint16_t header, uint16_t setup);
const char* layout_source(const Direct& d);

// smr_eager.cpp, for smr_seq_run (the caller holds d.mu): has the library queued HIP work on owned stream s since its last drain / it was drained
bool eager_hip_pending(int dev, hipStream_t s);
void eager_hip_drained(int dev, hipStream_t s);

}  // namespace smr
