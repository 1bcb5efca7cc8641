// smr_direct.cpp -- direct dispatch (smr_direct.h): the library submits hand-built AQL packets on HSA queues of its own.
//
// Kernel objects come from the code objects HIP itself has loaded: host stub -> kernel name (hipKernelNameRefByPtr) -> "<name>.kd" looked
// up in the process's HSA executables (loader extension 1.03: hsa_ven_amd_loader_iterate_executables).  Nothing is loaded twice.
// One probe packet goes through queue 0 before anything depends on the path (direct_selftest); every wait is bounded.  Also here: the
// thread-local recorder the launchers append to while a sequence records or an eager call collects its launches.
#include <dlfcn.h>
#include <link.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "smr_direct.h"

namespace smr {

static thread_local std::vector<RecLaunch>* tl_recorder = nullptr;
std::vector<RecLaunch>* recorder() { return tl_recorder; }
static thread_local bool tl_rec_seq = false, tl_self_released = false;
static thread_local bool tl_rec_eager = false;  // the recorder belongs to an eager call: `allow` was decided by the eager option, not the sequence's
void set_recorder(std::vector<RecLaunch>* r, bool allow_self_release, bool eager) {
    tl_recorder = r;
    tl_rec_seq = r != nullptr && allow_self_release;
    tl_rec_eager = r != nullptr && eager;
}
void mark_self_released() {
    if (tl_recorder) tl_self_released = true;
}
bool want_self_release(const Plan& plan) {
    if (!tl_recorder || !tl_rec_seq) return false;
    const Options& o = options();
    // the two knobs are independent: a sequence asks seq_self_release, an eager call was admitted by eager_self_release
    if (!(tl_rec_eager ? o.eager_self_release : o.seq_self_release)) return false;
    const Canon& c = plan.c;
    i64 lo = 0, hi = 0;  // extent of the destination in elements
    for (int d = 0; d < c.N; ++d) {
        const i64 ext = (c.dims[d] - 1) * c.strides[0][d];
        (ext < 0 ? lo : hi) += ext;
    }
    return (hi - lo + 1) * (i64)c.esize[0] <= o.self_release_max_bytes;
}
static thread_local int tl_slice_kind = 0;
static thread_local unsigned tl_slice_off = 0, tl_slice_row = 0;
void mark_sliceable(int kind, unsigned off, unsigned row) {
    if (!tl_recorder) return;
    tl_slice_kind = kind;
    tl_slice_off = off;
    tl_slice_row = row;
}
void take_slice_mark(RecLaunch& r) {
    r.slice_kind = tl_slice_kind;
    r.slice_off = tl_slice_off;
    r.slice_row = tl_slice_row;
    tl_slice_kind = 0;
    r.self_released = tl_self_released;
    tl_self_released = false;
}

namespace {
int find_hsa(struct dl_phdr_info* info, size_t, void* data) {
    if (info->dlpi_name && std::strstr(info->dlpi_name, "libhsa-runtime64")) {
        *(std::string*)data = info->dlpi_name;
        return 1;
    }
    return 0;
}
}  // namespace

Hsa& hsa() {
    static Hsa* h = [] {
        Hsa* x = new Hsa();
        // A profiler (rocprofv3, HSA_TOOLS_LIB) intercepts queue creation and hands out proxy queues whose rings are not meant to be
        // written by the application directly (measured: rocprofv3 --kernel-trace crashes inside the first ring write).  Under such a
        // tool -- or with SMR_SEQ_DIRECT=0 -- sequences replay through HIP, in recorded order, and the profiler sees ordinary launches.
        {
            const char* force = std::getenv("SMR_SEQ_DIRECT");
            bool tool = false;
            for (const char* v : {"HSA_TOOLS_LIB", "ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_FORCE_LOAD", "ROCPROF_OUTPUT_PATH"})
                if (const char* e = std::getenv(v)) tool = tool || *e;
            if (const char* e = std::getenv("LD_PRELOAD")) tool = tool || std::strstr(e, "rocprof") != nullptr;
            if ((force && force[0] == '0') || (tool && !(force && force[0] == '1'))) {
                x->why = force && force[0] == '0' ? "SMR_SEQ_DIRECT=0" : "an HSA tools library (profiler) intercepts the queues";
                return x;
            }
        }
        std::string path;
        dl_iterate_phdr(find_hsa, &path);
        if (path.empty()) {
            x->why = "libhsa-runtime64 is not loaded in this process (HIP not initialised?)";
            return x;
        }
        x->lib = dlopen(path.c_str(), RTLD_NOW | RTLD_NOLOAD);
        if (!x->lib) {
            x->why = std::string("dlopen(RTLD_NOLOAD) of ") + path + " failed";
            return x;
        }
        bool all = true;
#define SMR_HSA_SYM(field, name)                                   \
    x->field = (decltype(x->field))dlsym(x->lib, #name);            \
    if (!x->field) {                                                \
        all = false;                                                \
        x->why += std::string(" missing ") + #name;                 \
    }
        SMR_HSA_SYM(init, hsa_init)
        SMR_HSA_SYM(iterate_agents, hsa_iterate_agents)
        SMR_HSA_SYM(agent_get_info, hsa_agent_get_info)
        SMR_HSA_SYM(queue_create, hsa_queue_create)
        SMR_HSA_SYM(queue_destroy, hsa_queue_destroy)
        SMR_HSA_SYM(load_read_index, hsa_queue_load_read_index_scacquire)
        SMR_HSA_SYM(add_write_index, hsa_queue_add_write_index_relaxed)
        SMR_HSA_SYM(signal_create, hsa_signal_create)
        SMR_HSA_SYM(signal_destroy, hsa_signal_destroy)
        SMR_HSA_SYM(signal_store_relaxed, hsa_signal_store_relaxed)
        SMR_HSA_SYM(signal_store_screlease, hsa_signal_store_screlease)
        SMR_HSA_SYM(signal_load, hsa_signal_load_scacquire)
        SMR_HSA_SYM(signal_wait, hsa_signal_wait_scacquire)
        SMR_HSA_SYM(signal_value_pointer, hsa_amd_signal_value_pointer)
        SMR_HSA_SYM(get_ext_table, hsa_system_get_major_extension_table)
        SMR_HSA_SYM(get_symbol_by_name, hsa_executable_get_symbol_by_name)
        SMR_HSA_SYM(symbol_get_info, hsa_executable_symbol_get_info)
        SMR_HSA_SYM(status_string, hsa_status_string)
#undef SMR_HSA_SYM
        x->amd_signal_create = (decltype(x->amd_signal_create))dlsym(x->lib, "hsa_amd_signal_create");
        x->iterate_pools = (decltype(x->iterate_pools))dlsym(x->lib, "hsa_amd_agent_iterate_memory_pools");
        x->pool_get_info = (decltype(x->pool_get_info))dlsym(x->lib, "hsa_amd_memory_pool_get_info");
        x->agent_pool_get_info = (decltype(x->agent_pool_get_info))dlsym(x->lib, "hsa_amd_agent_memory_pool_get_info");
        x->pool_allocate = (decltype(x->pool_allocate))dlsym(x->lib, "hsa_amd_memory_pool_allocate");
        x->allow_access = (decltype(x->allow_access))dlsym(x->lib, "hsa_amd_agents_allow_access");
        if (!all) return x;
        if (x->init() != HSA_STATUS_SUCCESS) {  // reference-counted: HIP holds the first reference
            x->why = "hsa_init failed";
            return x;
        }
        std::memset(&x->loader, 0, sizeof x->loader);
        if (x->get_ext_table(HSA_EXTENSION_AMD_LOADER, 1, sizeof x->loader, &x->loader) != HSA_STATUS_SUCCESS ||
            !x->loader.hsa_ven_amd_loader_iterate_executables) {
            x->why = "HSA loader extension 1.03 (iterate_executables) is unavailable";
            return x;
        }
        x->ok = true;
        return x;
    }();
    return *h;
}

namespace {
struct AgentPick {
    Hsa* h;
    uint32_t bdf, domain;
    hsa_agent_t found{};
    bool have = false;
    hsa_agent_t first{};
    int ngpu = 0;
};
hsa_status_t pick_agent(hsa_agent_t a, void* data) {
    AgentPick* p = (AgentPick*)data;
    hsa_device_type_t t;
    if (p->h->agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
    if (p->ngpu++ == 0) p->first = a;
    uint32_t bdf = 0, dom = 0;
    p->h->agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf);
    p->h->agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom);
    if (bdf == p->bdf && dom == p->domain) {
        p->found = a;
        p->have = true;
    }
    return HSA_STATUS_SUCCESS;
}

void queue_error(hsa_status_t st, hsa_queue_t*, void* data) {
    std::fprintf(stderr, "libstrided_hip: the direct-dispatch HSA queue reported error 0x%x; direct dispatch is switched off\n", (unsigned)st);
    if (Direct* d = (Direct*)data) d->failed.store(true);
}
}  // namespace

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// how long a wait on the direct queues may last before the path is declared dead ($SMR_DIRECT_TIMEOUT_MS, default 30 s: far above
// any replay this library issues, far below "forever")
double direct_timeout_s() {
    static const double t = [] {
        const char* e = std::getenv("SMR_DIRECT_TIMEOUT_MS");
        const double ms = e ? std::atof(e) : 0;
        return ms > 0 ? ms * 1e-3 : 30.0;
    }();
    return t;
}

void direct_fail(Direct& d, const std::string& why) {
    std::string msg;
    {
        std::lock_guard<std::mutex> g(d.why_mu);
        const bool first = !d.failed.exchange(true) || d.fail_why.empty();
        if (first) d.fail_why = why;
        d.ok = false;
        d.why = "direct dispatch failed earlier: " + d.fail_why;
        msg = d.fail_why;
    }
    // a holding kernel on some HIP stream may be polling the replay's completion signals (asynchronous smr_seq_run): let it go
    for (int k = 0; k < SEQ_MAXQ; ++k)
        if (d.q[k] && d.done_ptr[k]) hsa().signal_store_relaxed(d.done[k], 0);
    set_error(SMR_EHIP, "direct dispatch: " + msg);
}

// Bounded wait for a completion signal.  false: the queue reported an error or NOTHING MOVED for the time limit -- the device's
// direct path is marked failed (the caller unwinds; nothing waits on these queues again).  The limit is on the absence of progress,
// not on the wait: a replay of a million launches is allowed to take its time, the clock restarts whenever any of the device's
// queues has consumed packets since the last look.
bool wait_signal(Direct& d, hsa_signal_t sig) {
    Hsa& h = hsa();
    if (h.signal_load(sig) == 0) return true;
    if (d.failed.load()) {
        direct_fail(d, "the HSA queue reported an error");
        return false;
    }
    double t0 = now_s();
    const double limit = direct_timeout_s();
    uint64_t seen[SEQ_MAXQ] = {};
    for (int k = 0; k < SEQ_MAXQ; ++k)
        if (d.q[k]) seen[k] = h.load_read_index(d.q[k]);
    for (;;) {
        // timeout hint in timestamp ticks (100 MHz on this part: ~2 ms per slice)
        if (h.signal_wait(sig, HSA_SIGNAL_CONDITION_EQ, 0, 200000, HSA_WAIT_STATE_ACTIVE) == 0) return true;
        if (d.failed.load()) {
            direct_fail(d, "the HSA queue reported an error");
            return false;
        }
        for (int k = 0; k < SEQ_MAXQ; ++k)
            if (d.q[k]) {
                const uint64_t r = h.load_read_index(d.q[k]);
                if (r != seen[k]) {
                    seen[k] = r;
                    t0 = now_s();
                }
            }
        if (now_s() - t0 > limit) {
            direct_fail(d, "no hardware queue made progress and the completion signal did not arrive within the time limit ($SMR_DIRECT_TIMEOUT_MS)");
            return false;
        }
    }
}

static std::mutex g_direct_mu;
static std::map<int, Direct*> g_direct;
std::vector<int> direct_devices() {
    std::lock_guard<std::mutex> g(g_direct_mu);
    std::vector<int> devs;
    for (auto& kv : g_direct) devs.push_back(kv.first);
    return devs;
}

// queue k of the device (created on first use)
int direct_queue(Direct& d, int k) {
    if (d.q[k]) return SMR_OK;
    Hsa& h = hsa();
    hsa_status_t st = h.queue_create(d.agent, 16384, HSA_QUEUE_TYPE_SINGLE, queue_error, &d, UINT32_MAX, UINT32_MAX, &d.q[k]);
    if (st != HSA_STATUS_SUCCESS) {
        d.q[k] = nullptr;
        d.why = "hsa_queue_create failed";
        return set_error(SMR_EHIP, d.why);
    }
    if (h.signal_create(0, 0, nullptr, &d.done[k]) != HSA_STATUS_SUCCESS) {
        d.why = "hsa_signal_create failed";
        return set_error(SMR_EHIP, d.why);
    }
    volatile hsa_signal_value_t* vp = nullptr;
    if (h.signal_value_pointer(d.done[k], &vp) == HSA_STATUS_SUCCESS) d.done_ptr[k] = (volatile int64_t*)vp;
    return SMR_OK;
}

int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev;
}
// the device a stream belongs to (not the calling thread's current device: a process that drives several GPUs may submit to a
// stream of another one); the null stream belongs to the current device
int device_of(hipStream_t s) {
    if (s) {
        hipDevice_t dv = 0;
        if (hipStreamGetDevice(s, &dv) == hipSuccess) return (int)dv;
        (void)hipGetLastError();
    }
    return current_device();
}

namespace {
int direct_selftest(Direct& d);
}

Direct& direct_of(int dev) {
    std::lock_guard<std::mutex> g(g_direct_mu);
    auto it = g_direct.find(dev);
    if (it != g_direct.end()) return *it->second;
    Direct* d = new Direct();
    d->dev = dev;
    g_direct[dev] = d;
    Hsa& h = hsa();
    if (!h.ok) {
        d->why = h.why;
        return *d;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        d->why = "hipGetDeviceProperties failed";
        return *d;
    }
    AgentPick pick;
    pick.h = &h;
    pick.bdf = ((uint32_t)prop.pciBusID << 8) | ((uint32_t)prop.pciDeviceID << 3);
    pick.domain = (uint32_t)prop.pciDomainID;
    h.iterate_agents(pick_agent, &pick);
    if (!pick.have) {
        if (pick.ngpu == 1) {
            pick.found = pick.first;  // one GPU visible: nothing to confuse
        } else {
            d->why = "no HSA agent matches the HIP device's PCI address";
            return *d;
        }
    }
    d->agent = pick.found;
    d->agent_by_pci = pick.have;
    if (int rc = direct_queue(*d, 0)) {
        (void)rc;
        return *d;
    }
    int can = 0;
    // stream-side waits (hipStreamWaitValue64 on the completion signals) are opt-in ($SMR_SEQ_STREAM_WAIT=1): the MI355X boxes this was
    // developed on report hipDeviceAttributeCanUseStreamWaitValue = 0, so only the host-side wait has run on hardware
    const char* sw = std::getenv("SMR_SEQ_STREAM_WAIT");
    if (sw && sw[0] == '1' && hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, dev) == hipSuccess && can && d->done_ptr[0]) d->wait_value_ok = true;
    d->ok = true;
    // one packet through queue 0 before anything depends on the path: a probe kernel reports the blockDim / gridDim it sees and
    // writes through its dynamic LDS.  A wrong hidden-argument layout, a ring that is not ours to write, a signal that never
    // arrives -- all end here, with the path switched off and everything going through HIP.
    if (direct_selftest(*d) != SMR_OK) d->ok = false;
    return *d;
}
Direct& direct() { return direct_of(current_device()); }

namespace {
struct Lookup {
    Hsa* h;
    Direct* d;
    hsa_agent_t agent;
    std::string kd;
    KernelRef out;
    bool have = false;
};

// is [p, p + n) mapped in this process?  (the loader reports where the code object's image was when it was loaded; HIP keeps that
// memory for the life of the module, but a stale address must cost a fallback, not a fault)
bool range_mapped(const void* p, size_t n) {
    const long page = sysconf(_SC_PAGESIZE);
    if (page <= 0 || !p || !n) return false;
    const uintptr_t lo = (uintptr_t)p & ~(uintptr_t)(page - 1), hi = ((uintptr_t)p + n + (uintptr_t)page - 1) & ~(uintptr_t)(page - 1);
    std::vector<unsigned char> vec((hi - lo) / (uintptr_t)page);
    return mincore((void*)lo, hi - lo, vec.data()) == 0;
}

// the loaded code objects of the executable that holds the kernel: parse the metadata of each image once, look the kernel up
hsa_status_t scan_code_object(hsa_executable_t, hsa_loaded_code_object_t lco, void* data) {
    Lookup* l = (Lookup*)data;
    auto get = l->h->loader.hsa_ven_amd_loader_loaded_code_object_get_info;
    if (!get) return HSA_STATUS_INFO_BREAK;
    hsa_ven_amd_loader_code_object_storage_type_t st = HSA_VEN_AMD_LOADER_CODE_OBJECT_STORAGE_TYPE_NONE;
    if (get(lco, HSA_VEN_AMD_LOADER_LOADED_CODE_OBJECT_INFO_CODE_OBJECT_STORAGE_TYPE, &st) != HSA_STATUS_SUCCESS || st != HSA_VEN_AMD_LOADER_CODE_OBJECT_STORAGE_TYPE_MEMORY)
        return HSA_STATUS_SUCCESS;
    uint64_t base = 0, size = 0;
    if (get(lco, HSA_VEN_AMD_LOADER_LOADED_CODE_OBJECT_INFO_CODE_OBJECT_STORAGE_MEMORY_BASE, &base) != HSA_STATUS_SUCCESS ||
        get(lco, HSA_VEN_AMD_LOADER_LOADED_CODE_OBJECT_INFO_CODE_OBJECT_STORAGE_MEMORY_SIZE, &size) != HSA_STATUS_SUCCESS || !base || !size)
        return HSA_STATUS_SUCCESS;
    auto parse = [&] {
        std::map<std::string, KernargLayout> kernels;
        std::string why;
        if (range_mapped((const void*)base, (size_t)size)) (void)kmeta_parse((const void*)base, (size_t)size, kernels, why);
        return kernels;  // (an image that did not parse gives an empty entry)
    };
    auto it = l->d->code_objects.find(base);
    const bool cached = it != l->d->code_objects.end();
    if (!cached) it = l->d->code_objects.emplace(base, parse()).first;
    auto k = it->second.find(l->kd);
    if (k == it->second.end() && cached) {
        // The entry is keyed by the address of the image.  A runtime-compiled module that the JIT cache unloaded frees its image, and
        // the next one may be stored where it was: what was parsed then says nothing about the image that is there now.
        it->second = parse();
        k = it->second.find(l->kd);
    }
    if (k == it->second.end()) return HSA_STATUS_SUCCESS;
    l->out.layout = k->second;
    l->out.from_metadata = true;
    return HSA_STATUS_INFO_BREAK;
}

hsa_status_t lookup_exec(hsa_executable_t ex, void* data) {
    Lookup* l = (Lookup*)data;
    hsa_executable_symbol_t sym;
    if (l->h->get_symbol_by_name(ex, l->kd.c_str(), &l->agent, &sym) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    hsa_symbol_kind_t kind;
    if (l->h->symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_TYPE, &kind) != HSA_STATUS_SUCCESS || kind != HSA_SYMBOL_KIND_KERNEL) return HSA_STATUS_SUCCESS;
    l->h->symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &l->out.object);
    l->h->symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &l->out.kernarg_size);
    l->h->symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &l->out.group_static);
    l->h->symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &l->out.private_size);
    l->have = true;
    // the hidden-argument layout, from the metadata of the code object this executable was loaded from
    const char* off = std::getenv("SMR_DIRECT_METADATA");
    if (!(off && off[0] == '0') && l->h->loader.hsa_ven_amd_loader_executable_iterate_loaded_code_objects)
        (void)l->h->loader.hsa_ven_amd_loader_executable_iterate_loaded_code_objects(ex, scan_code_object, l);
    return HSA_STATUS_INFO_BREAK;
}
}  // namespace

// kernel name -> kernel descriptor among the executables loaded in this process
int resolve_name(Direct& d, const std::string& name, KernelRef& out) {
    Lookup l;
    l.h = &hsa();
    l.d = &d;
    l.agent = d.agent;
    l.kd = name + ".kd";
    l.h->loader.hsa_ven_amd_loader_iterate_executables(lookup_exec, &l);
    if (!l.have) return set_error(SMR_EUNSUPPORTED, std::string("direct dispatch: kernel descriptor not found for ") + name);
    l.out.name = name;
    if (l.out.from_metadata) {
        // the runtime's view of the kernel and the metadata's must agree, and nothing only HIP could supply may be asked for
        if ((uint32_t)l.out.layout.kernarg_size != l.out.kernarg_size)
            return set_error(SMR_EUNSUPPORTED, "direct dispatch: kernarg size of " + name + " differs between the loader and the code object's metadata");
        if (l.out.layout.needs_runtime) return set_error(SMR_EUNSUPPORTED, "direct dispatch: " + name + " declares hidden arguments only the HIP runtime can supply");
        ++d.n_meta;
    } else {
        ++d.n_v5;  // layout by the code-object-v5 rule once the explicit size is known (kernarg_layout_of); trusted only because the self-test passed with it
    }
    out = l.out;
    return SMR_OK;
}

// The layout to fill for a launch whose explicit arguments occupy `explicit_bytes`: the metadata's when it was found -- and then the
// recorded explicit block must end where the metadata says the explicit arguments end -- else the code-object-v5 rule.
// false: this launch cannot be dispatched directly.
bool kernarg_layout_of(const KernelRef& k, size_t explicit_bytes, KernargLayout& L) {
    if (k.from_metadata) {
        // the recorder packs the explicit arguments the way the kernarg segment holds them: its block must cover every explicit
        // argument the metadata lists and must not reach into the first hidden field
        int32_t first_hidden = k.layout.kernarg_size;
        auto lower = [&](int32_t off) {
            if (off >= 0) first_hidden = std::min(first_hidden, off);
        };
        for (int d3 = 0; d3 < 3; ++d3) {
            lower(k.layout.block_count[d3]);
            lower(k.layout.group_size[d3]);
            lower(k.layout.remainder[d3]);
            lower(k.layout.global_offset[d3]);
        }
        lower(k.layout.grid_dims);
        lower(k.layout.dynamic_lds);
        if ((size_t)k.layout.explicit_end > explicit_bytes || explicit_bytes > (size_t)first_hidden) return false;
        L = k.layout;
        return true;
    }
    L = kmeta_v5_default(explicit_bytes, k.kernarg_size);
    return true;
}

// host stub -> kernel descriptor in the code object HIP has loaded
int resolve_kernel(Direct& d, const void* hostfn, KernelRef& out) {
    auto it = d.kernels.find(hostfn);
    if (it != d.kernels.end()) {
        out = it->second;
        return SMR_OK;
    }
    hipFuncAttributes attr;  // forces HIP to load the code object that holds the kernel (deferred loading)
    hipError_t e = hipFuncGetAttributes(&attr, hostfn);
    if (e != hipSuccess) return hip_error(e, "hipFuncGetAttributes (sequence build)");
    const char* name = hipKernelNameRefByPtr(hostfn, nullptr);
    if (!name || !*name) return set_error(SMR_EUNSUPPORTED, "direct dispatch: HIP does not know the kernel's name");
    const int rc = resolve_name(d, name, out);
    if (rc) return rc;
    d.kernels[hostfn] = out;
    return SMR_OK;
}

// Can this recorded launch go out as a hand-built packet?  Resolves the kernel by host stub or by name (unless the caller did: k.object
// is set), refuses scratch memory and an explicit argument block that does not match the kernarg layout.  false: *why says which.
bool resolve_launch(Direct& d, const RecLaunch& l, KernelRef& k, std::string* why) {
    std::string sink;
    std::string& w = why ? *why : sink;
    if (!l.hostfn && l.kname.empty()) {
        w = "a launch without a kernel identity takes part";
        return false;
    }
    if (!k.object && (l.hostfn ? resolve_kernel(d, l.hostfn, k) : resolve_name(d, l.kname, k)) != SMR_OK) {
        w = smr_last_error();
        return false;
    }
    if (k.private_size != 0) {
        w = "a kernel needs scratch memory: " + k.name;
        return false;
    }
    KernargLayout lay;
    if (!kernarg_layout_of(k, l.args.size(), lay)) {
        w = "the recorded arguments of " + k.name + " do not match the kernarg layout in its code object's metadata";
        return false;
    }
    return true;
}

// The kernarg block of a launch of `grid_blocks` workgroups into dst (zeroed by the caller): the explicit arguments, then the hidden
// ones (block counts, group sizes, grid dims, dynamic LDS size) at the offsets the code object's metadata names -- when the block is
// large enough to hold them.
void fill_kernarg_image(const KernelRef& k, const RecLaunch& l, unsigned grid_blocks, unsigned char* dst, size_t dst_bytes) {
    KernargLayout lay;
    (void)kernarg_layout_of(k, l.args.size(), lay);
    std::memcpy(dst, l.args.data(), l.args.size());
    if (dst_bytes >= (size_t)lay.kernarg_size) kmeta_fill_hidden(lay, dst, grid_blocks, l.block, l.lds);
}

// a one-dimensional dispatch of `grid_blocks` workgroups of `block` threads; header and completion signal are the submitter's
hsa_kernel_dispatch_packet_t dispatch_packet(const KernelRef& k, unsigned grid_blocks, unsigned block, size_t lds, void* kernargs) {
    hsa_kernel_dispatch_packet_t pk;
    std::memset(&pk, 0, sizeof pk);
    pk.setup = 1 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS;
    pk.workgroup_size_x = (uint16_t)block;
    pk.workgroup_size_y = pk.workgroup_size_z = 1;
    pk.grid_size_x = grid_blocks * block;
    pk.grid_size_y = pk.grid_size_z = 1;
    pk.group_segment_size = k.group_static + (uint32_t)lds;
    pk.kernel_object = k.object;
    pk.kernarg_address = kernargs;
    return pk;
}

uint16_t header_of(bool barrier, int acq, int rel) {
    return (uint16_t)((HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | ((barrier ? 1 : 0) << HSA_PACKET_HEADER_BARRIER) |
                      (acq << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) | (rel << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE));
}
// a barrier-AND packet (barrier bit set)
uint16_t barrier_header(int acq, int rel) {
    return (uint16_t)((HSA_PACKET_TYPE_BARRIER_AND << HSA_PACKET_HEADER_TYPE) | (1 << HSA_PACKET_HEADER_BARRIER) |
                      (acq << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) | (rel << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE));
}

// false: the ring stayed full until the time limit or the queue failed (the packet is NOT written; the path is marked failed)
bool put_packet(Direct& d, hsa_queue_t* hq, const void* body64, uint16_t header, uint16_t setup) {
    Hsa& h = hsa();
    if (d.failed.load()) return false;
    const uint64_t idx = h.add_write_index(hq, 1);
    if (idx - h.load_read_index(hq) >= hq->size) {  // ring full: spin briefly, then yield the core; bounded
        const double t0 = now_s();
        for (unsigned spins = 0; idx - h.load_read_index(hq) >= hq->size; ++spins) {
            if (spins < 256) {
                __builtin_ia32_pause();
            } else {
                sched_yield();
                if ((spins & 63) == 0 && (d.failed.load() || now_s() - t0 > direct_timeout_s())) {
                    direct_fail(d, "a hardware queue stayed full (the packet processor stopped consuming packets)");
                    return false;
                }
            }
        }
    }
    char* slot = (char*)hq->base_address + (idx & (hq->size - 1)) * 64;
    std::memcpy(slot + 4, (const char*)body64 + 4, 60);
    __atomic_store_n((uint32_t*)slot, (uint32_t)header | ((uint32_t)setup << 16), __ATOMIC_RELEASE);
    h.signal_store_screlease(hq->doorbell_signal, (hsa_signal_value_t)idx);
    return true;
}

namespace {
// ---- self-test: one hand-built packet before anything relies on the path ------------------------------------------------------------
// out[0] = blockDim.x, out[1] = gridDim.x (both read by the compiler from the HIDDEN arguments this file fills), out[2] = a value that
// went through the dynamic LDS the packet asked for, out[3] = number of workgroups that ran.
__global__ void k_direct_probe(unsigned* out, unsigned magic) {
    extern __shared__ unsigned probe_lds[];
    probe_lds[threadIdx.x] = magic + threadIdx.x;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) {
            out[0] = blockDim.x;
            out[1] = gridDim.x;
            out[2] = probe_lds[blockDim.x - 1];
        }
        atomicAdd(&out[3], 1u);
    }
}

int direct_selftest(Direct& d) {
    const char* off = std::getenv("SMR_DIRECT_SELFTEST");
    if (off && off[0] == '0') return SMR_OK;
    if (off && std::strcmp(off, "fail") == 0) {  // tests: the path a failing self-test takes
        d.why = "direct-dispatch self-test: forced failure ($SMR_DIRECT_SELFTEST=fail)";
        return SMR_EUNSUPPORTED;
    }
    Hsa& h = hsa();
    unsigned* out = nullptr;
    void* kargs = nullptr;
    auto done = [&](int rc, const std::string& why) {
        if (out) (void)hipHostFree(out);
        if (kargs) (void)hipHostFree(kargs);
        (void)hipGetLastError();
        if (rc != SMR_OK) d.why = "direct-dispatch self-test: " + why;
        return rc;
    };
    if (hipHostMalloc((void**)&out, 64, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&kargs, 4096, hipHostMallocDefault) != hipSuccess)
        return done(SMR_EUNSUPPORTED, "hipHostMalloc failed");
    std::memset(out, 0, 64);
    KernelRef k;
    if (resolve_kernel(d, (const void*)k_direct_probe, k) != SMR_OK) return done(SMR_EUNSUPPORTED, smr_last_error());
    const unsigned grid = 5, block = 192, lds = 192 * 4, magic = 0x5eed0000u;
    std::vector<unsigned char> ex(12);  // (unsigned* out, unsigned magic) in kernarg layout
    std::memcpy(ex.data(), &out, 8);
    std::memcpy(ex.data() + 8, &magic, 4);
    KernargLayout lay;
    if (k.private_size != 0 || k.kernarg_size > 4096 || !kernarg_layout_of(k, ex.size(), lay)) return done(SMR_EUNSUPPORTED, "the probe kernel's arguments do not match its metadata");
    std::memset(kargs, 0, 4096);
    std::memcpy(kargs, ex.data(), ex.size());
    kmeta_fill_hidden(lay, (unsigned char*)kargs, grid, block, lds);
    hsa_kernel_dispatch_packet_t pk = dispatch_packet(k, grid, block, lds, kargs);
    pk.completion_signal = d.done[0];
    h.signal_store_relaxed(d.done[0], 1);
    if (!put_packet(d, d.q[0], &pk, header_of(true, HSA_FENCE_SCOPE_SYSTEM, HSA_FENCE_SCOPE_SYSTEM), pk.setup))
        return done(SMR_EUNSUPPORTED, "the probe packet could not be written (queue error)");
    // (a short limit of its own: a first packet that does not come back within 5 s never will)
    const double t0 = now_s();
    while (h.signal_wait(d.done[0], HSA_SIGNAL_CONDITION_EQ, 0, 200000, HSA_WAIT_STATE_ACTIVE) != 0) {
        if (d.failed.load() || now_s() - t0 > std::min(5.0, direct_timeout_s())) {
            d.failed.store(true);
            {
                std::lock_guard<std::mutex> g(d.why_mu);
                d.fail_why = "the self-test packet did not complete";
            }
            // the queue may still hold the packet: the buffers stay allocated (leaked on purpose)
            out = nullptr;
            kargs = nullptr;
            return done(SMR_EUNSUPPORTED, "the probe packet did not complete (queue error or time-out)");
        }
    }
    const unsigned want2 = magic + block - 1;
    if (out[0] != block || out[1] != grid || out[2] != want2 || out[3] != grid) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "the probe kernel saw blockDim %u (want %u), gridDim %u (want %u), LDS word 0x%x (want 0x%x), %u workgroups (want %u)", out[0], block,
                      out[1], grid, out[2], want2, out[3], grid);
        return done(SMR_EUNSUPPORTED, msg);
    }
    d.probe_ok = true;
    d.probe_meta = k.from_metadata;
    return done(SMR_OK, "");
}
}  // namespace

// how the hidden-argument layout of this device's direct launches is known
const char* layout_source(const Direct& d) {
    if (!d.probe_ok) return d.n_meta > 0 && d.n_v5 == 0 ? "metadata" : "v5-rule(unverified)";
    if (d.n_v5 == 0) return "metadata+verified";
    return d.n_meta > 0 ? "metadata|v5-rule+verified" : "v5-rule+verified";
}

// the replay in flight on this device's queues has completed when this returns SMR_OK (SMR_EHIP: the direct path failed)
int wait_all(Direct& d) {
    bool any = false;
    int rc = SMR_OK;
    for (int k = 0; k < SEQ_MAXQ; ++k)
        if (d.armed[k]) {
            if (rc == SMR_OK && !wait_signal(d, d.done[k])) rc = SMR_EHIP;
            d.armed[k] = false;
            any = true;
        }
    if (any && rc == SMR_OK) d.last_us = (now_s() - d.t_submit) * 1e6;
    return rc;
}

}  // namespace smr
