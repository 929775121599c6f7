// rt_device.hip -- what every part of the HIP backend stands on: the calling
// thread's error text and device, host CPU topology (NUMA node and L3 domains
// near a GPU), the device table with its pipeline slots, and the per-device
// CU budget of the persistent verify-queue drains.  Declared in
// sha1_runtime_internal.h; the C entry points here are the device queries.
#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <sched.h>
#include <string>
#include <vector>

#include "sha1_runtime_internal.h"

using namespace s1rt;

namespace {
// Kernel launches of this process by kind (count_launch, s1be_launch_stats).
std::atomic<uint64_t> g_launches[kLaunchCounters];

// First line of a sysfs file ("" if it cannot be read).
std::string sysfs_line(const char* path) {
    char buf[4096] = {0};
    if (FILE* f = fopen(path, "r")) {
        if (!fgets(buf, sizeof buf, f)) buf[0] = 0;
        fclose(f);
    }
    return buf;
}

// The CPUs of HIP device `id`'s NUMA node (the numa_node of its PCI device)
// within `allowed`, into *out; their count, 0 when the node is unknown.
int device_node_cpus(int id, const cpu_set_t& allowed, cpu_set_t* out) {
    CPU_ZERO(out);
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof bdf, id) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    for (char* c = bdf; *c; ++c) *c = static_cast<char>(tolower(static_cast<unsigned char>(*c)));
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    const std::string nl = sysfs_line(path);
    const int node = nl.empty() ? -1 : atoi(nl.c_str());
    if (node < 0) return 0;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    return s1host::cpus_from_list(sysfs_line(path).c_str(), allowed, out);
}

bool numa_off() {
    const char* e = getenv("SHA1CHUNK_NUMA");
    return e && (!strcmp(e, "off") || !strcmp(e, "0"));
}

thread_local std::string t_err;
std::once_flag g_once;
int g_count = -1;  // >= 0 once probed

void probe() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_count = 0;
        g_probe_err = "no HIP device visible";
        return;
    }
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, d) != hipSuccess) continue;
        if (strncmp(pr.gcnArchName, "gfx950", 6) != 0) {
            g_probe_err = std::string("device ") + std::to_string(d) + " is " + pr.gcnArchName +
                          ", this build targets gfx950 only";
            continue;
        }
        ++ok;
    }
    if (ok != n) {
        g_count = 0;
        return;
    }
    // SHA1CHUNK_VIRTUAL_DEVICES=k (testing): k logical devices over the n
    // physical ones (logical d -> physical d % n), each with its own streams,
    // slots and host thread, so the multi-device path (SHA1CHUNK_ALL_DEVICES:
    // byte-balanced slices, one thread per device) runs on a one-GPU box.
    int k = n;
    if (const char* e = getenv("SHA1CHUNK_VIRTUAL_DEVICES")) k = std::max(1, std::min(64, atoi(e)));
    g_count = k;
    g_dev = new Device[k];
    for (int d = 0; d < k; ++d) g_dev[d].id = d % n;
}
}  // namespace

namespace s1rt {
// Host CPUs near HIP device `id`: the CPUs of its NUMA node within this
// process's affinity mask (s1host::process_cpus).  The library's helper
// threads -- the pageable-batch packing, the file pipeline's preads into pinned slots, the verify
// queue's split copies when asked for (SHA1CHUNK_VQ_THREADS) -- run there,
// beside the pinned memory they write (hipHostMalloc already places it on
// the GPU's node: profiles/vq_place_r06*.jsonl) and the GPU that reads it.
// SHA1CHUNK_NUMA=off (or 0) leaves them to the scheduler.  nullptr: no
// placement (off, one node, node unknown, or none of its CPUs allowed, or
// fewer than four).
const cpu_set_t* near_cpus(int id) {
    struct Near {
        std::once_flag once;
        bool ok = false;
        cpu_set_t set;
    };
    static Near near[64];
    if (id < 0 || id >= 64) return nullptr;
    Near& n = near[id];
    std::call_once(n.once, [&] {
        if (numa_off()) return;
        // the process's CPUs, not the calling thread's: the set is cached for
        // the process, and the first caller may be a pinned receive thread
        cpu_set_t allowed, mine;
        if (!s1host::process_cpus(&allowed)) return;
        // nothing to gain when every allowed CPU is on this node already,
        // and no piling of a pool's helpers onto fewer than kMinNearCpus
        constexpr int kMinNearCpus = 4;
        if (device_node_cpus(id, allowed, &mine) < kMinNearCpus || CPU_EQUAL(&mine, &allowed)) return;
        n.set = mine;
        n.ok = true;
    });
    return n.ok ? &n.set : nullptr;
}

// Receive-thread placement (sha1chunk_receive_cpus): the L3 domains of
// HIP device `id`'s node's allowed CPUs, in CPU order (of every allowed CPU
// under SHA1CHUNK_NUMA=off or when the node is unknown), once per device.
// One receive thread per domain kept `submit` at 27.7-29.6 GiB/s where
// threads floating over the node gave 23.8-36.2 (profiles/vq_l3.jsonl).
const std::vector<cpu_set_t>& receive_domains(int id) {
    struct Dom {
        std::once_flag once;
        std::vector<cpu_set_t> dom;
    };
    static Dom doms[64];
    static const std::vector<cpu_set_t> none;
    if (id < 0 || id >= 64) return none;
    Dom& d = doms[id];
    std::call_once(d.once, [&] {
        cpu_set_t allowed, base;  // the process's CPUs, as in near_cpus
        if (!s1host::process_cpus(&allowed)) return;
        if (numa_off() || device_node_cpus(id, allowed, &base) == 0) base = allowed;
        s1host::l3_domains(base, &d.dom, [](int cpu) {
            char path[128];
            snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", cpu);
            return sysfs_line(path);
        });
    });
    return d.dom;
}

thread_local int t_dev = 0;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_err = buf;
    return code;
}

std::string g_probe_err;
Device* g_dev = nullptr;

int device_count() {
    std::call_once(g_once, probe);
    return g_count;
}

// Streams and events of slots [0, n), created on first use (caller holds D.mu).
int ensure_slots(Device& D, int n) {
    for (int i = 0; i < n && i < kMaxSlots; ++i) {
        Slot& s = D.slot[i];
        if (s.stream) continue;
        HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
        HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    }
    return SHA1CHUNK_OK;
}

// The shared H2D stream of multi-slot pipelines (caller holds D.mu).
int ensure_copy(Device& D) {
    if (!D.copy) HIP_TRY(hipStreamCreateWithFlags(&D.copy, hipStreamNonBlocking));
    return SHA1CHUNK_OK;
}

// Acquire the calling thread's device (initialising it on first use).
int get_device(Device** out) {
    if (device_count() <= 0) return fail(SHA1CHUNK_ENODEV, "%s", g_probe_err.c_str());
    if (t_dev < 0 || t_dev >= g_count) return fail(SHA1CHUNK_EINVAL, "bad device %d", t_dev);
    Device& D = g_dev[t_dev];
    HIP_TRY(hipSetDevice(D.id));
    if (!D.ready.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lk(D.mu);
        if (!D.ready.load(std::memory_order_relaxed)) {
            hipDeviceProp_t pr;
            HIP_TRY(hipGetDeviceProperties(&pr, D.id));
            D.cus = pr.multiProcessorCount;
            // Only slot 0 now: a stream costs ~12-20 ms to create
            // (profiles/startup_r01.json, init_cost_r02.jsonl), and a caller
            // whose batch fits one slot (shahash, verify_hash, the CLI on a
            // small file) copies on that slot's own stream.  Other slots and
            // the copy stream are made on first use (ensure_slots, ensure_copy).
            int rc = ensure_slots(D, 1);
            if (rc) return rc;
            D.ready.store(true, std::memory_order_release);
        }
    }
    *out = &D;
    return SHA1CHUNK_OK;
}

// The slot's stream waits for its H2D copies, issued on stream `cs` (the
// copy stream, or the slot's own stream for a batch of one fill).
int copies_issued(Slot& s, hipStream_t cs) {
    if (cs == s.stream) return SHA1CHUNK_OK;
    HIP_TRY(hipEventRecord(s.copied, cs));
    HIP_TRY(hipStreamWaitEvent(s.stream, s.copied, 0));
    return SHA1CHUNK_OK;
}

// A call that failed half-way can leave a slot in flight; its results
// belong to that call, so the next call waits for the work and drops them
// instead of scattering stale digests into its own output.
int discard_in_flight(Device& D) {
    for (auto& s : D.slot) {
        if (!s.busy) continue;
        s.busy = false;
        HIP_TRY(hipEventSynchronize(s.done));
    }
    return SHA1CHUNK_OK;
}

// Share of the device's CUs a drain takes (SHA1CHUNK_VQ_CUS, default 64),
// within a per-device budget for all drains (SHA1CHUNK_VQ_CU_BUDGET,
// default half the CUs) so that queues never hold every CU: a drain
// workgroup takes a whole CU while its queue is busy, and a process's hash
// kernels and other queues need the rest.  0 when the budget is spent.
int drain_cus_take(Device* D) {
    const int want = static_cast<int>(
        std::max<uint64_t>(1, std::min<uint64_t>({static_cast<uint64_t>(D->cus), 1024, env_u64("SHA1CHUNK_VQ_CUS", 64)})));
    const int budget = static_cast<int>(std::min<uint64_t>(
        static_cast<uint64_t>(D->cus), env_u64("SHA1CHUNK_VQ_CU_BUDGET", static_cast<uint64_t>(D->cus / 2))));
    std::lock_guard<std::mutex> lk(D->drain_mu);
    const int left = budget - D->drain_cus;
    const int take = std::min(want, left);
    if (take < std::min(want, 8)) return 0;  // too few left to be worth a drain
    D->drain_cus += take;
    return take;
}

void drain_cus_give(int dev, int cus) {
    if (dev < 0 || dev >= g_count) return;
    std::lock_guard<std::mutex> lk(g_dev[dev].drain_mu);
    g_dev[dev].drain_cus -= cus;
}

// CUs of the calling thread's device that its persistent drains hold now
// (0 before the device table exists).  A kernel shape that needs every CU it
// counts on free asks this (sha1_runtime.hip split_unit).
int drain_cus_held() {
    if (!g_dev || t_dev < 0 || t_dev >= g_count) return 0;
    std::lock_guard<std::mutex> lk(g_dev[t_dev].drain_mu);
    return g_dev[t_dev].drain_cus;
}
}  // namespace s1rt

// ================================================================ C ABI ====
extern "C" {

int s1be_device_count(void) {
    const int n = device_count();
    if (n <= 0) fail(SHA1CHUNK_ENODEV, "%s", g_probe_err.c_str());
    return n;
}

int s1be_set_device(int device) {
    const int n = device_count();
    if (n <= 0) return fail(SHA1CHUNK_ENODEV, "%s", g_probe_err.c_str());
    if (device < 0 || device >= n) return fail(SHA1CHUNK_EINVAL, "device %d of %d", device, n);
    t_dev = device;
    return SHA1CHUNK_OK;
}

const char* s1be_last_error(void) { return t_err.c_str(); }

// PCI address of logical device `device`'s physical GPU (multi-device tests
// and bench.py's device identity: distinct ranks/threads, distinct GPUs).
int s1be_device_pci_bus_id(int device, char* buf, size_t len) {
    const int n = device_count();
    if (n <= 0) return fail(SHA1CHUNK_ENODEV, "%s", g_probe_err.c_str());
    if (device < 0 || device >= n) return fail(SHA1CHUNK_EINVAL, "device %d of %d", device, n);
    if (len > static_cast<size_t>(INT32_MAX)) len = INT32_MAX;
    HIP_TRY(hipDeviceGetPCIBusId(buf, static_cast<int>(len), g_dev[device].id));
    return SHA1CHUNK_OK;
}

// The CPUs for receive thread `slot` of device `device` (L3 domain slot mod
// their count; receive_domains), as a cpu_set_t of `len` >= its size bytes.
int s1be_receive_cpus(int device, unsigned slot, void* mask, size_t len, unsigned* domains) {
    const int n = device_count();
    if (n <= 0) return fail(SHA1CHUNK_ENODEV, "%s", g_probe_err.c_str());
    if (device < 0 || device >= n) return fail(SHA1CHUNK_EINVAL, "device %d of %d", device, n);
    const std::vector<cpu_set_t>& dom = receive_domains(g_dev[device].id);
    if (dom.empty()) return fail(SHA1CHUNK_EINVAL, "no CPU of this process's affinity mask found");
    const cpu_set_t& d = dom[slot % dom.size()];
    memset(mask, 0, len);
    memcpy(mask, &d, sizeof d);
    if (domains) *domains = static_cast<unsigned>(dom.size());
    return CPU_COUNT(&d);
}

// Diagnostics (tests/launch_stats.py; no front-end symbol): how often each
// kind of kernel was enqueued in this process so far, out[0 .. 10] in
// LaunchCounter's order (sha1_kernels.h); reset != 0 then zeroes them.
// out[11]: the CUs the calling thread's device's persistent drains hold now
// (drain_cus_held), a gauge that reset leaves alone.
void s1be_launch_stats(uint64_t* out, int reset) {
    for (int i = 0; i < kLaunchCounters; ++i) {
        if (out) out[i] = g_launches[i].load(std::memory_order_relaxed);
        if (reset) g_launches[i].store(0, std::memory_order_relaxed);
    }
    if (out) out[kLaunchCounters] = static_cast<uint64_t>(drain_cus_held());
}

}  // extern "C"

void count_launch(LaunchCounter which) { g_launches[which].fetch_add(1, std::memory_order_relaxed); }
