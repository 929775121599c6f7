// sha1_runtime_internal.h -- the internal header of the backend's host side
// (rt_device.hip, sha1_runtime.hip, rt_file.hip, vq.hip, vq_persistent.hip,
// sha1_pv.hip, rt_update.hip, rt_gather.hip, rt_index.hip): the thread's error text and device, the device table and its
// pipeline slots, host CPU placement, kernel choice and checked launches, and
// what the verify queues and the progressive verifier share.  All of it is
// internal to libsha1chunk_hip.so: the library exports its s1be_* entry
// points only (backend.map).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <ctime>
#include <memory>
#include <mutex>
#include <sched.h>
#include <string>
#include <vector>

#include "../../include/sha1chunk.h"
#include "part_pool.hpp"
#include "sha1_kernels.h"

extern "C" const char* s1be_last_error(void);  // rt_device.hip

namespace s1rt {
using s1host::PartPool;

// ---- rt_device.hip: error text, devices, slots, topology, drain CU budget --
// (each function's comment is at its definition)
// Sets the calling thread's error text (s1be_last_error) and returns code.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return s1rt::fail(SHA1CHUNK_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                              __FILE__, __LINE__);                                                  \
    } while (0)

constexpr size_t kAlign = 128;  // device layout: every chunk starts on a 128-B line
inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* e = getenv(name);
    return e ? strtoull(e, nullptr, 10) : dflt;
}

inline int64_t mono_ns() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return int64_t(ts.tv_sec) * 1000000000 + ts.tv_nsec;
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return SHA1CHUNK_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        bytes = round_up(std::max(bytes, size_t(1) << 20), size_t(1) << 20);
        if (hipMalloc(&p, bytes) != hipSuccess)
            return fail(SHA1CHUNK_ENOMEM, "hipMalloc(%zu) failed", bytes);
        cap = bytes;
        return SHA1CHUNK_OK;
    }
};

struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return SHA1CHUNK_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        bytes = round_up(std::max(bytes, size_t(1) << 20), size_t(1) << 20);
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess)
            return fail(SHA1CHUNK_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
        cap = bytes;
        return SHA1CHUNK_OK;
    }
};

constexpr int kMaxSlots = 8;

// One pipeline slot: pinned staging for [meta | data], device mirror,
// digests on both sides, its own stream and completion event.
struct Slot {
    PinBuf hpin;    // meta (offsets, lengths, order) then chunk bytes
    PinBuf hdig;    // n x 20 digests back from the device
    DevBuf dmem;    // device copy of hpin
    DevBuf ddig;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t copied = nullptr;  // this slot's H2D has landed (copy stream)
    bool busy = false;
    // bookkeeping for the batch in flight
    std::vector<uint32_t> ids;  // caller chunk index of each staged entry
};

struct Device {
    std::mutex mu;
    std::atomic<bool> ready{false};  // set once, under mu, after the streams exist
    int id = -1;
    int cus = 256;
    // Host batches use slots 0-1; the stream (file) pipeline cycles through
    // stream_slots() of them.
    Slot slot[kMaxSlots];
    // Every slot's H2D goes through this one stream: copies run back to back
    // at the full PCIe rate instead of two slots splitting it (which would
    // delay the first kernel), and the next slot's copy queues behind the
    // current one while the current slot's kernel runs.
    hipStream_t copy = nullptr;
    DevBuf small;  // streaming calls: state + data
    PinBuf small_pin;
    // threads that pack pageable host chunks into pinned staging (created on
    // the first such batch, alive with the process; idle ones sleep)
    std::unique_ptr<PartPool> pack;
    // CUs held by the persistent verify-queue drains of this device (under
    // drain_mu): each drain workgroup takes a whole CU (all of its LDS)
    std::mutex drain_mu;
    int drain_cus = 0;
};

// The device table (g_dev[0 .. device_count()), null before the probe), why
// the probe found no usable device, and the calling thread's logical device
// (s1be_set_device; the multi-device paths' per-device threads set their own).
extern Device* g_dev;
extern std::string g_probe_err;
extern thread_local int t_dev;
int device_count();
int get_device(Device** out);  // the calling thread's, initialised on first use
int ensure_slots(Device& D, int n);
int ensure_copy(Device& D);
int copies_issued(Slot& s, hipStream_t cs);
int discard_in_flight(Device& D);
const cpu_set_t* near_cpus(int id);
const std::vector<cpu_set_t>& receive_domains(int id);
int drain_cus_take(Device* D);
void drain_cus_give(int dev, int cus);
int drain_cus_held();

// ---- sha1_runtime.hip: kernel choice and checked launches ------------------
int choose_kernel(int kernel, size_t n, int cus);
int launch_checked(int kernel, const BatchArgs& A, hipStream_t st, int cus = 256);
bool use_mixed(size_t n, int cus);
int launch_mixed_checked(const BatchArgs& A, const uint32_t* sorted_len, const BigFix* big, uint32_t* plan, int cus,
                         hipStream_t st);
bool host_pinned(const void* p);
int pack_threads();

// ---- vq.hip: shared by both queue modes and the progressive verifier -------
int vq_copy_helpers();
unsigned ring_flags();
int vq_stream_create(hipStream_t* s);  // 0 or -1
}  // namespace s1rt
