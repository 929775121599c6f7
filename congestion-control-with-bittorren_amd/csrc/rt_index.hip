// rt_index.hip -- host side of the digest index (include/sha1chunk.h, "Digest
// index": sha1chunk_index_create / _destroy / _size / _capacity / _reserve, the
// device and host lookups and appends, sha1chunk_match_batch,
// sha1chunk_match_fd and sha1chunk_admit_batch; kernels in sha1_index.hip,
// arithmetic in index_map.hpp).
//
// An index owns two device allocations: a table with room for `capacity`
// digests, and slots_for(capacity) slots behind a 128-byte block of counters
// (the build's three words first, the appends' three from byte 64 on).
// create() fills both on the index stream of its device (one per device, made
// by the first create; creates and growths on one device take turns on it),
// builds, reads the counters back and waits; from then on any stream may look
// up.
//
// An append is a copy of the new rows into table + 5 size and, behind it on
// the same stream, the append kernel; the host knows the new size when it
// enqueues.  The device form never allocates and refuses when capacity is
// short.  Growth (reserve, and the host append when the index is full):
// wait for the device, new table and slots, rows [0, size) and the counters
// copied, slots emptied, the old slots rehashed into the new ones on the index
// stream, wait for the device, old arrays freed.
//
// The host forms go through the device: the queries are staged up in
// sub-batches of at most 2^22 through a stage per device, looked up on slot
// 0's stream under the device's mutex, and 4 bytes per query come back.  The
// host append takes the same turn: rows straight into the table, skip bytes
// through a stage, one wait at the end.
// match_batch(HOST) and match_fd run s1be_hash_batch / s1be_hash_fd unchanged
// and look the digests up afterwards; match_batch(DEVICE) is
// s1be_verify_batch(DEVICE) with the lookup where the compare is, and
// admit_batch(DEVICE) is the same sequence with the append behind the compare.
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <mutex>
#include <new>

#include "index_map.hpp"
#include "sha1_runtime_internal.h"

using namespace s1rt;

extern "C" {
int s1be_hash_device_async(const void*, const uint64_t*, const uint32_t*, size_t, uint8_t*, void*, int);
int s1be_hash_batch(const void*, const uint64_t*, const uint32_t*, size_t, uint8_t*, unsigned);
int s1be_compare_device_async(const uint8_t*, const uint8_t*, size_t, uint8_t*, void*);
long s1be_hash_fd(int, uint8_t*, size_t, size_t*);
}

struct sha1chunk_index {
    int dev;  // the logical device it belongs to
    // positions handed out and room for them: written by one appender at a
    // time, read by sha1chunk_index_size / _capacity from any thread
    std::atomic<uint64_t> m, capacity;
    uint64_t slots;   // slots_for(capacity)
    uint32_t* table;  // capacity x 5 words, rows [0, m) written
    uint8_t* mem;     // [counters: 128 bytes | slots]
    uint64_t stats[4];
};

namespace {
constexpr size_t kCounterBytes = 128;
constexpr size_t kAppendCounters = 64;  // byte offset of the appends' counters in the block
constexpr size_t kHostSub = size_t(1) << 22;        // queries per staged sub-batch of the host lookup
constexpr size_t kBatchMax = 0xffffffffu - 1024u;   // check_batch's limit (sha1_runtime.hip)

struct IndexDev {
    std::mutex build;              // creates on this device, one at a time
    hipStream_t stream = nullptr;  // the index stream
    DevBuf queries, ids;           // host lookups, under the device's mutex
    DevBuf skip;                   // host appends' skip bytes, under the device's mutex
};
IndexDev* g_ixdev;  // one per logical device
std::once_flag g_ixdev_once;

IndexDev& ixdev_of(Device& D) {
    std::call_once(g_ixdev_once, [] { g_ixdev = new IndexDev[std::max(1, device_count())]; });
    return g_ixdev[&D - g_dev];
}

IndexArgs args_of(const sha1chunk_index* ix) {
    IndexArgs X{};
    X.table = ix->table;
    X.m = static_cast<uint32_t>(ix->m.load(std::memory_order_relaxed));
    X.slots = reinterpret_cast<uint32_t*>(ix->mem + kCounterBytes);
    X.mask = static_cast<uint32_t>(ix->slots - 1);
    X.stats = reinterpret_cast<unsigned long long*>(ix->mem);
    return X;
}

bool misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) & 3u; }

// The calling thread's device, which must be the index's.
int device_of(const sha1chunk_index* ix, Device** D) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (int rc = get_device(D)) return rc;
    if (t_dev != ix->dev)
        return fail(SHA1CHUNK_EINVAL, "the index belongs to device %d, the current device is %d", ix->dev, t_dev);
    return SHA1CHUNK_OK;
}

// Every refusal of a lookup of n queries.
int check_lookup(const void* digests, size_t n, const void* ids) {
    if (n > s1ix::kMaxQueries) return fail(SHA1CHUNK_EINVAL, "n too large: at most 2^32 - 256 per call");
    if (n && (!digests || !ids)) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (n && (misaligned(digests) || misaligned(ids)))
        return fail(SHA1CHUNK_EALIGN, "digest and id arrays must be 4-byte aligned");
    return SHA1CHUNK_OK;
}

int enqueue_lookup(const sha1chunk_index* ix, const void* d_digests, size_t n, void* d_ids, hipStream_t st) {
    const hipError_t e = launch_index_lookup(args_of(ix), static_cast<const uint32_t*>(d_digests),
                                             static_cast<uint32_t>(n), static_cast<uint32_t*>(d_ids), st);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "index lookup launch: %s", hipGetErrorString(e));
    return SHA1CHUNK_OK;
}

// Host arrays, already checked: staged up, looked up, 4 n bytes back.
int lookup_host(Device& D, const sha1chunk_index* ix, const uint8_t* digests, size_t n, uint32_t* ids) {
    IndexDev& I = ixdev_of(D);
    std::lock_guard<std::mutex> lk(D.mu);
    int rc;
    if ((rc = discard_in_flight(D))) return rc;
    hipStream_t st = D.slot[0].stream;
    for (size_t lo = 0; lo < n; lo += kHostSub) {
        const size_t k = std::min(kHostSub, n - lo);
        if ((rc = I.queries.ensure(k * 20)) || (rc = I.ids.ensure(k * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(I.queries.p, digests + 20 * lo, k * 20, hipMemcpyHostToDevice, st));
        if ((rc = enqueue_lookup(ix, I.queries.p, k, I.ids.p, st))) return rc;
        HIP_TRY(hipMemcpyAsync(ids + lo, I.ids.p, k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SHA1CHUNK_OK;
}

// Every refusal of an append of k digests that needs no look at the index.
int check_append(const void* digests, size_t k) {
    if (k > s1ix::kMaxQueries) return fail(SHA1CHUNK_EINVAL, "k too large: at most 2^32 - 256 per call");
    if (k && !digests) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (k && misaligned(digests)) return fail(SHA1CHUNK_EALIGN, "digest array must be 4-byte aligned");
    return SHA1CHUNK_OK;
}

int check_total(const sha1chunk_index* ix, size_t k) {
    if (ix->m.load(std::memory_order_relaxed) + k > s1ix::kMaxEntries)
        return fail(SHA1CHUNK_EINVAL, "index of %llu digests and %zu more: at most 2^31",
                    static_cast<unsigned long long>(ix->m.load(std::memory_order_relaxed)), k);
    return SHA1CHUNK_OK;
}

// The device form's refusal: it never allocates.
int check_room(const sha1chunk_index* ix, size_t k) {
    const uint64_t m = ix->m.load(std::memory_order_relaxed), cap = ix->capacity.load(std::memory_order_relaxed);
    if (m + k > cap)
        return fail(SHA1CHUNK_EINVAL,
                    "index full: %llu digests and %zu more, capacity %llu; call sha1chunk_index_reserve first",
                    static_cast<unsigned long long>(m), k, static_cast<unsigned long long>(cap));
    return SHA1CHUNK_OK;
}

// k rows from `rows` (device memory, or host memory with from_host) into the
// table behind the last position, then the append kernel: both on st.  Checked
// by the caller: k > 0 and m + k <= capacity.  The size grows here, at enqueue.
int enqueue_append(sha1chunk_index* ix, const void* rows, size_t k, const uint8_t* d_skip, bool from_host,
                   hipStream_t st) {
    const uint64_t m = ix->m.load(std::memory_order_relaxed);
    HIP_TRY(hipMemcpyAsync(ix->table + s1ix::kWords * m, rows, k * 20,
                           from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    IndexArgs X = args_of(ix);
    X.stats = reinterpret_cast<unsigned long long*>(ix->mem + kAppendCounters);
    const hipError_t e = launch_index_append(X, static_cast<uint32_t>(m), static_cast<uint32_t>(k), d_skip, st);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "index append launch: %s", hipGetErrorString(e));
    ix->m.store(m + k, std::memory_order_relaxed);
    return SHA1CHUNK_OK;
}

// Room for `capacity` digests, which is more than the index has.  The caller
// holds the device's mutex (the host forms wait their turn); the index stream
// is taken here.  Device-form calls of other threads must not overlap: their
// queued work is waited for first, and whatever they queued later would meet
// freed arrays.
int grow(Device& D, sha1chunk_index* ix, uint64_t capacity) {
    IndexDev& I = ixdev_of(D);
    std::lock_guard<std::mutex> lk(I.build);
    if (!I.stream) HIP_TRY(hipStreamCreateWithFlags(&I.stream, hipStreamNonBlocking));
    HIP_TRY(hipDeviceSynchronize());  // appends queued on any stream have filled the old slots
    const uint64_t m = ix->m.load(std::memory_order_relaxed), slots = s1ix::slots_for(capacity);
    uint32_t* table = nullptr;
    uint8_t* mem = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&table), std::max<size_t>(capacity * 20, 128)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&mem), kCounterBytes + slots * 4) != hipSuccess) {
        (void)hipGetLastError();
        if (table) (void)hipFree(table);
        return fail(SHA1CHUNK_ENOMEM, "index of %llu digests: device allocation failed",
                    static_cast<unsigned long long>(capacity));
    }
    IndexArgs X = args_of(ix);  // the old arrays
    const uint32_t* old_slots = X.slots;
    const uint32_t old_mask = X.mask;
    X.table = table;
    X.slots = reinterpret_cast<uint32_t*>(mem + kCounterBytes);
    X.mask = static_cast<uint32_t>(slots - 1);
    X.stats = nullptr;
    hipError_t e = hipSuccess;
    if (m) e = hipMemcpyAsync(table, ix->table, m * 20, hipMemcpyDeviceToDevice, I.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(mem, ix->mem, kCounterBytes, hipMemcpyDeviceToDevice, I.stream);
    if (e == hipSuccess) e = hipMemsetAsync(mem + kCounterBytes, 0xff, slots * 4, I.stream);
    if (e == hipSuccess) e = launch_index_rehash(X, old_slots, old_mask, I.stream);
    const hipError_t waited = hipDeviceSynchronize();
    if (e == hipSuccess) e = waited;
    if (e != hipSuccess) {
        (void)hipFree(table);
        (void)hipFree(mem);
        return fail(SHA1CHUNK_EHIP, "index growth to %llu digests: %s", static_cast<unsigned long long>(capacity),
                    hipGetErrorString(e));
    }
    (void)hipFree(ix->table);
    (void)hipFree(ix->mem);
    ix->table = table;
    ix->mem = mem;
    ix->slots = slots;
    ix->capacity.store(capacity, std::memory_order_relaxed);
    ix->stats[0] = slots;
    return SHA1CHUNK_OK;
}

// Host arrays, already checked: grown when full (at least doubled), rows
// straight into the table, skip bytes staged up, one wait at the end.
int append_host(Device& D, sha1chunk_index* ix, const uint8_t* digests, size_t k, const uint8_t* skip) {
    IndexDev& I = ixdev_of(D);
    std::lock_guard<std::mutex> lk(D.mu);
    int rc;
    if ((rc = check_total(ix, k))) return rc;
    if ((rc = discard_in_flight(D))) return rc;
    const uint64_t m = ix->m.load(std::memory_order_relaxed), cap = ix->capacity.load(std::memory_order_relaxed);
    if (m + k > cap && (rc = grow(D, ix, std::min<uint64_t>(std::max<uint64_t>(m + k, 2 * cap), s1ix::kMaxEntries))))
        return rc;
    hipStream_t st = D.slot[0].stream;
    for (size_t lo = 0; lo < k; lo += kHostSub) {
        const size_t sub = std::min(kHostSub, k - lo);
        if (skip) {
            if ((rc = I.skip.ensure(sub))) return rc;
            HIP_TRY(hipMemcpyAsync(I.skip.p, skip + lo, sub, hipMemcpyHostToDevice, st));
        }
        if ((rc = enqueue_append(ix, digests + 20 * lo, sub, skip ? static_cast<const uint8_t*>(I.skip.p) : nullptr, true,
                                 st)))
            return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SHA1CHUNK_OK;
}

void release(sha1chunk_index* ix) {
    if (ix->table) (void)hipFree(ix->table);
    if (ix->mem) (void)hipFree(ix->mem);
    delete ix;
}

// Table up, slots emptied, counters zeroed, build, counters back: all on the
// index stream, waited for.
int build(Device& D, sha1chunk_index* ix, const uint8_t* digests, unsigned flags) {
    IndexDev& I = ixdev_of(D);
    std::lock_guard<std::mutex> lk(I.build);
    if (!I.stream) HIP_TRY(hipStreamCreateWithFlags(&I.stream, hipStreamNonBlocking));
    const uint64_t m = ix->m.load(std::memory_order_relaxed);
    if (hipMalloc(reinterpret_cast<void**>(&ix->table), std::max<size_t>(m * 20, 128)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&ix->mem), kCounterBytes + ix->slots * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SHA1CHUNK_ENOMEM, "index of %llu digests: device allocation failed",
                    static_cast<unsigned long long>(m));
    }
    if (m)
        HIP_TRY(hipMemcpyAsync(ix->table, digests, m * 20,
                               flags & SHA1CHUNK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, I.stream));
    HIP_TRY(hipMemsetAsync(ix->mem, 0, kCounterBytes, I.stream));
    HIP_TRY(hipMemsetAsync(ix->mem + kCounterBytes, 0xff, ix->slots * 4, I.stream));
    const hipError_t e = launch_index_build(args_of(ix), I.stream);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "index build launch: %s", hipGetErrorString(e));
    unsigned long long counters[3];
    HIP_TRY(hipMemcpyAsync(counters, ix->mem, sizeof counters, hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipStreamSynchronize(I.stream));
    ix->stats[0] = ix->slots;
    ix->stats[1] = m ? std::max<uint64_t>(1, counters[0]) : 0;
    ix->stats[2] = counters[1];
    ix->stats[3] = counters[2];
    return SHA1CHUNK_OK;
}
}  // namespace

// ================================================================ C ABI ====
extern "C" {

sha1chunk_index* s1be_index_create(const uint8_t* digests, size_t m, unsigned flags) {
    if (flags & SHA1CHUNK_ALL_DEVICES) {
        fail(SHA1CHUNK_EINVAL, "SHA1CHUNK_ALL_DEVICES: an index belongs to one device");
        return nullptr;
    }
    if (flags & ~SHA1CHUNK_DEVICE) {
        fail(SHA1CHUNK_EINVAL, "unknown flags %#x", flags);
        return nullptr;
    }
    if (m > s1ix::kMaxEntries) {
        fail(SHA1CHUNK_EINVAL, "index of %zu digests: at most 2^31", m);
        return nullptr;
    }
    if (m && !digests) {
        fail(SHA1CHUNK_EINVAL, "null pointer");
        return nullptr;
    }
    if (m && misaligned(digests)) {
        fail(SHA1CHUNK_EALIGN, "digest array must be 4-byte aligned");
        return nullptr;
    }
    Device* D;
    if (get_device(&D)) return nullptr;
    sha1chunk_index* ix = new (std::nothrow) sha1chunk_index{};
    if (!ix) {
        fail(SHA1CHUNK_ENOMEM, "index allocation failed");
        return nullptr;
    }
    ix->dev = t_dev;
    ix->m = m;
    ix->capacity = m;
    ix->slots = s1ix::slots_for(m);
    if (build(*D, ix, digests, flags)) {
        release(ix);
        return nullptr;
    }
    return ix;
}

// On the index's device, whichever is current.
void s1be_index_destroy(sha1chunk_index* ix) {
    if (!ix) return;
    if (g_dev && ix->dev >= 0 && ix->dev < device_count()) (void)hipSetDevice(g_dev[ix->dev].id);
    release(ix);
    if (g_dev && t_dev >= 0 && t_dev < device_count()) (void)hipSetDevice(g_dev[t_dev].id);
}

size_t s1be_index_size(const sha1chunk_index* ix) {
    return ix ? static_cast<size_t>(ix->m.load(std::memory_order_relaxed)) : 0;
}

size_t s1be_index_capacity(const sha1chunk_index* ix) {
    return ix ? static_cast<size_t>(ix->capacity.load(std::memory_order_relaxed)) : 0;
}

int s1be_index_reserve(sha1chunk_index* ix, size_t capacity) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (capacity > s1ix::kMaxEntries) return fail(SHA1CHUNK_EINVAL, "index of %zu digests: at most 2^31", capacity);
    Device* D;
    if (int rc = device_of(ix, &D)) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    if (capacity <= ix->capacity.load(std::memory_order_relaxed)) return SHA1CHUNK_OK;
    if (int rc = discard_in_flight(*D)) return rc;
    return grow(*D, ix, capacity);
}

int s1be_index_append_device_async(sha1chunk_index* ix, const uint8_t* d_digests, size_t k, const uint8_t* d_skip,
                                   void* stream) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (int rc = check_append(d_digests, k)) return rc;
    Device* D;
    if (int rc = device_of(ix, &D)) return rc;
    if (k == 0) return SHA1CHUNK_OK;
    if (int rc = check_total(ix, k)) return rc;
    if (int rc = check_room(ix, k)) return rc;
    return enqueue_append(ix, d_digests, k, d_skip, false, static_cast<hipStream_t>(stream));
}

int s1be_index_append(sha1chunk_index* ix, const uint8_t* digests, size_t k, const uint8_t* skip) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (int rc = check_append(digests, k)) return rc;
    Device* D;
    if (int rc = device_of(ix, &D)) return rc;
    if (k == 0) return SHA1CHUNK_OK;
    return append_host(*D, ix, digests, k, skip);
}

int s1be_index_lookup_device_async(const sha1chunk_index* ix, const uint8_t* d_digests, size_t n, uint32_t* d_ids,
                                   void* stream) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (int rc = check_lookup(d_digests, n, d_ids)) return rc;
    Device* D;
    if (int rc = device_of(ix, &D)) return rc;
    if (n == 0) return SHA1CHUNK_OK;
    return enqueue_lookup(ix, d_digests, n, d_ids, static_cast<hipStream_t>(stream));
}

int s1be_index_lookup(const sha1chunk_index* ix, const uint8_t* digests, size_t n, uint32_t* ids) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (int rc = check_lookup(digests, n, ids)) return rc;
    Device* D;
    if (int rc = device_of(ix, &D)) return rc;
    if (n == 0) return SHA1CHUNK_OK;
    return lookup_host(*D, ix, digests, n, ids);
}

int s1be_match_batch(const sha1chunk_index* ix, const void* base, const uint64_t* offsets, const uint32_t* lengths,
                     size_t n, uint32_t* ids, unsigned flags) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (flags & SHA1CHUNK_ALL_DEVICES)
        return fail(SHA1CHUNK_EINVAL, "SHA1CHUNK_ALL_DEVICES: an index belongs to one device");
    if (flags & ~SHA1CHUNK_DEVICE) return fail(SHA1CHUNK_EINVAL, "unknown flags %#x", flags);
    if (n > kBatchMax) return fail(SHA1CHUNK_EINVAL, "n too large: at most 2^32 - 1025 chunks per call");
    if (n && (!base || !offsets || !lengths || !ids)) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (n && misaligned(ids)) return fail(SHA1CHUNK_EALIGN, "id array must be 4-byte aligned");
    Device* D;
    int rc = device_of(ix, &D);
    if (rc || n == 0) return rc;
    if (flags & SHA1CHUNK_DEVICE) {
        std::lock_guard<std::mutex> lk(D->mu);
        Slot& s = D->slot[0];
        if ((rc = s.ddig.ensure(n * 20))) return rc;
        if ((rc = s1be_hash_device_async(base, offsets, lengths, n, static_cast<uint8_t*>(s.ddig.p), s.stream,
                                         SHA1CHUNK_KERNEL_AUTO)))
            return rc;
        if ((rc = enqueue_lookup(ix, s.ddig.p, n, ids, s.stream))) return rc;
        HIP_TRY(hipStreamSynchronize(s.stream));
        return SHA1CHUNK_OK;
    }
    uint8_t* dig = new (std::nothrow) uint8_t[n * 20];
    if (!dig) return fail(SHA1CHUNK_ENOMEM, "digests of %zu chunks", n);
    rc = s1be_hash_batch(base, offsets, lengths, n, dig, SHA1CHUNK_HOST);
    if (!rc) rc = lookup_host(*D, ix, dig, n, ids);
    delete[] dig;
    return rc;
}

int s1be_admit_batch(sha1chunk_index* ix, const void* base, const uint64_t* offsets, const uint32_t* lengths,
                     size_t n, const uint8_t* expected, uint8_t* mismatch, unsigned flags) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (flags & SHA1CHUNK_ALL_DEVICES)
        return fail(SHA1CHUNK_EINVAL, "SHA1CHUNK_ALL_DEVICES: an index belongs to one device");
    if (flags & ~SHA1CHUNK_DEVICE) return fail(SHA1CHUNK_EINVAL, "unknown flags %#x", flags);
    if (n > kBatchMax) return fail(SHA1CHUNK_EINVAL, "n too large: at most 2^32 - 1025 chunks per call");
    if (n && (!base || !offsets || !lengths || !expected || !mismatch)) return fail(SHA1CHUNK_EINVAL, "null pointer");
    Device* D;
    int rc = device_of(ix, &D);
    if (rc || n == 0) return rc;
    if (flags & SHA1CHUNK_DEVICE) {
        std::lock_guard<std::mutex> lk(D->mu);
        if ((rc = check_total(ix, n)) || (rc = check_room(ix, n))) return rc;
        Slot& s = D->slot[0];
        if ((rc = s.ddig.ensure(n * 20))) return rc;
        if ((rc = s1be_hash_device_async(base, offsets, lengths, n, static_cast<uint8_t*>(s.ddig.p), s.stream,
                                         SHA1CHUNK_KERNEL_AUTO)))
            return rc;
        if ((rc = s1be_compare_device_async(static_cast<uint8_t*>(s.ddig.p), expected, n, mismatch, s.stream)))
            return rc;
        if ((rc = enqueue_append(ix, s.ddig.p, n, mismatch, false, s.stream))) return rc;
        HIP_TRY(hipStreamSynchronize(s.stream));
        return SHA1CHUNK_OK;
    }
    if ((rc = check_total(ix, n))) return rc;
    uint8_t* dig = new (std::nothrow) uint8_t[n * 20];
    if (!dig) return fail(SHA1CHUNK_ENOMEM, "digests of %zu chunks", n);
    rc = s1be_hash_batch(base, offsets, lengths, n, dig, SHA1CHUNK_HOST);
    if (!rc) {
        for (size_t i = 0; i < n; ++i) mismatch[i] = memcmp(dig + 20 * i, expected + 20 * i, 20) != 0;
        rc = append_host(*D, ix, dig, n, mismatch);
    }
    delete[] dig;
    return rc;
}

long s1be_match_fd(const sha1chunk_index* ix, int fd, uint32_t* ids, size_t max_chunks, size_t* total_chunks) {
    if (!ix) return fail(SHA1CHUNK_EINVAL, "null index");
    if (max_chunks && !ids) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (max_chunks && misaligned(ids)) return fail(SHA1CHUNK_EALIGN, "id array must be 4-byte aligned");
    Device* D;
    if (int rc = device_of(ix, &D)) return rc;
    // digests for the chunks asked for, and of a regular file for no more
    // than it holds from the fd's offset on
    size_t cap = max_chunks;
    struct stat st;
    const off_t pos = lseek(fd, 0, SEEK_CUR);
    if (pos >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
        const uint64_t bytes = st.st_size > pos ? static_cast<uint64_t>(st.st_size - pos) : 0;
        cap = std::min<uint64_t>(cap, (bytes + SHA1CHUNK_CHUNK_LEN - 1) / SHA1CHUNK_CHUNK_LEN);
    }
    if (cap > s1ix::kMaxQueries) return fail(SHA1CHUNK_EINVAL, "max_chunks too large: at most 2^32 - 256 per call");
    uint8_t* dig = new (std::nothrow) uint8_t[std::max<size_t>(cap, 1) * 20];
    if (!dig) return fail(SHA1CHUNK_ENOMEM, "digests of %zu chunks", cap);
    size_t total = 0;
    long n = s1be_hash_fd(fd, dig, cap, &total);
    if (n >= 0 && total > cap && cap < max_chunks)
        n = fail(SHA1CHUNK_EIO, "the file grew while it was hashed");
    if (n > 0)
        if (int rc = lookup_host(*D, ix, dig, static_cast<size_t>(n), ids)) n = rc;
    delete[] dig;
    if (n >= 0 && total_chunks) *total_chunks = total;
    return n;
}

// Diagnostics (tests; no front-end entry point): out[0] slots, out[1] the
// longest build probe in slots visited (1 = every home was free, 0 for an
// empty table), out[2] entries that found their own digest in place (m less
// the number of distinct digests), out[3] entries whose probe wrapped past the
// last slot.  out[1] and out[3] depend on the order the lanes arrived in.
int s1be_index_stats(const sha1chunk_index* ix, uint64_t out[4]) {
    if (!ix || !out) return fail(SHA1CHUNK_EINVAL, "null pointer");
    memcpy(out, ix->stats, sizeof ix->stats);
    return SHA1CHUNK_OK;
}

// Diagnostics (tests; no front-end entry point), after every append so far
// is complete: what the append kernels added up since create -- out[0] the
// longest probe in slots visited where one went past its home (else 0), out[1]
// appended entries that found their own digest in place, out[2] entries whose
// probe wrapped past the last slot.  Skipped entries probe nothing.
int s1be_index_append_stats(const sha1chunk_index* ix, uint64_t out[3]) {
    if (!ix || !out) return fail(SHA1CHUNK_EINVAL, "null pointer");
    Device* D;
    if (int rc = device_of(ix, &D)) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    if (int rc = discard_in_flight(*D)) return rc;
    unsigned long long counters[3];
    hipStream_t st = D->slot[0].stream;
    HIP_TRY(hipMemcpyAsync(counters, ix->mem + kAppendCounters, sizeof counters, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) out[i] = counters[i];
    return SHA1CHUNK_OK;
}

}  // extern "C"
