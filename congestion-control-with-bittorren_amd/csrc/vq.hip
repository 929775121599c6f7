// vq.hip -- the verify queue of the HIP backend (sha1chunk_vq): the queue
// object, its batch mode (a launch per batch: SHA1CHUNK_VQ_MODE=batch, or the
// device's drain CU budget spent), the lock and its statistics, and every
// s1be_vq_* entry point.  The default mode, the persistent drain, is
// vq_persistent.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "vq_persistent.hpp"

using namespace s1rt;

namespace s1rt {
int vq_copy_helpers() {
    const char* e = getenv("SHA1CHUNK_VQ_THREADS");
    // threads in all, the caller included.  Default 1: the calling thread
    // copies the chunk it has just filled (hot in its own core's caches);
    // helper threads on other cores have to pull it across the fabric and
    // cost more than they add.  16384 x 512 KiB, 1484-byte fills, receive
    // threads one per L3 domain (profiles/vq_threads*_r06.jsonl): 1 / 4
    // receive threads at 1 copy thread 18.5 / 46.7 GiB/s, at 4 7.7 / 26.8
    // (persistent queue; batch mode 19.3 / 29.2 against 8.8 / 22.4, and the
    // same with a DRAM-resident source).  Round 2 had measured 4 best (16.9
    // / 46.4 / 36.5 GiB/s for 1 / 4 / 8 on one thread submitting batches of
    // 1024) on the round-2 queue.
    return std::max(0, (e ? atoi(e) : 1) - 1);
}

// Ring memory (SHA1CHUNK_VQ_RING_MEM): "uncached" (default) or "coherent"
// pinned host memory; the drain reads it over PCIe while the host writes.
unsigned ring_flags() {
    const char* e = getenv("SHA1CHUNK_VQ_RING_MEM");
    return e && !strcmp(e, "coherent") ? hipHostMallocCoherent : hipHostMallocUncached;
}

// The verify queue's own streams (its drains' two launch slots and its copy
// stream) are created at a priority of their own (SHA1CHUNK_VQ_PRIO: "low",
// the default, "normal" or "high").  HIP serves a process's streams from a
// few hardware queues (GPU_MAX_HW_QUEUES, 4) and streams of different
// priorities from different ones, so a queue's persistent drain and the
// barrier packets its copy stream's events leave behind (each waits for a
// staged copy on the copy engine) never sit in front of the caller's own
// work -- a hash batch on a stream of the default priority.
int vq_stream_create(hipStream_t* s) {
    const char* e = getenv("SHA1CHUNK_VQ_PRIO");
    const std::string want = e ? e : "low";
    if (want == "normal") return hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess ? 0 : -1;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return -1;
    const int prio = want == "high" ? greatest : least;
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio) == hipSuccess ? 0 : -1;
}
}  // namespace s1rt

// ------------------------------------------------------------ verify queue --
// Three fill/flight sets per queue: while earlier sets' batches are copied
// to the device, hashed and compared, submissions fill the next one.  With
// two, a batch of 1024 chunks had to wait for its set's H2D + kernel (~15
// ms) and the queue topped out near 30 GiB/s (profiles/file_vq_r01.json).
// Set layout (pinned host and device alike): [off u64 x B][len u32 x B]
// [expected 20 x B] pad to 128 | B slots of `stride` bytes; the device side
// adds B x 20 digests and B mismatch bytes.
namespace {
using s1host::pool_copy;
constexpr int kVqSets = 3;

struct VqSet {
    PinBuf h;
    DevBuf d;
    PinBuf res;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    std::vector<uint64_t> tags;
    size_t count = 0;
    bool inflight = false;
};
}  // namespace

struct s1be_vq {
    Pvq* pv = nullptr;  // the persistent drain (default), or null: batch launches (SHA1CHUNK_VQ_MODE=batch)
    int dev = 0;
    int cus = 256;
    size_t batch = 0;  // launch threshold
    size_t cap = 0;    // chunks a set holds: a batch grows up to this while the device is busy
    uint32_t maxlen = 0;
    size_t stride = 0, meta = 0;
    VqSet set[kVqSets];
    int fill = 0;
    std::deque<int> flight;  // launched sets, oldest first
    std::deque<std::pair<uint64_t, uint8_t>> ready;
    size_t pending = 0;
    PartPool* copier = nullptr;
    std::mutex mu;  // every entry point holds it: a queue may be shared by threads
    // batch mode's reservations: buffer -> (length, storage)
    std::unordered_map<void*, std::pair<uint32_t, std::unique_ptr<uint8_t[]>>> reserved;
    // SHA1CHUNK_VQ_STATS=1: per entry point (submit, reserve, commit, release,
    // poll, other) the calls, ns spent waiting for `mu` and ns holding it;
    // printed as one JSON line to stderr by destroy (diagnostics)
    bool stats = false;
    uint64_t st_calls[6] = {}, st_wait_ns[6] = {}, st_hold_ns[6] = {};
};

namespace {

uint64_t* vq_off(s1be_vq*, uint8_t* base) { return reinterpret_cast<uint64_t*>(base); }  // offsets lead the set
uint32_t* vq_len(s1be_vq* q, uint8_t* base) {
    return reinterpret_cast<uint32_t*>(base + q->cap * 8);
}
uint8_t* vq_exp(s1be_vq* q, uint8_t* base) { return base + q->cap * 12; }

int vq_launch(s1be_vq* q, int which) {
    VqSet& S = q->set[which];
    if (S.count == 0) return SHA1CHUNK_OK;
    HIP_TRY(hipSetDevice(q->dev));
    uint8_t* h = static_cast<uint8_t*>(S.h.p);
    uint8_t* d = static_cast<uint8_t*>(S.d.p);
    HIP_TRY(hipMemcpyAsync(d, h, q->meta + S.count * q->stride, hipMemcpyHostToDevice, S.stream));
    uint8_t* ddig = d + q->meta + q->cap * q->stride;
    uint8_t* dmis = ddig + q->cap * 20;
    BatchArgs A{};
    A.base = d;
    A.off = vq_off(q, d);
    A.len = vq_len(q, d);
    A.n = static_cast<uint32_t>(S.count);
    A.dig = ddig;
    int rc = launch_checked(choose_kernel(SHA1CHUNK_KERNEL_AUTO, S.count, q->cus), A, S.stream, q->cus);
    if (rc) return rc;
    hipError_t e = launch_compare(ddig, vq_exp(q, d), static_cast<uint32_t>(S.count), dmis, S.stream);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "compare launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(S.res.p, dmis, S.count, hipMemcpyDeviceToHost, S.stream));
    HIP_TRY(hipEventRecord(S.done, S.stream));
    S.inflight = true;
    q->flight.push_back(which);
    return SHA1CHUNK_OK;
}

// Move the oldest launched set's results to `ready` (blocking on it).
int vq_collect_oldest(s1be_vq* q) {
    if (q->flight.empty()) return SHA1CHUNK_OK;
    const int which = q->flight.front();
    VqSet& S = q->set[which];
    HIP_TRY(hipEventSynchronize(S.done));
    const uint8_t* r = static_cast<const uint8_t*>(S.res.p);
    for (size_t i = 0; i < S.count; ++i) q->ready.emplace_back(S.tags[i], r[i]);
    S.tags.clear();
    S.count = 0;
    S.inflight = false;
    q->flight.pop_front();
    return SHA1CHUNK_OK;
}

// Collect every launched set that has finished, oldest first, without
// blocking.
int vq_reap(s1be_vq* q) {
    while (!q->flight.empty()) {
        hipError_t e = hipEventQuery(q->set[q->flight.front()].done);
        if (e == hipErrorNotReady) break;
        if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "vq: %s", hipGetErrorString(e));
        int rc = vq_collect_oldest(q);
        if (rc) return rc;
    }
    return SHA1CHUNK_OK;
}

// Launch the fill set once it holds `batch` chunks, unless the device is
// busy with kVqSets - 1 earlier sets: then the set keeps growing, a batch at
// a time (up to `cap`), and goes at the first whole batch after one of them
// finishes.  Every launch costs at
// least one chunk's serial hash time (~6 ms), so while the device is busy a
// bigger batch is free throughput; while it is idle, `batch` bounds latency.
int vq_maybe_launch(s1be_vq* q) {
    VqSet& S = q->set[q->fill];
    // only at whole multiples of `batch`: a caller that submits whole batches
    // still gets every result back through non-blocking polls, no flush
    if (S.inflight || S.count < q->batch || S.count % q->batch) return SHA1CHUNK_OK;
    int rc = vq_reap(q);
    if (rc) return rc;
    if (S.count < q->cap && q->flight.size() >= static_cast<size_t>(kVqSets - 1)) return SHA1CHUNK_OK;
    if ((rc = vq_launch(q, q->fill))) return rc;
    q->fill = (q->fill + 1) % kVqSets;
    return SHA1CHUNK_OK;
}

size_t vq_cap(size_t batch) {
    const char* e = getenv("SHA1CHUNK_VQ_GROW");  // 0: launch at exactly `batch`
    if ((e && atoi(e) == 0) || batch >= 512) return batch;
    return std::max(batch, std::min(4 * batch, 512 / batch * batch));  // a multiple of batch
}

// Batch mode has no ring to reserve in: a reservation is a host buffer of
// the queue's, committed by copying (submit) and freed on release.
int vq_batch_submit(s1be_vq* q, const void* chunk, uint32_t len, const uint8_t expected[20], uint64_t tag) {
    if (len > q->maxlen) return fail(SHA1CHUNK_EINVAL, "vq: chunk of %u bytes > max %u", len, q->maxlen);
    VqSet* S = &q->set[q->fill];
    while (S->inflight) {  // the fill set is still on the device: drain in order
        int rc = vq_collect_oldest(q);
        if (rc) return rc;
    }
    if (S->count >= q->cap) {  // only after a failed launch
        int rc = vq_maybe_launch(q);
        if (rc) return rc;
        S = &q->set[q->fill];
        while (S->inflight) {
            if ((rc = vq_collect_oldest(q))) return rc;
        }
    }
    uint8_t* h = static_cast<uint8_t*>(S->h.p);
    const size_t i = S->count;
    vq_off(q, h)[i] = q->meta + i * q->stride;
    vq_len(q, h)[i] = len;
    memcpy(vq_exp(q, h) + 20 * i, expected, 20);
    if (len) pool_copy(*q->copier, h + q->meta + i * q->stride, static_cast<const uint8_t*>(chunk), len);
    S->tags.push_back(tag);
    ++S->count;
    ++q->pending;
    return vq_maybe_launch(q);
}

int vq_batch_flush(s1be_vq* q) {
    if (q->set[q->fill].count == 0 || q->set[q->fill].inflight) return SHA1CHUNK_OK;
    int rc = vq_launch(q, q->fill);
    if (rc) return rc;
    q->fill = (q->fill + 1) % kVqSets;
    return SHA1CHUNK_OK;
}

long vq_batch_poll(s1be_vq* q, uint64_t* tags, uint8_t* mismatch, size_t max, int wait) {
    int rc;
    if (wait) {
        if ((rc = vq_batch_flush(q))) return rc;
        while (!q->flight.empty())
            if ((rc = vq_collect_oldest(q))) return rc;
    } else {
        if ((rc = vq_reap(q))) return rc;
        if ((rc = vq_maybe_launch(q))) return rc;  // a grown batch waiting for the device
    }
    size_t n = 0;
    while (n < max && !q->ready.empty()) {
        tags[n] = q->ready.front().first;
        mismatch[n] = q->ready.front().second;
        q->ready.pop_front();
        ++n;
    }
    q->pending -= n;
    return static_cast<long>(n);
}

}  // namespace

// The backend's queue entry points take and return the queue as void*
// (the front end's handle type); every call holds the queue's lock, so any
// thread may reserve, fill, commit, release and poll on a shared queue.
extern "C" {

void s1be_vq_destroy(void* qv);

void* s1be_vq_create(size_t batch, uint32_t max_chunk_len) {
    if (batch == 0 || batch > (1u << 20) || max_chunk_len == 0) {
        fail(SHA1CHUNK_EINVAL, "vq: batch 1..2^20 and max_chunk_len > 0 required");
        return nullptr;
    }
    Device* D;
    if (get_device(&D)) return nullptr;
    auto* q = new s1be_vq();
    q->dev = D->id;
    q->stats = env_u64("SHA1CHUNK_VQ_STATS", 0) != 0;
    // the persistent drain unless SHA1CHUNK_VQ_MODE=batch (launch per batch)
    // or the device's drain CU budget is spent (then batch launches too)
    const char* mode = getenv("SHA1CHUNK_VQ_MODE");
    const int cus = mode && !strcmp(mode, "batch") ? 0 : drain_cus_take(D);
    if (cus > 0) {
        q->pv = pvq_create(D, batch, max_chunk_len, cus, &q->mu);
        if (!q->pv) {
            delete q;
            return nullptr;
        }
        return q;
    }
    q->cus = D->cus;
    q->batch = batch;
    q->cap = vq_cap(batch);
    q->maxlen = max_chunk_len;
    q->stride = round_up(max_chunk_len, kAlign);
    q->meta = round_up(q->cap * (8 + 4 + 20), kAlign);
    q->copier = new PartPool(vq_copy_helpers(), near_cpus(D->id));
    const size_t hbytes = q->meta + q->cap * q->stride;
    for (auto& S : q->set) {
        if (S.h.ensure(hbytes) || S.d.ensure(hbytes + q->cap * 21) || S.res.ensure(q->cap) ||
            vq_stream_create(&S.stream) != 0 ||
            hipEventCreateWithFlags(&S.done, hipEventDisableTiming) != hipSuccess) {
            if (!*s1be_last_error()) fail(SHA1CHUNK_ENOMEM, "vq: allocation failed");
            s1be_vq_destroy(q);
            return nullptr;
        }
        S.tags.reserve(q->cap);
    }
    return q;
}

enum { kOpSubmit, kOpReserve, kOpCommit, kOpRelease, kOpPoll, kOpOther };
struct VqLock {
    s1be_vq* q;
    int op;
    int64_t t1 = 0;
    VqLock(s1be_vq* q_, int op_) : q(q_), op(op_) {
        if (!q->stats) {
            q->mu.lock();
            return;
        }
        const int64_t t0 = mono_ns();
        q->mu.lock();
        t1 = mono_ns();
        ++q->st_calls[op];
        q->st_wait_ns[op] += static_cast<uint64_t>(t1 - t0);
    }
    ~VqLock() {
        if (q->stats) q->st_hold_ns[op] += static_cast<uint64_t>(mono_ns() - t1);
        q->mu.unlock();
    }
};

void vq_print_stats(const s1be_vq* q) {
    static const char* names[6] = {"submit", "reserve", "commit", "release", "poll", "other"};
    fprintf(stderr, "{\"vq_stats\": {");
    for (int i = 0; i < 6; ++i)
        fprintf(stderr, "\"%s\": [%llu, %.3f, %.3f], ", names[i], (unsigned long long)q->st_calls[i],
                q->st_wait_ns[i] * 1e-6, q->st_hold_ns[i] * 1e-6);
    if (q->pv) pvq_print_stats(q->pv, stderr);
    fprintf(stderr, "\"units\": \"[calls, ms waiting for the lock, ms holding it]\"}}\n");
}

int s1be_vq_submit(void* qv, const void* chunk, uint32_t len, const uint8_t expected[20], uint64_t tag) {
    auto* q = static_cast<s1be_vq*>(qv);
    if (!q || (len && !chunk) || !expected) return fail(SHA1CHUNK_EINVAL, "vq: null argument");
    VqLock lk(q, kOpSubmit);
    if (q->pv) {
        if (len > pvq_max_len(q->pv))
            return fail(SHA1CHUNK_EINVAL, "vq: chunk of %u bytes > max %u", len, pvq_max_len(q->pv));
        return pvq_submit(q->pv, chunk, len, expected, tag);
    }
    return vq_batch_submit(q, chunk, len, expected, tag);
}

void* s1be_vq_reserve(void* qv, uint32_t len) {
    auto* q = static_cast<s1be_vq*>(qv);
    if (!q) {
        fail(SHA1CHUNK_EINVAL, "vq: null queue");
        return nullptr;
    }
    VqLock lk(q, kOpReserve);
    const uint32_t maxlen = q->pv ? pvq_max_len(q->pv) : q->maxlen;
    if (len > maxlen) {
        fail(SHA1CHUNK_EINVAL, "vq: reservation of %u bytes > max %u", len, maxlen);
        return nullptr;
    }
    if (q->pv) return pvq_reserve(q->pv, len);
    auto buf = std::unique_ptr<uint8_t[]>(new (std::nothrow) uint8_t[std::max<uint32_t>(len, 1)]);
    if (!buf) {
        fail(SHA1CHUNK_ENOMEM, "vq: reservation of %u bytes", len);
        return nullptr;
    }
    void* p = buf.get();
    q->reserved.emplace(p, std::make_pair(len, std::move(buf)));
    return p;
}

int s1be_vq_commit(void* qv, void* buf, uint32_t len, const uint8_t expected[20], uint64_t tag) {
    auto* q = static_cast<s1be_vq*>(qv);
    if (!q || !buf || !expected) return fail(SHA1CHUNK_EINVAL, "vq: null argument");
    VqLock lk(q, kOpCommit);
    if (q->pv) return pvq_commit(q->pv, buf, len, expected, tag);
    auto it = q->reserved.find(buf);
    if (it == q->reserved.end()) return fail(SHA1CHUNK_EINVAL, "vq: %p is not a reserved buffer", buf);
    if (len > it->second.first)
        return fail(SHA1CHUNK_EINVAL, "vq: commit of %u bytes into a %u-byte reservation", len, it->second.first);
    return vq_batch_submit(q, buf, len, expected, tag);
}

int s1be_vq_release(void* qv, void* buf) {
    auto* q = static_cast<s1be_vq*>(qv);
    if (!q || !buf) return fail(SHA1CHUNK_EINVAL, "vq: null argument");
    VqLock lk(q, kOpRelease);
    if (q->pv) return pvq_release(q->pv, buf);
    if (!q->reserved.erase(buf)) return fail(SHA1CHUNK_EINVAL, "vq: %p is not a reserved buffer", buf);
    return SHA1CHUNK_OK;
}

int s1be_vq_flush(void* qv) {
    auto* q = static_cast<s1be_vq*>(qv);
    if (!q) return fail(SHA1CHUNK_EINVAL, "vq: null queue");
    VqLock lk(q, kOpOther);
    return q->pv ? pvq_publish(q->pv) : vq_batch_flush(q);
}

long s1be_vq_poll(void* qv, uint64_t* tags, uint8_t* mismatch, size_t max, int wait) {
    auto* q = static_cast<s1be_vq*>(qv);
    if (!q || (max && (!tags || !mismatch))) return fail(SHA1CHUNK_EINVAL, "vq: null argument");
    VqLock lk(q, kOpPoll);
    return q->pv ? pvq_poll(q->pv, tags, mismatch, max, wait) : vq_batch_poll(q, tags, mismatch, max, wait);
}

size_t s1be_vq_pending(const void* qv) {
    auto* q = static_cast<s1be_vq*>(const_cast<void*>(qv));
    if (!q) return 0;
    VqLock lk(q, kOpOther);
    return q->pv ? pvq_pending(q->pv) : q->pending;
}

void s1be_vq_destroy(void* qv) {
    auto* q = static_cast<s1be_vq*>(qv);
    if (!q) return;
    if (q->stats) vq_print_stats(q);
    if (q->pv) {
        pvq_destroy(q->pv);
        delete q;
        return;
    }
    (void)hipSetDevice(q->dev);
    for (auto& S : q->set) {
        if (S.stream) (void)hipStreamSynchronize(S.stream);
        if (S.done) (void)hipEventDestroy(S.done);
        if (S.stream) (void)hipStreamDestroy(S.stream);
        if (S.h.p) (void)hipHostFree(S.h.p);
        if (S.res.p) (void)hipHostFree(S.res.p);
        if (S.d.p) (void)hipFree(S.d.p);
    }
    delete q->copier;
    delete q;
}

}  // extern "C"
