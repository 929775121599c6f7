// vq_persistent.hip -- the verify queue's default mode: a persistent drain
// kernel fed through rings in pinned host memory (interface:
// vq_persistent.hpp; the queue object and the s1be_vq_* entry points: vq.hip).
// Also the process-wide state that outlives a queue: the caches of pinned and
// device rings, and the list of live queues the exit handler stops.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <emmintrin.h>
#include <mutex>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "vq_persistent.hpp"

using namespace s1rt;

namespace {
using s1host::pool_copy;

// ------------------------------------------------ persistent verify queue --
// s1be_vq with a persistent drain kernel (sha1_vq_drain_kernel): the
// host copies each submitted chunk into a ring in pinned, uncached host
// memory, writes its length and expected digest next to it, and publishes
// groups of up to 64 chunks by bumping `pub`.  The drain -- one workgroup
// per CU on SHA1CHUNK_VQ_CUS CUs, (re)launched whenever work is published
// and fewer of its workgroups are alive than that, gone again after
// SHA1CHUNK_VQ_IDLE_MS (default 20) without a claim -- reads the ring over
// PCIe, hashes each group in the one-group split shape and writes
// one 0/1 per chunk plus the group's completion word back to host memory.
// No copy engine, no launch per batch: a chunk starts hashing as soon as
// its group is published.  A group is published when it holds
// min(batch, 64) chunks, or at once while fewer groups are in flight than
// the drain has workgroups (so at low rates every chunk goes alone and comes
// back after its own serial chain, ~6 ms for 512 KiB, whatever the batch
// size).  The drain takes SHA1CHUNK_VQ_CUS CUs (default 64 of 256): the
// queue is PCIe-bound (64 groups of 64 chunks in flight are far more than
// the link feeds), and the rest of the GPU stays free for the process's
// other kernels, which could not share a CU with a drain workgroup (it holds
// the CU's whole LDS).
// Positions in both rings are monotonic counters (physical = counter mod
// ring size).  A group is a run of consecutive slots that never wraps the
// slot ring; each slot points at its chunk's region of the data ring, a
// region never wraps the data ring, and regions are freed in allocation
// order (the data ring's head is the oldest region still held).
// Zero-copy receive (sha1chunk_vq_reserve / commit / release): the caller
// fills a region in place -- the peer's session buffer (reliable_udp.c:121,
// filled at :339) -- and commits it, which gives it a slot; the region stays
// the caller's after its result is collected, until the caller releases it
// (after copying the verified chunk into its job buffer, reliable_udp.c:
// 696-709).  A submitted (copied) chunk's region is freed when its result
// is collected.
constexpr uint32_t kPvqMaxGroup = 64;
struct PvqCtl {
    uint32_t pub;        // groups published (host store, release)
    uint32_t stop;       // destroy: exit once nothing is claimable
    uint32_t last_done;  // drain: index + 1 of the group it finished last
    uint32_t pad[29];
    uint8_t alive[2][1024];   // per launch slot, per workgroup (bytes: 16 per uncached read)
};
struct PvqGroup {
    uint64_t g;         // group index
    uint64_t slot0;     // first slot (monotonic)
    uint32_t count;
    bool collected;
};
// A byte range of the data ring [start, end) (monotonic positions).
struct PvqRegion {
    uint64_t start, end;
    bool reserved;   // handed out by reserve(): freed by release()
    bool committed;  // a slot refers to it: its result is pending until collected
    bool collected;
    bool released;
    std::thread::id owner;  // the thread that allocated it (reserve or submit)
    bool polled = false;    // poll() handed its result out: what is left is its owner's release()
};
// A collected result waiting for poll(), with its region's id (a copied
// chunk's region may be freed, its id below reg_base, before the result is
// popped).
struct PvqResult {
    uint64_t tag;
    uint8_t mismatch;
    uint64_t region;
};
}  // namespace

namespace s1rt {
struct Pvq {
    int dev = 0, cus = 256;  // cus: the drain's workgroups (one per CU)
    uint32_t nslots = 0;  // slot ring (chunks) = group ring entries
    uint64_t nbytes = 0;  // data ring bytes
    uint32_t maxlen = 0;
    uint32_t group_max = kPvqMaxGroup;
    uint64_t idle_ticks = 0, life_ticks = 0;
    // pinned, uncached host memory: data ring, then the per-slot and
    // per-group arrays, then the control words
    uint8_t* hmem = nullptr;
    uint8_t* data = nullptr;
    uint64_t* off = nullptr;
    uint32_t* grp = nullptr;
    uint32_t* len = nullptr;
    uint32_t* done = nullptr;
    uint8_t* exp = nullptr;
    uint8_t* res = nullptr;
    PvqCtl* ctl = nullptr;
    // device memory: digest scratch + the claim counter
    uint8_t* dmem = nullptr;
    std::vector<uint64_t> tags;
    std::vector<uint64_t> slot_reg;  // per slot: its region's id
    std::deque<PvqRegion> regions;   // allocated, not yet freed, oldest first
    uint64_t reg_base = 0;           // id of regions.front()
    std::unordered_map<uint64_t, uint64_t> held;  // reserved regions not released: ring offset -> id
    uint64_t slot_head = 0, slot_tail = 0, byte_head = 0, byte_tail = 0;
    uint32_t seen_done = 0;  // ctl->last_done at the last scan
    std::mutex* mu = nullptr;  // the queue's lock (held by every caller; pvq_wait drops it to sleep)
    std::mutex copy_mu;        // the copy helpers run one submit's copy at a time
    // counters for SHA1CHUNK_VQ_STATS
    uint64_t n_publish = 0, n_published = 0, n_copies = 0, n_launch = 0, n_scans = 0, n_sleeps = 0;
    std::atomic<uint64_t> copy_ns{0};  // submit's copies (outside the lock), all threads
    uint64_t sleep_ns = 0;             // pvq_wait's sleeps (lock dropped), all threads
    int64_t alive_scan_ns = 0;  // pvq_ensure_drain: when it last read the alive words
    int alive_seen = 0;         // and how many it found (or launched)
    uint64_t open_slot0 = 0;
    uint32_t open_count = 0;
    uint64_t next_g = 0;
    std::deque<PvqGroup> groups;  // published, oldest first
    size_t inflight = 0;          // published, not yet collected
    std::deque<PvqResult> ready;
    size_t pending = 0;
    // two launch slots, each a stream, an alive-word set and the event of
    // its last drain; a slot is reused only once that drain has ended
    hipStream_t stream[2] = {nullptr, nullptr};
    hipEvent_t ended[2] = {nullptr, nullptr};
    bool launched[2] = {false, false};
    PartPool* copier = nullptr;
    size_t hbytes = 0;
    unsigned hflags = 0;
    int budget_dev = -1;  // device whose drain CU budget this queue holds (pvq_create)
    // DMA staging (default since round 4; SHA1CHUNK_VQ_DMA=0 turns it off):
    // the data ring lives in ordinary pinned host memory (`hdata`), each
    // published group's chunks are copied by the copy engine into a device
    // mirror of the ring (`ddata`, uncached device memory, the drain reads it
    // from HBM), and the group is released to the drain (`pub`) once its copy
    // event has completed.  The drain reading the ring over PCIe tops out at
    // 26-28 GiB/s (8 receive threads, zero-copy), the copy engine at 37-45
    // (profiles/vq_dma_r04.jsonl, vq_dma_knobs_r04.log).
    bool dma = false;
    uint8_t* hdata = nullptr;
    size_t hdata_bytes = 0;
    uint8_t* ddata = nullptr;
    hipStream_t cstream = nullptr;
    std::deque<std::pair<uint64_t, hipEvent_t>> staged;  // group, its copies' event
    std::vector<hipEvent_t> spare_events;
};
}  // namespace s1rt

namespace {
int pvq_launch(Pvq* P, int k, int wgs) {
    // every workgroup of the new drain counts as alive from here on, so a
    // submit right after does not launch another one
    for (int w = 0; w < wgs; ++w) __atomic_store_n(&P->ctl->alive[k][w], uint8_t{1}, __ATOMIC_RELEASE);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    VqDrainArgs Q{};
    Q.data = P->dma ? P->ddata : P->data;
    Q.off = P->off;
    Q.len = P->len;
    Q.exp = P->exp;
    Q.grp = P->grp;
    Q.pub = &P->ctl->pub;
    Q.stop = &P->ctl->stop;
    Q.alive = P->ctl->alive[k];
    Q.res = P->res;
    Q.done = P->done;
    Q.last_done = &P->ctl->last_done;
    Q.dig = P->dmem;
    Q.claim = reinterpret_cast<uint32_t*>(P->dmem + 20ull * P->nslots);
    Q.grp_ring = P->nslots;
    Q.idle_ticks = P->idle_ticks;
    Q.life_ticks = P->life_ticks;
    HIP_TRY(hipSetDevice(P->dev));
    hipError_t e = launch_vq_drain(Q, static_cast<uint32_t>(wgs), P->stream[k]);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "vq drain launch: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(P->ended[k], P->stream[k]));
    P->launched[k] = true;
    ++P->n_launch;
    return SHA1CHUNK_OK;
}

// After `pub` moved (and while waiting): keep the drain at full strength.
// Workgroups leave when they find nothing to claim, each with the exit
// handshake of sha1_kernels.hip (so no published group is left without a
// live workgroup that sees it), and after their lifetime even under load
// (SHA1CHUNK_VQ_LIFE_MS, so that no drain holds its hardware queue for
// good); the latter relies on this call, which every submit, commit and
// poll makes while groups are in flight.  When fewer than the drain's
// workgroups are alive, the missing ones are launched on a slot whose
// previous drain has ended; the leftovers of the old one keep working.
//
// The alive flags are uncached host memory (a CPU read costs ~0.15 us, and
// every submit, commit and poll lands here under the queue's lock), so they
// are bytes read 16 at a time -- 8 reads for a 64-workgroup drain's two
// launch slots -- and a call that did not move `pub` does not read them again
// within kAliveScanNs of a scan that found the drain at full strength: a
// workgroup that leaves in that window is replaced at most that much later
// (workgroups live >= 4 ms), and the next publish rescans anyway.  A call
// that moved `pub` (publish, or a DMA-staged group released) always reads
// them: that read is the host's half of the exit handshake, so
// a group published just as the drain's last workgroups leave is never left
// unclaimed until some later call.
constexpr int64_t kAliveScanNs = 50000;

int count_alive(const uint8_t* a, int n) {
    int c = 0, w = 0;
    for (; w + 16 <= n; w += 16) {  // one 16-byte uncached read per 16 flags
        const __m128i v = _mm_load_si128(reinterpret_cast<const __m128i*>(a + w));
        c += 16 - __builtin_popcount(_mm_movemask_epi8(_mm_cmpeq_epi8(v, _mm_setzero_si128())));
    }
    for (; w < n; ++w) c += __atomic_load_n(a + w, __ATOMIC_ACQUIRE) != 0;
    return c;
}

int pvq_ensure_drain(Pvq* P, bool moved_pub = false) {
    const int64_t now = mono_ns();
    if (!moved_pub && P->alive_seen >= P->cus && now - P->alive_scan_ns < kAliveScanNs) return SHA1CHUNK_OK;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    int alive = 0;
    for (int k = 0; k < 2; ++k)  // a slot never launched has no live workgroup
        if (P->launched[k]) alive += count_alive(P->ctl->alive[k], P->cus);
    ++P->n_scans;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    P->alive_scan_ns = now;
    P->alive_seen = alive;
    if (alive >= P->cus) return SHA1CHUNK_OK;
    for (int k = 0; k < 2; ++k) {
        if (P->launched[k]) {
            const hipError_t q = hipEventQuery(P->ended[k]);
            if (q == hipErrorNotReady) continue;
            if (q != hipSuccess) return fail(SHA1CHUNK_EHIP, "vq drain: %s", hipGetErrorString(q));
        }
        P->alive_seen = P->cus;  // pvq_launch marks the new workgroups alive
        return pvq_launch(P, k, P->cus - alive);
    }
    return SHA1CHUNK_OK;  // both slots' drains still leaving: the next call launches
}

// DMA staging: release every staged group whose copies have landed, in
// order (the copy stream completes them in order), to the drain.
int pvq_release_staged(Pvq* P) {
    bool moved = false;
    while (!P->staged.empty()) {
        const hipError_t q = hipEventQuery(P->staged.front().second);
        if (q == hipErrorNotReady) break;
        if (q != hipSuccess) return fail(SHA1CHUNK_EHIP, "vq copy: %s", hipGetErrorString(q));
        __atomic_store_n(&P->ctl->pub, static_cast<uint32_t>(P->staged.front().first + 1), __ATOMIC_RELEASE);
        P->spare_events.push_back(P->staged.front().second);
        P->staged.pop_front();
        moved = true;
    }
    return moved ? pvq_ensure_drain(P, true) : SHA1CHUNK_OK;
}

// Copy the chunks of slots [slot0, slot0 + count) into the device ring and
// record the group's event.  Receive threads commit in their own order, so a
// group's regions are sorted by ring offset and copied as runs, a run taking
// in gaps of up to kStageGap bytes: one 512 KiB copy runs at ~30 GiB/s on the
// copy engine (15-19 us, profiles), a run of many at the link's rate.  A
// gap's bytes are other reservations' (filling, committed or free): their
// device copy is rewritten with the same or later bytes before any group
// that holds them is released to the drain, and none of them is in a group
// the drain is hashing unless committed (whose bytes no longer change).
constexpr uint64_t kStageGap = 1ull << 20;

int pvq_stage(Pvq* P, uint64_t g, uint64_t slot0, uint32_t count) {
    HIP_TRY(hipSetDevice(P->dev));
    std::pair<uint64_t, uint64_t> rg[kPvqMaxGroup];  // (ring offset, end)
    uint32_t n = 0;
    for (uint32_t j = 0; j < count && n < kPvqMaxGroup; ++j) {
        const PvqRegion& r = P->regions[P->slot_reg[(slot0 + j) % P->nslots] - P->reg_base];
        const uint64_t at = r.start % P->nbytes;
        rg[n++] = {at, at + (r.end - r.start)};
    }
    std::sort(rg, rg + n);
    for (uint32_t i = 0; i < n;) {
        uint64_t run_at = rg[i].first, run_end = rg[i].second;
        for (++i; i < n && rg[i].first <= run_end + kStageGap; ++i) run_end = std::max(run_end, rg[i].second);
        HIP_TRY(hipMemcpyAsync(P->ddata + run_at, P->hdata + run_at, run_end - run_at, hipMemcpyHostToDevice,
                               P->cstream));
        ++P->n_copies;
    }
    hipEvent_t ev;
    if (!P->spare_events.empty()) {
        ev = P->spare_events.back();
        P->spare_events.pop_back();
    } else {
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(ev, P->cstream));
    P->staged.emplace_back(g, ev);
    return SHA1CHUNK_OK;
}
}  // namespace

namespace s1rt {
int pvq_publish(Pvq* P) {
    if (P->open_count == 0) return SHA1CHUNK_OK;
    // the drain indexes a group's slots first..first+count with no modulo
    if (P->open_slot0 % P->nslots + P->open_count > P->nslots || P->open_count > kPvqMaxGroup)
        return fail(SHA1CHUNK_EHIP, "vq: internal: group of %u slots at %llu crosses the slot ring's end",
                    P->open_count, static_cast<unsigned long long>(P->open_slot0 % P->nslots));
    const uint64_t g = P->next_g++;
    const uint32_t gi = static_cast<uint32_t>(g % P->nslots);
    P->grp[2 * gi] = static_cast<uint32_t>(P->open_slot0 % P->nslots);
    P->grp[2 * gi + 1] = P->open_count;
    P->groups.push_back(PvqGroup{g, P->open_slot0, P->open_count, false});
    ++P->inflight;
    const uint64_t slot0 = P->open_slot0;
    const uint32_t count = P->open_count;
    ++P->n_publish;
    P->n_published += count;
    P->open_slot0 = P->slot_tail;
    P->open_count = 0;
    if (P->dma) {
        // released to the drain once its copies land (pvq_release_staged)
        if (int rc = pvq_stage(P, g, slot0, count)) return rc;
        return pvq_release_staged(P);
    }
    // the group's bytes, lengths, digests and descriptor are written: release them
    __atomic_store_n(&P->ctl->pub, static_cast<uint32_t>(g + 1), __ATOMIC_RELEASE);
    return pvq_ensure_drain(P, true);
}
}  // namespace s1rt

namespace {
// A region is free once nothing refers to it: a copied chunk once its
// result is collected; a reserved one once the caller released it and its
// result (if it was committed) is collected.
bool region_free(const PvqRegion& r) {
    if (!r.reserved) return r.collected;
    return r.released && (r.collected || !r.committed);
}

// Free the oldest regions that are free; the data ring's head follows.
void pvq_free_regions(Pvq* P) {
    while (!P->regions.empty() && region_free(P->regions.front())) {
        P->regions.pop_front();
        ++P->reg_base;
    }
    P->byte_head = P->regions.empty() ? P->byte_tail : P->regions.front().start;
}

// Collect finished groups (in any order) and free ring space up to the
// oldest unfinished one.  The drain claims groups in publication order and
// runs at most one per CU at a time, so the scan stops after 2 x CUs
// unfinished groups in a row: a submit costs O(CUs), not O(groups in flight).
int pvq_reap(Pvq* P) {
    if (P->dma && !P->staged.empty())
        if (int rc = pvq_release_staged(P)) return rc;
    // The completion words live in uncached host memory (~0.1-0.2 us per
    // CPU read); every submit, reserve and commit reaps, so scan them only
    // when the drain's last-finished word moved since the last scan (each
    // group writes its own index there, so the word changes whenever any
    // group finished).
    const uint32_t ld = __atomic_load_n(&P->ctl->last_done, __ATOMIC_ACQUIRE);
    if (ld == P->seen_done) return SHA1CHUNK_OK;
    bool whole = true;  // the scan reached the end (else scan again next time)
    size_t unfinished = 0;
    for (auto& G : P->groups) {
        if (G.collected) continue;
        const uint32_t gi = static_cast<uint32_t>(G.g % P->nslots);
        if (__atomic_load_n(&P->done[gi], __ATOMIC_ACQUIRE) != static_cast<uint32_t>(G.g + 1)) {
            if (++unfinished > 2 * static_cast<size_t>(P->cus)) {
                whole = false;
                break;
            }
            continue;
        }
        unfinished = 0;
        for (uint32_t j = 0; j < G.count; ++j) {
            const uint64_t sl = (G.slot0 + j) % P->nslots;
            P->ready.push_back(PvqResult{P->tags[sl], P->res[sl], P->slot_reg[sl]});
            P->regions[P->slot_reg[sl] - P->reg_base].collected = true;
        }
        G.collected = true;
        --P->inflight;
    }
    while (!P->groups.empty() && P->groups.front().collected) {
        P->slot_head = P->groups.front().slot0 + P->groups.front().count;
        P->groups.pop_front();
    }
    if (P->groups.empty()) P->slot_head = P->open_slot0;
    if (whole) P->seen_done = ld;
    pvq_free_regions(P);
    return SHA1CHUNK_OK;
}

// Wait (bounded) until `pred` holds, reaping and keeping a drain alive.
// An open group is published first (its chunks hold ring space too), and a
// wait that only the caller can end -- the oldest region of the data ring
// is a reserved buffer not yet committed, or collected and not released --
// fails at once when `stuck(false)` says so.  When the bound runs out,
// `stuck(true)` may still name a caller's buffer as what holds the room
// (ENOMEM); otherwise the drain is what did not progress (EHIP).
// Bound on any one wait (SHA1CHUNK_VQ_WAIT_S, default 120 s).
std::chrono::seconds pvq_wait_bound() {
    static const std::chrono::seconds b(std::max<uint64_t>(1, env_u64("SHA1CHUNK_VQ_WAIT_S", 120)));
    return b;
}

template <typename Pred, typename Stuck>
int pvq_wait(Pvq* P, Pred pred, const char* what, Stuck stuck) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    for (;;) {
        if ((rc = pvq_reap(P))) return rc;
        if (pred()) return SHA1CHUNK_OK;
        if (P->open_count && (rc = pvq_publish(P))) return rc;
        const bool expired = std::chrono::steady_clock::now() - t0 > pvq_wait_bound();
        if (const char* why = stuck(expired))
            return fail(SHA1CHUNK_ENOMEM, "vq: %s: the ring's oldest region is %s (%zu reserved buffers held)", what,
                        why, P->held.size());
        if (P->inflight && (rc = pvq_ensure_drain(P))) return rc;
        if (expired) return fail(SHA1CHUNK_EHIP, "vq: %s timed out (drain not progressing)", what);
        ++P->n_sleeps;
        // sleep without the queue's lock: the other threads' commits, polls
        // and releases are what frees the ring (each call re-checks its state
        // after the wait)
        const int64_t z0 = mono_ns();
        if (P->mu) P->mu->unlock();
        std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (P->mu) P->mu->lock();
        P->sleep_ns += static_cast<uint64_t>(mono_ns() - z0);
    }
}
template <typename Pred>
int pvq_wait(Pvq* P, Pred pred, const char* what) {
    return pvq_wait(P, pred, what, [](bool) { return static_cast<const char*>(nullptr); });
}

// Queues alive at process exit (a caller that never destroys its queue):
// an exit handler raises every live drain's stop word and waits for its
// launches, so no drain wave is still polling the pinned ring when the
// runtime and the process's mappings go away.  The handler is registered at
// the first queue, after HIP's own start-up, so it runs before HIP's
// teardown (exit handlers run in reverse order).
std::mutex g_pvq_mu;
std::vector<Pvq*>* g_pvq_live = nullptr;
void pvq_stop_all_at_exit();
void pvq_track(Pvq* P, bool add) {
    std::lock_guard<std::mutex> lk(g_pvq_mu);
    if (!g_pvq_live) {
        if (!add) return;
        g_pvq_live = new std::vector<Pvq*>();
        std::atexit(pvq_stop_all_at_exit);
    }
    auto& v = *g_pvq_live;
    if (add)
        v.push_back(P);
    else
        v.erase(std::remove(v.begin(), v.end(), P), v.end());
}

// Pinned rings of destroyed queues, kept for the next queue of the same
// size: hipHostFree (like hipFree) can wait for the whole device, i.e. for
// other threads' busy drains, so a queue's destroy never frees its ring.
std::mutex g_ring_mu;
std::vector<std::tuple<uint8_t*, size_t, unsigned>> g_ring_cache;
constexpr size_t kRingCacheMax = 8;

uint8_t* ring_get(size_t bytes, unsigned flags) {
    {
        std::lock_guard<std::mutex> lk(g_ring_mu);
        for (size_t i = 0; i < g_ring_cache.size(); ++i)
            if (std::get<1>(g_ring_cache[i]) == bytes && std::get<2>(g_ring_cache[i]) == flags) {
                uint8_t* p = std::get<0>(g_ring_cache[i]);
                g_ring_cache.erase(g_ring_cache.begin() + i);
                return p;
            }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, flags) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<uint8_t*>(p);
}

void ring_put(uint8_t* p, size_t bytes, unsigned flags) {
    std::lock_guard<std::mutex> lk(g_ring_mu);
    if (g_ring_cache.size() < kRingCacheMax) {
        g_ring_cache.emplace_back(p, bytes, flags);
        return;
    }
    (void)hipHostFree(p);  // beyond the cache: rare (more than kRingCacheMax queues destroyed at once)
}

// Device mirrors of DMA-staged rings, kept like the pinned rings (hipFree
// can wait for the whole device).
std::vector<std::tuple<int, uint8_t*, size_t>> g_dring_cache;

uint8_t* dring_get(int dev, size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(g_ring_mu);
        for (size_t i = 0; i < g_dring_cache.size(); ++i)
            if (std::get<0>(g_dring_cache[i]) == dev && std::get<2>(g_dring_cache[i]) == bytes) {
                uint8_t* p = std::get<1>(g_dring_cache[i]);
                g_dring_cache.erase(g_dring_cache.begin() + i);
                return p;
            }
    }
    void* p = nullptr;
    // uncached device memory: the drain's loads go to HBM, never to an L2
    // line left from the ring's previous lap (the copy engine does not
    // invalidate the XCDs' L2)
    if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<uint8_t*>(p);
}

void dring_put(int dev, uint8_t* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_ring_mu);
    if (g_dring_cache.size() < kRingCacheMax) {
        g_dring_cache.emplace_back(dev, p, bytes);
        return;
    }
    (void)hipFree(p);
}

// The device's logical index for D (the CU budget lives there).
int device_index(Device* D) { return static_cast<int>(D - g_dev); }
}  // namespace

namespace s1rt {
void pvq_destroy(Pvq* P) {
    if (!P) return;
    pvq_track(P, false);
    (void)hipSetDevice(P->dev);
    if (P->ctl) {
        __atomic_store_n(&P->ctl->stop, 1u, __ATOMIC_RELEASE);
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
    }
    // Wait for this queue's own work only (never the whole device): both
    // drain slots and the copy stream.  The device scratch (claim counter,
    // digests) is freed only after both drains have ended -- a drain still
    // running on slot 1 would otherwise write into memory the pool already
    // handed to the next queue.
    for (int k = 0; k < 2; ++k)
        if (P->stream[k]) (void)hipStreamSynchronize(P->stream[k]);
    if (P->cstream) {
        (void)hipStreamSynchronize(P->cstream);
        (void)hipStreamDestroy(P->cstream);
    }
    if (P->dmem && P->stream[0]) {
        (void)hipFreeAsync(P->dmem, P->stream[0]);
        (void)hipStreamSynchronize(P->stream[0]);
    }
    for (auto& st : P->staged) (void)hipEventDestroy(st.second);
    for (hipEvent_t ev : P->spare_events) (void)hipEventDestroy(ev);
    if (P->hdata) ring_put(P->hdata, P->hdata_bytes, hipHostMallocDefault);
    if (P->ddata) dring_put(P->dev, P->ddata, P->nbytes);
    for (int k = 0; k < 2; ++k) {
        if (P->ended[k]) (void)hipEventDestroy(P->ended[k]);
        if (P->stream[k]) (void)hipStreamDestroy(P->stream[k]);
    }
    if (P->hmem) ring_put(P->hmem, P->hbytes, P->hflags);
    drain_cus_give(P->budget_dev, P->cus);
    delete P->copier;
    delete P;
}

Pvq* pvq_create(Device* D, size_t batch, uint32_t max_chunk_len, int cus, std::mutex* mu) {
    auto* P = new Pvq();
    P->mu = mu;
    P->dev = D->id;
    P->cus = cus;
    P->budget_dev = device_index(D);
    P->maxlen = max_chunk_len;
    P->group_max = static_cast<uint32_t>(std::min<size_t>(batch, kPvqMaxGroup));
    P->idle_ticks = env_u64("SHA1CHUNK_VQ_IDLE_MS", 20) * 100000ull;  // s_memrealtime: 100 MHz
    P->life_ticks = std::max<uint64_t>(1, env_u64("SHA1CHUNK_VQ_LIFE_MS", 4)) * 100000ull;
    const uint64_t stride = round_up(max_chunk_len, kAlign);
    const uint64_t ring_mib = std::max<uint64_t>(env_u64("SHA1CHUNK_VQ_RING_MIB", 1024), 1);
    P->nbytes = round_up(std::max<uint64_t>(ring_mib << 20, 2 * kPvqMaxGroup * stride), kAlign);
    // slots: room for the ring's bytes in chunks of a quarter of the max length
    P->nslots = static_cast<uint32_t>(std::min<uint64_t>(
        std::max<uint64_t>(P->nbytes / std::max<uint64_t>(kAlign, stride / 4), 4 * kPvqMaxGroup), 1u << 20));
    const size_t ns = P->nslots;
    const size_t meta = round_up(ns * 45, 4096);  // off 8, grp 8, len 4, done 4, exp 20, res 1
    // with DMA staging the data ring is ordinary (cached) pinned memory of its
    // own, read only by the copy engine; the slot arrays and control words
    // stay in uncached memory the drain polls
    P->dma = env_u64("SHA1CHUNK_VQ_DMA", 1) != 0;
    const size_t inline_data = P->dma ? 0 : P->nbytes;
    P->hbytes = inline_data + meta + sizeof(PvqCtl);
    P->hflags = ring_flags();
    if (!(P->hmem = ring_get(P->hbytes, P->hflags)) &&
        (P->hflags == hipHostMallocCoherent ||
         !(P->hmem = ring_get(P->hbytes, P->hflags = hipHostMallocCoherent)))) {
        fail(SHA1CHUNK_ENOMEM, "vq: pinned ring of %zu bytes", P->hbytes);
        pvq_destroy(P);
        return nullptr;
    }
    if (P->dma) {
        P->hdata_bytes = P->nbytes;
        if (!(P->hdata = ring_get(P->nbytes, hipHostMallocDefault)) || !(P->ddata = dring_get(P->dev, P->nbytes)) ||
            vq_stream_create(&P->cstream) != 0) {
            (void)hipGetLastError();
            fail(SHA1CHUNK_ENOMEM, "vq: DMA-staged ring of %llu bytes", static_cast<unsigned long long>(P->nbytes));
            pvq_destroy(P);
            return nullptr;
        }
    }
    memset(P->hmem + inline_data, 0, meta + sizeof(PvqCtl));
    uint8_t* m = P->hmem + inline_data;
    P->data = P->dma ? P->hdata : P->hmem;
    P->off = reinterpret_cast<uint64_t*>(m);
    P->grp = reinterpret_cast<uint32_t*>(m + ns * 8);
    P->len = reinterpret_cast<uint32_t*>(m + ns * 16);
    P->done = reinterpret_cast<uint32_t*>(m + ns * 20);
    P->exp = m + ns * 24;
    P->res = m + ns * 44;
    P->ctl = reinterpret_cast<PvqCtl*>(P->hmem + inline_data + meta);
    P->tags.assign(ns, 0);
    P->slot_reg.assign(ns, 0);
    // streams first: the device scratch is allocated and cleared in stream
    // order on stream 0, so creating a queue never waits for the whole device
    // (other threads' drains and batches)
    for (int k = 0; k < 2; ++k)
        if (vq_stream_create(&P->stream[k]) != 0 ||
            hipEventCreateWithFlags(&P->ended[k], hipEventDisableTiming) != hipSuccess) {
            fail(SHA1CHUNK_EHIP, "vq: stream creation");
            pvq_destroy(P);
            return nullptr;
        }
    if (hipMallocAsync(reinterpret_cast<void**>(&P->dmem), 20ull * ns + 256, P->stream[0]) != hipSuccess ||
        hipMemsetAsync(P->dmem + 20ull * ns, 0, 256, P->stream[0]) != hipSuccess ||
        hipStreamSynchronize(P->stream[0]) != hipSuccess) {
        (void)hipGetLastError();
        fail(SHA1CHUNK_ENOMEM, "vq: device scratch");
        pvq_destroy(P);
        return nullptr;
    }
    P->copier = new PartPool(vq_copy_helpers(), near_cpus(P->dev));
    pvq_track(P, true);
    return P;
}
}  // namespace s1rt

namespace {
void pvq_stop_all_at_exit() {
    std::lock_guard<std::mutex> lk(g_pvq_mu);
    if (!g_pvq_live) return;
    for (Pvq* P : *g_pvq_live)
        if (P->ctl) __atomic_store_n(&P->ctl->stop, 1u, __ATOMIC_RELEASE);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    for (Pvq* P : *g_pvq_live) {
        (void)hipSetDevice(P->dev);
        for (int k = 0; k < 2; ++k)
            if (P->stream[k]) (void)hipStreamSynchronize(P->stream[k]);
    }
}

// Room for `len` bytes in the data ring (a region never wraps it): a bounded
// wait while in-flight groups can free space.  Returns the new region's id.
constexpr auto kHeldResultWait = std::chrono::milliseconds(2);
int pvq_alloc(Pvq* P, uint32_t len, bool reserved, uint64_t* id) {
    const uint64_t need = round_up(std::max<uint32_t>(len, 1), kAlign);
    auto pos = [&] {
        const uint64_t t = P->byte_tail;
        return (t % P->nbytes) + need > P->nbytes ? t + (P->nbytes - t % P->nbytes) : t;
    };
    // The wait is hopeless when the ring's head is
    //  * the caller's own reservation, not committed (this thread cannot
    //    commit it while it waits here), or
    //  * the caller's own verified buffer, not released, its result polled
    //    or not (this thread cannot release it while it waits here), or
    //  * another thread's verified buffer whose result is still unpolled:
    //    only a poll() that hands out the result and the release() after it
    //    free that room.  When every receive thread sits in reserve() nobody
    //    polls, so after a short grace (another thread may be polling and
    //    releasing right now) the call fails and its caller polls and
    //    releases (round 6: four receive threads all waiting here stalled for
    //    the whole 120 s bound).
    // Another thread's reservation not yet committed is a session still
    // filling, which that thread will commit, and another
    // thread's verified buffer whose result poll() has handed out is being
    // copied into its owner's job buffer, which that thread will release
    // (no poll() of the caller's could free it): the call waits
    // for either as for any in-flight group (bounded, pvq_wait).  If the
    // bound runs out on such a polled buffer the call fails with ENOMEM and
    // names it: the drain is fine, the room is a caller's to free.
    const std::thread::id me = std::this_thread::get_id();
    std::chrono::steady_clock::time_point held_since{};
    uint64_t held_id = ~0ull;  // the head region the grace is running for
    auto stuck = [&](bool expired) -> const char* {
        if (P->regions.empty()) return nullptr;
        const PvqRegion& r = P->regions.front();
        if (!r.reserved || r.released) return nullptr;
        const char* own = "this thread's own reserved buffer, not committed or not released";
        if (!r.committed) return r.owner == me ? own : nullptr;
        if (!r.collected) return nullptr;
        if (r.owner == me) return own;
        if (r.polled)
            return expired ? "another thread's verified buffer, its result polled and not released within "
                             "SHA1CHUNK_VQ_WAIT_S (that thread's release() frees it)"
                           : nullptr;
        const auto now = std::chrono::steady_clock::now();
        if (held_id != P->reg_base) {  // a new head region: its own grace
            held_id = P->reg_base;
            held_since = now;
        }
        return now - held_since >= kHeldResultWait
                   ? "a verified buffer whose result is not yet polled and released (poll() and release() free it)"
                   : nullptr;
    };
    if (int rc = pvq_wait(P, [&] { return pos() + need - P->byte_head <= P->nbytes; }, "data ring full", stuck))
        return rc;
    const uint64_t at = pos();
    P->regions.push_back(PvqRegion{at, at + need, reserved, false, false, false, me});
    P->byte_tail = at + need;
    *id = P->reg_base + P->regions.size() - 1;
    return SHA1CHUNK_OK;
}

// Give region `id` (filled, `len` bytes) the next slot, with its expected
// digest and tag, and publish when the group is full or the device idle.
int pvq_enqueue(Pvq* P, uint64_t id, uint32_t len, const uint8_t expected[20], uint64_t tag) {
    int rc;
    // A group never wraps the slot ring: an open group that ends where the
    // ring wraps is closed first.  pvq_wait sleeps without the queue's lock,
    // so another thread may fill the ring's last slot meanwhile and leave its
    // group open there: check again after every wait, under the
    // lock, until the next slot does not continue a group across the wrap.
    for (;;) {
        if (P->open_count && P->slot_tail % P->nslots == 0 && (rc = pvq_publish(P))) return rc;
        if ((rc = pvq_wait(P, [&] { return P->slot_tail + 1 - P->slot_head <= P->nslots; }, "slot ring full")))
            return rc;
        if (!(P->open_count && P->slot_tail % P->nslots == 0)) break;
    }
    PvqRegion& r = P->regions[id - P->reg_base];
    const uint64_t sl = P->slot_tail % P->nslots;
    P->off[sl] = r.start % P->nbytes;
    P->len[sl] = len;
    memcpy(P->exp + 20 * sl, expected, 20);
    P->tags[sl] = tag;
    P->slot_reg[sl] = id;
    r.committed = true;
    if (P->open_count == 0) P->open_slot0 = P->slot_tail;
    ++P->open_count;
    ++P->slot_tail;
    ++P->pending;
    if ((rc = pvq_reap(P))) return rc;
    if (P->open_count >= P->group_max || P->inflight < static_cast<size_t>(P->cus)) return pvq_publish(P);
    return SHA1CHUNK_OK;
}

// The reserved region `buf` points at (its id), or fails.
int pvq_held(Pvq* P, const void* buf, uint64_t* id) {
    const uint8_t* b = static_cast<const uint8_t*>(buf);
    if (b < P->data || b >= P->data + P->nbytes)
        return fail(SHA1CHUNK_EINVAL, "vq: %p is not a buffer of this queue", buf);
    auto it = P->held.find(static_cast<uint64_t>(b - P->data));
    if (it == P->held.end())
        return fail(SHA1CHUNK_EINVAL, "vq: %p is not a reserved buffer (released already?)", buf);
    *id = it->second;
    return SHA1CHUNK_OK;
}
}  // namespace

namespace s1rt {
// The copy runs without the queue's lock (the region is this call's until
// it is enqueued; nothing frees an uncollected region), on the helper
// threads when no other submit is using them, else on the calling thread:
// receive threads then copy side by side instead of one after another.
int pvq_submit(Pvq* P, const void* chunk, uint32_t len, const uint8_t expected[20], uint64_t tag) {
    uint64_t id;
    if (int rc = pvq_alloc(P, len, false, &id)) return rc;
    if (len) {
        uint8_t* dst = P->data + P->regions[id - P->reg_base].start % P->nbytes;
        const int64_t c0 = mono_ns();
        if (P->mu) P->mu->unlock();
        {
            // (streaming stores into the ring measured no faster: 28.3-29.2
            // against 27.5-28.9 GiB/s, profiles/vq_copy_r05.log)
            std::unique_lock<std::mutex> cl(P->copy_mu, std::try_to_lock);
            if (cl.owns_lock())
                pool_copy(*P->copier, dst, static_cast<const uint8_t*>(chunk), len);
            else
                memcpy(dst, chunk, len);
        }
        P->copy_ns.fetch_add(static_cast<uint64_t>(mono_ns() - c0), std::memory_order_relaxed);
        if (P->mu) P->mu->lock();
    }
    return pvq_enqueue(P, id, len, expected, tag);
}

void* pvq_reserve(Pvq* P, uint32_t len) {
    uint64_t id;
    if (pvq_alloc(P, len, true, &id)) return nullptr;
    const uint64_t at = P->regions[id - P->reg_base].start % P->nbytes;
    P->held[at] = id;
    return P->data + at;
}

int pvq_commit(Pvq* P, void* buf, uint32_t len, const uint8_t expected[20], uint64_t tag) {
    uint64_t id;
    if (int rc = pvq_held(P, buf, &id)) return rc;
    const PvqRegion& r = P->regions[id - P->reg_base];
    if (r.committed) return fail(SHA1CHUNK_EINVAL, "vq: buffer %p committed twice", buf);
    if (len > r.end - r.start)
        return fail(SHA1CHUNK_EINVAL, "vq: commit of %u bytes into a %llu-byte reservation", len,
                    static_cast<unsigned long long>(r.end - r.start));
    return pvq_enqueue(P, id, len, expected, tag);
}

int pvq_release(Pvq* P, void* buf) {
    uint64_t id;
    if (int rc = pvq_held(P, buf, &id)) return rc;
    P->held.erase(static_cast<uint64_t>(static_cast<uint8_t*>(buf) - P->data));
    P->regions[id - P->reg_base].released = true;
    pvq_free_regions(P);
    return SHA1CHUNK_OK;
}

long pvq_poll(Pvq* P, uint64_t* tags, uint8_t* mismatch, size_t max, int wait) {
    int rc;
    if (wait) {
        if ((rc = pvq_publish(P))) return rc;
        // every group published so far (other threads may keep publishing
        // while this one sleeps; their later groups are not waited for)
        const uint64_t target = P->next_g;
        if ((rc = pvq_wait(P, [&] { return P->groups.empty() || P->groups.front().g >= target; }, "poll(wait)")))
            return rc;
    } else {
        if ((rc = pvq_reap(P))) return rc;
        // an open group goes out once the device has room for it
        if (P->open_count && P->inflight < static_cast<size_t>(P->cus) && (rc = pvq_publish(P))) return rc;
        if (P->inflight && (rc = pvq_ensure_drain(P))) return rc;
    }
    size_t n = 0;
    while (n < max && !P->ready.empty()) {
        const PvqResult& r = P->ready.front();
        tags[n] = r.tag;
        mismatch[n] = r.mismatch;
        // a copied chunk's region may be freed already (its id below reg_base)
        if (r.region >= P->reg_base) P->regions[r.region - P->reg_base].polled = true;
        P->ready.pop_front();
        ++n;
    }
    P->pending -= n;
    return static_cast<long>(n);
}

uint32_t pvq_max_len(const Pvq* P) { return P->maxlen; }
size_t pvq_pending(const Pvq* P) { return P->pending; }

void pvq_print_stats(const Pvq* P, FILE* f) {
    fprintf(f, "\"publish\": %llu, \"published\": %llu, \"copies\": %llu, \"launch\": %llu, "
            "\"scans\": %llu, \"sleeps\": %llu, \"sleep_ms\": %.3f, \"submit_copy_ms\": %.3f, ",
            (unsigned long long)P->n_publish, (unsigned long long)P->n_published,
            (unsigned long long)P->n_copies, (unsigned long long)P->n_launch,
            (unsigned long long)P->n_scans, (unsigned long long)P->n_sleeps, P->sleep_ns * 1e-6,
            P->copy_ns.load() * 1e-6);
}
}  // namespace s1rt
