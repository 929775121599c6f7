// sha1_pv.hip -- host side of the progressive verifier (sha1chunk_pv,
// include/sha1chunk.h; kernels: sha1_progress.hip, one lane per session, and
// sha1_progress_shared.hip, loads shared across the wave).  Exports s1be_pv_*,
// s1be_burst_advance and s1be_progress_stats to the front end, nothing else.
//
// The object owns `sessions` receive buffers in pinned host memory, one
// private stream and two launch slots.  advance() only records a session's
// new mark; pump() -- run by advance, hashed and poll under the object's
// lock -- does the rest, without ever waiting for the device:
//   reap     a launch slot whose event has completed confirms the bytes its
//            entries covered and drops its references to their sessions;
//   harvest  a session whose final entry is enqueued is finished once its
//            completion word in host memory holds the session's generation
//            (the kernel's system-scope store, seen before the launch's
//            event is);
//   launch   with a launch slot free and work pending (a session with a new
//            whole block, or a completed one), one kernel takes all of it:
//            the work list goes into the slot's part of a pinned ring, one
//            entry per session.  Which kernel: SHA1CHUNK_PV_KERNEL (pv_pick).
// While both slots are outstanding work accumulates, so the launch rate is
// bounded by the kernel's time, with no threshold to tune.  The host owns
// the byte accounting (from / upto of every entry); the device only the
// midstates, which launches on the one stream hand from one to the next.
//
// A session closed while launches still refer to it keeps its buffer until
// they have completed (refs); a generation number per open() tells a
// session's completion word from its slot's previous occupant's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sha1chunk.h"
#include "sha1_kernels.h"
#include "sha1_runtime_internal.h"

namespace {
using s1rt::fail;
using s1rt::kAlign;  // every session buffer starts on a 128-byte line
using s1rt::round_up;

constexpr int kLaunchSlots = 2;
enum { kKernelAuto = 0, kKernelLane = 1, kKernelShared = 2 };
// `auto` takes the shared-load kernel for a work list with at least this
// many entries that carry a whole block; 0: never.  64, a whole wave: the
// smallest session count measured (4, 16, 64, 256; DESIGN.md section 6,
// profiles/pv_shared.jsonl) at which the shared kernel's median passed the
// lane kernel's by more than the lane kernel's own spread -- 1531 against
// 217 MB/s (194-280) fed per call; at 16 both hash at the lanes' compute
// rate, 820 against 807 (736-861).  It counts one launch's entries: fewer
// than 64 sessions with a new block stay on the lane kernel.
constexpr uint32_t kSharedThreshold = 64;

struct PvSession {
    bool open = false;       // handed out by open(), not yet freed
    bool closing = false;    // close()d; freed once nothing refers to it
    bool complete = false;   // advance() reached len
    bool final_issued = false;
    bool harvested = false;  // the verdict is in the result queue (or was dropped)
    bool dirty = false;      // in Pv::dirty
    uint32_t len = 0;
    uint32_t mark = 0;       // bytes the caller declared final
    uint32_t issued = 0;     // bytes covered by enqueued entries (multiple of 64, or len)
    uint32_t confirmed = 0;  // bytes of completed launches (or len once harvested)
    uint32_t gen = 0;
    int refs = 0;            // enqueued launches with an entry of this session
    uint64_t tag = 0;
};

struct PvItem {
    uint32_t session, gen, upto;
};

struct PvLaunch {
    hipEvent_t ev = nullptr;
    bool busy = false;
    std::vector<PvItem> items;
};

struct PvResult {
    uint64_t tag;
    uint8_t mismatch;
    uint8_t digest[20];
};

struct Pv {
    std::mutex mu;
    int dev = -1;
    int depth = 4;
    uint32_t sessions = 0, maxlen = 0;
    size_t stride = 0;
    // pinned: the session buffers; then expected | result | done | work ring
    uint8_t* data = nullptr;
    size_t data_bytes = 0;
    uint8_t* meta = nullptr;
    size_t meta_bytes = 0;
    uint32_t* expected = nullptr;  // 8 words per session
    uint32_t* result = nullptr;    // 8 words per session
    uint32_t* done = nullptr;      // 1 word per session
    PvEntry* work = nullptr;       // kLaunchSlots x sessions entries
    uint32_t* state = nullptr;     // device: 5 words per session, then the 64-byte dummy line
    const uint8_t* dummy = nullptr;
    int kernel = kKernelAuto;      // SHA1CHUNK_PV_KERNEL
    hipStream_t stream = nullptr;
    PvLaunch launch[kLaunchSlots];
    std::vector<PvSession> ses;
    std::vector<uint32_t> free_list;  // session indices open() may hand out
    std::vector<uint32_t> dirty;      // sessions with work for the next launch
    std::vector<uint32_t> awaiting;   // sessions whose final entry is enqueued
    std::deque<PvResult> results;
    size_t pending = 0;  // completed sessions whose result poll() has not returned
    uint32_t next_gen = 1;
    int error = 0;  // a HIP failure in pump(): every later call reports it
    std::string error_text;
    bool stats = false;
    uint64_t n_launch = 0, n_launch_shared = 0, n_entries = 0, n_blocks = 0;
};

void pv_free_session(Pv* p, uint32_t s) {
    p->ses[s] = PvSession();
    p->free_list.push_back(s);
}

// A closing session goes once no enqueued launch refers to it and, if it
// completed, its verdict has been taken.
void pv_maybe_free(Pv* p, uint32_t s) {
    PvSession& S = p->ses[s];
    if (S.open && S.closing && S.refs == 0 && (!S.complete || S.harvested)) pv_free_session(p, s);
}

int pv_hip_error(Pv* p, hipError_t e, const char* what) {
    p->error = SHA1CHUNK_EHIP;
    char buf[256];
    snprintf(buf, sizeof buf, "pv: %s failed: %s", what, hipGetErrorString(e));
    p->error_text = buf;
    return fail(SHA1CHUNK_EHIP, "%s", buf);
}

void pv_mark_dirty(Pv* p, uint32_t s) {
    PvSession& S = p->ses[s];
    if (S.dirty) return;
    S.dirty = true;
    p->dirty.push_back(s);
}

// The kernel of a launch of n entries, `with_block` of them with a whole block.
bool pv_pick_shared(const Pv* p, uint32_t n, uint32_t with_block) {
    if (p->kernel != kKernelAuto) return p->kernel == kKernelShared;
    // a lone session's launches stay what they were
    return n > 1 && kSharedThreshold != 0 && with_block >= kSharedThreshold;
}

// Caller holds p->mu and has made p->dev current.  Never blocks.
int pv_pump(Pv* p) {
    if (p->error) return fail(p->error, "%s", p->error_text.c_str());
    // reap
    for (PvLaunch& L : p->launch) {
        if (!L.busy) continue;
        const hipError_t e = hipEventQuery(L.ev);
        if (e == hipErrorNotReady) continue;
        if (e != hipSuccess) return pv_hip_error(p, e, "hipEventQuery");
        for (const PvItem& it : L.items) {
            PvSession& S = p->ses[it.session];
            if (!S.open || S.gen != it.gen) continue;
            --S.refs;
            S.confirmed = std::max(S.confirmed, S.harvested ? S.len : it.upto & ~63u);
            pv_maybe_free(p, it.session);
        }
        L.items.clear();
        L.busy = false;
    }
    // harvest
    for (size_t i = 0; i < p->awaiting.size();) {
        const uint32_t s = p->awaiting[i];
        PvSession& S = p->ses[s];
        if (__atomic_load_n(&p->done[s], __ATOMIC_ACQUIRE) != S.gen) {
            ++i;
            continue;
        }
        PvResult R;
        R.tag = S.tag;
        R.mismatch = p->result[8 * s + 5] ? 1 : 0;
        memcpy(R.digest, p->result + 8 * s, 20);
        p->results.push_back(R);
        S.harvested = true;
        S.confirmed = S.len;
        p->awaiting[i] = p->awaiting.back();
        p->awaiting.pop_back();
        pv_maybe_free(p, s);
    }
    // launch
    if (p->dirty.empty()) return SHA1CHUNK_OK;
    int k = -1;
    for (int i = 0; i < kLaunchSlots; ++i)
        if (!p->launch[i].busy) {
            k = i;
            break;
        }
    if (k < 0) return SHA1CHUNK_OK;
    PvLaunch& L = p->launch[k];
    PvEntry* W = p->work + size_t(k) * p->sessions;
    uint32_t n = 0, with_block = 0;
    for (const uint32_t s : p->dirty) {
        PvSession& S = p->ses[s];
        S.dirty = false;
        if (!S.open || (S.closing && !S.complete) || S.final_issued) continue;
        const uint32_t upto = S.complete ? S.len : S.mark & ~63u;
        if (!S.complete && upto <= S.issued) continue;
        PvEntry E{};
        E.session = s;
        E.from = S.issued;
        E.upto = upto;
        E.len = S.len;
        E.final = S.complete ? 1u : 0u;
        E.gen = S.gen;
        W[n++] = E;
        L.items.push_back({s, S.gen, upto});
        p->n_blocks += (upto - S.issued) / 64u;
        with_block += upto - S.issued >= 64u ? 1u : 0u;
        S.issued = S.complete ? S.len : upto;
        ++S.refs;
        if (S.complete) {
            S.final_issued = true;
            p->awaiting.push_back(s);
        }
    }
    p->dirty.clear();
    if (n == 0) return SHA1CHUNK_OK;
    // the work list is in host memory the device reads: written before the launch
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    PvArgs A{};
    A.data = p->data;
    A.stride = p->stride;
    A.work = W;
    A.n = n;
    A.sessions = p->sessions;
    A.state = p->state;
    A.expected = p->expected;
    A.result = p->result;
    A.done = p->done;
    A.dummy = p->dummy;
    const bool shared = pv_pick_shared(p, n, with_block);
    hipError_t e = shared ? launch_progress_shared(A, p->stream) : launch_progress(A, p->depth, p->stream);
    if (e != hipSuccess)
        return pv_hip_error(p, e, shared ? "sha1_progress_shared_kernel launch" : "sha1_progress_kernel launch");
    if ((e = hipEventRecord(L.ev, p->stream)) != hipSuccess) return pv_hip_error(p, e, "hipEventRecord");
    L.busy = true;
    ++p->n_launch;
    p->n_launch_shared += shared ? 1u : 0u;
    p->n_entries += n;
    return SHA1CHUNK_OK;
}

// The open session whose buffer starts at buf, or -1.
long pv_find(const Pv* p, const void* buf) {
    const uint8_t* b = static_cast<const uint8_t*>(buf);
    if (!b || b < p->data || b >= p->data + p->data_bytes) return -1;
    const size_t off = static_cast<size_t>(b - p->data);
    if (off % p->stride) return -1;
    const size_t s = off / p->stride;
    if (s >= p->sessions || !p->ses[s].open || p->ses[s].closing) return -1;
    return static_cast<long>(s);
}

// Pinned host memory of the persistent queue's PCIe-read ring's kind, coherent
// when that kind cannot be had.  (Not from the queues' cache of rings: that
// holds a few large rings by exact size, which these would push out.)
uint8_t* pinned_alloc(size_t bytes) {
    void* p = nullptr;
    const unsigned flags = s1rt::ring_flags();
    if (hipHostMalloc(&p, bytes, flags) == hipSuccess) return static_cast<uint8_t*>(p);
    (void)hipGetLastError();
    if (flags != hipHostMallocCoherent && hipHostMalloc(&p, bytes, hipHostMallocCoherent) == hipSuccess)
        return static_cast<uint8_t*>(p);
    (void)hipGetLastError();
    return nullptr;
}

void pv_release(Pv* p) {
    if (p->dev >= 0) (void)hipSetDevice(p->dev);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (PvLaunch& L : p->launch)
        if (L.ev) (void)hipEventDestroy(L.ev);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    if (p->state) (void)hipFree(p->state);
    if (p->meta) (void)hipHostFree(p->meta);
    if (p->data) (void)hipHostFree(p->data);
    delete p;
}

}  // namespace

extern "C" {

void* s1be_pv_create(size_t sessions, uint32_t max_chunk_len) {
    if (sessions == 0 || sessions > (1u << 20)) {
        fail(SHA1CHUNK_EINVAL, "pv: 1..2^20 sessions required");
        return nullptr;
    }
    s1rt::Device* D;
    if (s1rt::get_device(&D)) return nullptr;
    Pv* p = new Pv();
    p->dev = D->id;
    p->sessions = static_cast<uint32_t>(sessions);
    p->maxlen = max_chunk_len;
    p->stride = round_up(std::max<size_t>(max_chunk_len, 1), kAlign);
    // blocks in flight per lane (sha1_progress.hip): 2, 4 and 8 measured alike
    // (profiles/pv_latency.jsonl), 4 costs no registers
    // over 2; SHA1CHUNK_PV_DEPTH for A/B
    if (const char* e = getenv("SHA1CHUNK_PV_DEPTH")) {
        p->depth = atoi(e);
        if (p->depth != 2 && p->depth != 4 && p->depth != 8) {
            fail(SHA1CHUNK_EINVAL, "pv: SHA1CHUNK_PV_DEPTH must be 2, 4 or 8");
            delete p;
            return nullptr;
        }
    }
    // which kernel a launch takes: auto (pv_pick_shared), or one of them for
    // every launch, single-entry work lists included
    if (const char* e = getenv("SHA1CHUNK_PV_KERNEL")) {
        if (!strcmp(e, "auto")) {
            p->kernel = kKernelAuto;
        } else if (!strcmp(e, "lane")) {
            p->kernel = kKernelLane;
        } else if (!strcmp(e, "shared")) {
            p->kernel = kKernelShared;
        } else {
            fail(SHA1CHUNK_EINVAL, "pv: SHA1CHUNK_PV_KERNEL must be auto, lane or shared, not \"%.32s\"", e);
            delete p;
            return nullptr;
        }
    }
    if (const char* e = getenv("SHA1CHUNK_PV_STATS")) p->stats = atoi(e) != 0;
    p->data_bytes = p->stride * sessions;
    const size_t o_exp = 0, o_res = o_exp + 32 * sessions, o_done = o_res + 32 * sessions,
                 o_work = round_up(o_done + 4 * sessions, kAlign);
    p->meta_bytes = o_work + sizeof(PvEntry) * kLaunchSlots * sessions;
    if (!(p->data = pinned_alloc(p->data_bytes)) || !(p->meta = pinned_alloc(p->meta_bytes))) {
        fail(SHA1CHUNK_ENOMEM, "pv: pinned buffers of %zu + %zu bytes", p->data_bytes, p->meta_bytes);
        pv_release(p);
        return nullptr;
    }
    memset(p->meta, 0, p->meta_bytes);
    p->expected = reinterpret_cast<uint32_t*>(p->meta + o_exp);
    p->result = reinterpret_cast<uint32_t*>(p->meta + o_res);
    p->done = reinterpret_cast<uint32_t*>(p->meta + o_done);
    p->work = reinterpret_cast<PvEntry*>(p->meta + o_work);
    // the midstates, then the dummy line on a 128-byte boundary (zeroed: what
    // it holds is loaded and discarded)
    const size_t o_dummy = round_up(20 * sessions, kAlign);
    bool ok = hipMalloc(reinterpret_cast<void**>(&p->state), o_dummy + 64) == hipSuccess &&
              hipMemset(reinterpret_cast<uint8_t*>(p->state) + o_dummy, 0, 64) == hipSuccess &&
              s1rt::vq_stream_create(&p->stream) == 0;
    if (ok) p->dummy = reinterpret_cast<const uint8_t*>(p->state) + o_dummy;
    for (PvLaunch& L : p->launch)
        ok = ok && hipEventCreateWithFlags(&L.ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        fail(SHA1CHUNK_ENOMEM, "pv: device state, stream or events");
        pv_release(p);
        return nullptr;
    }
    p->ses.resize(sessions);
    p->free_list.reserve(sessions);
    for (size_t s = sessions; s-- > 0;) p->free_list.push_back(static_cast<uint32_t>(s));
    return p;
}

void* s1be_pv_open(void* pv, uint32_t len, const uint8_t expected[20], uint64_t tag) {
    Pv* p = static_cast<Pv*>(pv);
    if (!p || !expected) {
        fail(SHA1CHUNK_EINVAL, "pv: null argument");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(p->mu);
    if (len > p->maxlen) {
        fail(SHA1CHUNK_EINVAL, "pv: chunk of %u bytes > max %u", len, p->maxlen);
        return nullptr;
    }
    if (p->free_list.empty()) {
        // sessions closed with launches in flight come free as those complete
        (void)hipSetDevice(p->dev);
        (void)pv_pump(p);
    }
    if (p->free_list.empty()) {
        fail(SHA1CHUNK_ENOMEM, "pv: all %u sessions are in use", p->sessions);
        return nullptr;
    }
    const uint32_t s = p->free_list.back();
    p->free_list.pop_back();
    PvSession& S = p->ses[s];
    S = PvSession();
    S.open = true;
    S.len = len;
    S.tag = tag;
    S.gen = p->next_gen++;
    if (p->next_gen == 0) p->next_gen = 1;  // 0 is the cleared completion word
    memcpy(p->expected + 8 * s, expected, 20);
    return p->data + p->stride * s;
}

// advance() without its pump: records the mark.  Caller holds p->mu.
static int pv_apply(Pv* p, void* buf, uint32_t ready) {
    const long s = pv_find(p, buf);
    if (s < 0) return fail(SHA1CHUNK_EINVAL, "pv: %p is not an open session's buffer", buf);
    PvSession& S = p->ses[s];
    if (S.complete) return fail(SHA1CHUNK_EINVAL, "pv: advance after the session completed");
    if (ready < S.mark) return fail(SHA1CHUNK_EINVAL, "pv: mark moved back from %u to %u", S.mark, ready);
    if (ready > S.len) return fail(SHA1CHUNK_EINVAL, "pv: mark %u beyond the chunk's %u bytes", ready, S.len);
    S.mark = ready;
    if (ready == S.len) {
        S.complete = true;
        ++p->pending;
    }
    if (S.complete || (ready & ~63u) > S.issued) pv_mark_dirty(p, static_cast<uint32_t>(s));
    return SHA1CHUNK_OK;
}

int s1be_pv_advance(void* pv, void* buf, uint32_t ready) {
    Pv* p = static_cast<Pv*>(pv);
    if (!p) return fail(SHA1CHUNK_EINVAL, "pv: null object");
    std::lock_guard<std::mutex> lk(p->mu);
    if (int rc = pv_apply(p, buf, ready)) return rc;
    HIP_TRY(hipSetDevice(p->dev));
    return pv_pump(p);
}

// n advances under one lock, one pump -- one launch decision -- at the end.
// The pairs before a refused one still go to the device; its error (and
// text) is what the call returns.
int s1be_burst_advance(void* pv, void* const* bufs, const uint32_t* ready, size_t n, size_t* applied) {
    Pv* p = static_cast<Pv*>(pv);
    if (applied) *applied = 0;
    if (!p || (n && (!bufs || !ready))) return fail(SHA1CHUNK_EINVAL, "pv: null argument");
    std::lock_guard<std::mutex> lk(p->mu);
    int rc = SHA1CHUNK_OK;
    size_t i = 0;
    for (; i < n; ++i)
        if ((rc = pv_apply(p, bufs[i], ready[i]))) break;
    if (applied) *applied = i;
    if (rc) {
        const std::string text = s1be_last_error();  // a failing pump would overwrite it
        if (hipSetDevice(p->dev) == hipSuccess) (void)pv_pump(p);
        return fail(rc, "%s", text.c_str());
    }
    HIP_TRY(hipSetDevice(p->dev));
    return pv_pump(p);
}

int s1be_progress_stats(void* pv, void* out, size_t size) {
    Pv* p = static_cast<Pv*>(pv);
    if (!p || !out) return fail(SHA1CHUNK_EINVAL, "pv: null argument");
    sha1chunk_progress_stats_t st;
    memset(&st, 0, sizeof st);
    {
        std::lock_guard<std::mutex> lk(p->mu);
        st.launches = p->n_launch;
        st.launches_shared = p->n_launch_shared;
        st.entries = p->n_entries;
        st.blocks = p->n_blocks;
        st.kernel = static_cast<uint32_t>(p->kernel);
        st.depth = static_cast<uint32_t>(p->depth);
    }
    memcpy(out, &st, std::min(size, sizeof st));
    return SHA1CHUNK_OK;
}

int s1be_pv_hashed(void* pv, const void* buf, uint32_t* bytes) {
    Pv* p = static_cast<Pv*>(pv);
    if (!p || !bytes) return fail(SHA1CHUNK_EINVAL, "pv: null argument");
    std::lock_guard<std::mutex> lk(p->mu);
    const long s = pv_find(p, buf);
    if (s < 0) return fail(SHA1CHUNK_EINVAL, "pv: %p is not an open session's buffer", buf);
    HIP_TRY(hipSetDevice(p->dev));
    if (int rc = pv_pump(p)) return rc;
    *bytes = p->ses[s].confirmed;
    return SHA1CHUNK_OK;
}

long s1be_pv_poll(void* pv, uint64_t* tags, uint8_t* mismatch, uint8_t* digests, size_t max, int wait) {
    Pv* p = static_cast<Pv*>(pv);
    if (!p || (max && (!tags || !mismatch))) return fail(SHA1CHUNK_EINVAL, "pv: null argument");
    std::unique_lock<std::mutex> lk(p->mu);
    HIP_TRY(hipSetDevice(p->dev));
    if (int rc = pv_pump(p)) return rc;
    if (wait) {
        // every session completed before the call (later ones are not waited for)
        std::vector<std::pair<uint32_t, uint32_t>> want;
        for (uint32_t s = 0; s < p->sessions; ++s)
            if (p->ses[s].open && p->ses[s].complete && !p->ses[s].harvested) want.emplace_back(s, p->ses[s].gen);
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            bool all = true;
            for (const auto& w : want) {
                const PvSession& S = p->ses[w.first];
                if (S.open && S.gen == w.second && !S.harvested) all = false;
            }
            if (all) break;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                return fail(SHA1CHUNK_EHIP, "pv: no result within 120 s");
            lk.unlock();
            std::this_thread::sleep_for(std::chrono::microseconds(20));
            lk.lock();
            if (int rc = pv_pump(p)) return rc;
        }
    }
    size_t n = 0;
    while (n < max && !p->results.empty()) {
        const PvResult& R = p->results.front();
        tags[n] = R.tag;
        mismatch[n] = R.mismatch;
        if (digests) memcpy(digests + 20 * n, R.digest, 20);
        p->results.pop_front();
        --p->pending;
        ++n;
    }
    return static_cast<long>(n);
}

int s1be_pv_close(void* pv, void* buf) {
    Pv* p = static_cast<Pv*>(pv);
    if (!p) return fail(SHA1CHUNK_EINVAL, "pv: null object");
    std::lock_guard<std::mutex> lk(p->mu);
    const long s = pv_find(p, buf);
    if (s < 0) return fail(SHA1CHUNK_EINVAL, "pv: %p is not an open session's buffer", buf);
    PvSession& S = p->ses[s];
    S.closing = true;
    // a completed session's verdict is still delivered; an incomplete chunk is dropped
    pv_maybe_free(p, static_cast<uint32_t>(s));
    return SHA1CHUNK_OK;
}

size_t s1be_pv_pending(const void* pv) {
    Pv* p = static_cast<Pv*>(const_cast<void*>(pv));
    if (!p) return 0;
    std::lock_guard<std::mutex> lk(p->mu);
    return p->pending;
}

void s1be_pv_destroy(void* pv) {
    Pv* p = static_cast<Pv*>(pv);
    if (!p) return;
    if (p->stats)
        fprintf(stderr,
                "{\"pv_stats\": {\"depth\": %d, \"launches\": %llu, \"launches_shared\": %llu, \"entries\": %llu, "
                "\"blocks\": %llu}}\n",
                p->depth, (unsigned long long)p->n_launch, (unsigned long long)p->n_launch_shared,
                (unsigned long long)p->n_entries, (unsigned long long)p->n_blocks);
    pv_release(p);
}

}  // extern "C"
