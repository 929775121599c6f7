// rt_gather.hip -- host side of hashing and verifying messages given as
// segment lists (include/sha1chunk.h, sha1chunk_gather_device_async,
// sha1chunk_hash_gather_batch, sha1chunk_verify_gather_batch and the pinned
// allocation for packet rings; kernels in sha1_gather.hip).
//
// Device form: scan -> copy on the caller's stream, scratch (a position per
// segment, a length word per message) from the stream-ordered allocator, as
// rt_update.hip takes its scratch.
//
// Host-array forms: the batch goes in sub-batches of whole messages whose
// packed size (every message on a 128-byte line) stays under
// SHA1CHUNK_GATHER_STAGE_MIB (default 4096, at least one message each).  Where
// `base` lives decides the path of the whole call:
//   device memory, or host memory the device reads in place (host_pinned):
//       per sub-batch the segment arrays go up, the gather kernels reassemble
//       into a device stage owned by this file, s1be_hash_device_async hashes
//       the stage under KERNEL_AUTO (SHA1CHUNK_FORCE_KERNEL and
//       SHA1CHUNK_SPLIT_UNIT apply), the compare kernel follows for verify,
//       and only digests or flags come back;
//   pageable host memory (the compatibility path):
//       the device's pack pool copies each sub-batch's segments contiguously
//       into a pinned fill and the existing host-batch path (s1be_hash_batch /
//       s1be_verify_batch) takes it from there; no gather kernel runs.
// Unpipelined: a sub-batch is finished before the next is staged.
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

#include "gather_map.hpp"
#include "sha1_runtime_internal.h"

using namespace s1rt;

extern "C" {
int s1be_hash_device_async(const void*, const uint64_t*, const uint32_t*, size_t, uint8_t*, void*, int);
int s1be_compare_device_async(const uint8_t*, const uint8_t*, size_t, uint8_t*, void*);
int s1be_hash_batch(const void*, const uint64_t*, const uint32_t*, size_t, uint8_t*, unsigned);
int s1be_verify_batch(const void*, const uint64_t*, const uint32_t*, size_t, const uint8_t*, uint8_t*, unsigned);
int s1be_gather_device_async(const void*, const uint64_t*, const uint32_t*, size_t, const uint32_t*, size_t, void*,
                             const uint64_t*, uint64_t, uint32_t*, void*);
}

namespace {
constexpr size_t kCountMax = 0xffffffffu - 1024u;  // check_batch's limit (sha1_runtime.hip)

// s1be_gather_stats: sub-batches, gather launches (scan + copy pairs), then
// after the device's count of skipped messages the host-form calls by source.
enum { kSubBatches, kLaunches, kSkippedSlot, kFromDevice, kFromPinned, kFromPageable, kStats };
std::atomic<uint64_t> g_stat[kStats];

struct Stage {
    std::mutex mu;      // one host-form call at a time per device; taken before the device's
    PinBuf hmeta;       // segment arrays up, digests / flags back
    DevBuf dmeta;
    DevBuf data;        // the reassembled messages
    PinBuf fill;        // pageable path: the packed messages
    uint32_t* skipped = nullptr;  // device counter of skipped messages
    size_t cap = 0;     // packed bytes per sub-batch
};
Stage* g_stage;  // one per logical device
std::once_flag g_stage_once;

Stage& stage_of(Device& D) {
    std::call_once(g_stage_once, [] { g_stage = new Stage[std::max(1, device_count())]; });
    return g_stage[&D - g_dev];
}

// The device's counter of skipped messages, made on the first gather.
int skipped_counter(Device& D, uint32_t** out) {
    Stage& S = stage_of(D);
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!S.skipped) {
        void* p = nullptr;
        if (hipMalloc(&p, 128) != hipSuccess) return fail(SHA1CHUNK_ENOMEM, "hipMalloc(128) failed");
        if (hipMemset(p, 0, 128) != hipSuccess) {
            (void)hipFree(p);
            return fail(SHA1CHUNK_EHIP, "hipMemset failed");
        }
        S.skipped = static_cast<uint32_t*>(p);
    }
    *out = S.skipped;
    return SHA1CHUNK_OK;
}

int launched(hipError_t e, const char* what) {
    return e == hipSuccess ? SHA1CHUNK_OK : fail(SHA1CHUNK_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// Message lengths of a host segment list, with every refusal of the host forms.
int message_lengths(const uint32_t* seg_lengths, size_t n_segments, const uint32_t* seg_first, size_t n,
                    std::vector<uint32_t>& len) {
    len.resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (s1ga::skip_range(seg_first[i], seg_first[i + 1], n_segments))
            return fail(SHA1CHUNK_EINVAL, "message %zu: segments %u..%u of %zu", i, seg_first[i], seg_first[i + 1],
                        n_segments);
        uint64_t total = 0;
        for (size_t s = seg_first[i]; s < seg_first[i + 1]; ++s) total += seg_lengths[s];
        if (total > s1ga::kMaxMessage) return fail(SHA1CHUNK_EINVAL, "message %zu: longer than 2^32 - 2 bytes", i);
        len[i] = static_cast<uint32_t>(total);
    }
    return SHA1CHUNK_OK;
}

struct Call {
    const uint8_t* base;
    const uint64_t* seg_off;
    const uint32_t* seg_len;
    const uint32_t* seg_first;
    const uint32_t* len;      // message lengths
    uint8_t* digests;         // hash: n x 20
    const uint8_t* expected;  // verify: n x 20, and
    uint8_t* mismatch;        //   n flags
};

// Messages [lo, hi) from a source the device reads: arrays up, gather, hash,
// (compare,) results back.  Under the stage's and the device's mutex.
int run_device_sub(Device& D, Stage& S, const Call& c, size_t lo, size_t hi, size_t packed) {
    const size_t m = hi - lo, s0 = c.seg_first[lo], ns = c.seg_first[hi] - s0;
    const size_t dstoff_at = ns * 8, seglen_at = dstoff_at + m * 8, first_at = seglen_at + ns * 4;
    const size_t exp_at = round_up(first_at + (m + 1) * 4, kAlign);
    const size_t up = exp_at + (c.expected ? m * 20 : 0);
    const size_t outlen_at = round_up(up, kAlign), dig_at = outlen_at + round_up(m * 4, kAlign);
    const size_t mis_at = dig_at + round_up(m * 20, kAlign), bytes = mis_at + round_up(m, kAlign);
    int rc;
    if ((rc = S.hmeta.ensure(bytes)) || (rc = S.dmeta.ensure(bytes)) || (rc = S.data.ensure(std::max(packed, kAlign))))
        return rc;
    uint8_t* h = static_cast<uint8_t*>(S.hmeta.p);
    uint8_t* d = static_cast<uint8_t*>(S.dmeta.p);
    if (ns) {
        memcpy(h, c.seg_off + s0, ns * 8);
        memcpy(h + seglen_at, c.seg_len + s0, ns * 4);
    }
    uint64_t* hdst = reinterpret_cast<uint64_t*>(h + dstoff_at);
    uint32_t* hfirst = reinterpret_cast<uint32_t*>(h + first_at);
    size_t cur = 0;
    for (size_t j = 0; j < m; ++j) {
        hdst[j] = cur;
        hfirst[j] = static_cast<uint32_t>(c.seg_first[lo + j] - s0);
        cur += round_up(c.len[lo + j], kAlign);
    }
    hfirst[m] = static_cast<uint32_t>(ns);
    if (c.expected) memcpy(h + exp_at, c.expected + 20 * lo, m * 20);
    hipStream_t st = D.slot[0].stream;
    HIP_TRY(hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, st));
    const uint64_t* d_dst = reinterpret_cast<const uint64_t*>(d + dstoff_at);
    uint32_t* d_len = reinterpret_cast<uint32_t*>(d + outlen_at);
    if ((rc = s1be_gather_device_async(c.base, reinterpret_cast<const uint64_t*>(d),
                                       reinterpret_cast<const uint32_t*>(d + seglen_at), ns,
                                       reinterpret_cast<const uint32_t*>(d + first_at), m, S.data.p, d_dst, packed, d_len,
                                       st)))
        return rc;
    if ((rc = s1be_hash_device_async(S.data.p, d_dst, d_len, m, d + dig_at, st, SHA1CHUNK_KERNEL_AUTO))) return rc;
    if (c.expected) {
        if ((rc = s1be_compare_device_async(d + dig_at, d + exp_at, m, d + mis_at, st))) return rc;
        HIP_TRY(hipMemcpyAsync(h + mis_at, d + mis_at, m, hipMemcpyDeviceToHost, st));
    } else {
        HIP_TRY(hipMemcpyAsync(h + dig_at, d + dig_at, m * 20, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (c.expected)
        memcpy(c.mismatch + lo, h + mis_at, m);
    else
        memcpy(c.digests + 20 * lo, h + dig_at, m * 20);
    return SHA1CHUNK_OK;
}

// Messages [lo, hi) from pageable memory: packed into the pinned fill (every
// message on a 16-byte boundary, so equal lengths that are multiples of 16 lie
// back to back and the host-batch path copies them up in one piece), then the
// host-batch path.  Under the stage's mutex; the device's only while packing.
int run_pageable_sub(Device& D, Stage& S, const Call& c, size_t lo, size_t hi) {
    const size_t m = hi - lo;
    std::vector<uint64_t> off(m + 1);
    size_t cur = 0;
    for (size_t j = 0; j < m; ++j) {
        off[j] = cur;
        cur += round_up(c.len[lo + j], 16);
    }
    off[m] = cur;
    int rc;
    if ((rc = S.fill.ensure(std::max(cur, kAlign)))) return rc;
    uint8_t* h = static_cast<uint8_t*>(S.fill.p);
    {
        std::lock_guard<std::mutex> lk(D.mu);
        if (!D.pack) D.pack.reset(new PartPool(pack_threads() - 1, near_cpus(D.id)));
        const size_t T = std::min<size_t>({D.pack->width(), m, std::max<size_t>(1, cur >> 23)});
        std::vector<size_t> cut(T + 1, m);
        cut[0] = 0;
        for (size_t t = 1, j = 0; t < T; ++t) {
            while (j < m && off[j] < cur * t / T) ++j;
            cut[t] = j;
        }
        D.pack->run(T, [&](size_t t) {
            for (size_t j = cut[t]; j < cut[t + 1]; ++j) {
                uint8_t* to = h + off[j];
                for (size_t s = c.seg_first[lo + j]; s < c.seg_first[lo + j + 1]; ++s) {
                    if (c.seg_len[s]) memcpy(to, c.base + c.seg_off[s], c.seg_len[s]);
                    to += c.seg_len[s];
                }
            }
        });
    }
    if (c.expected)
        return s1be_verify_batch(h, off.data(), c.len + lo, m, c.expected + 20 * lo, c.mismatch + lo, SHA1CHUNK_HOST);
    return s1be_hash_batch(h, off.data(), c.len + lo, m, c.digests + 20 * lo, SHA1CHUNK_HOST);
}

int gather_batch(const void* base, const uint64_t* seg_offsets, const uint32_t* seg_lengths, size_t n_segments,
                 const uint32_t* seg_first, size_t n, uint8_t* digests, const uint8_t* expected, uint8_t* mismatch,
                 unsigned flags) {
    if (n == 0) return SHA1CHUNK_OK;
    if (flags & SHA1CHUNK_ALL_DEVICES) return fail(SHA1CHUNK_EINVAL, "SHA1CHUNK_ALL_DEVICES: one device per call");
    if (flags & ~SHA1CHUNK_DEVICE) return fail(SHA1CHUNK_EINVAL, "unknown flags %#x", flags);
    if (n > kCountMax || n_segments > kCountMax)
        return fail(SHA1CHUNK_EINVAL, "n too large: at most 2^32 - 1025 messages and segments per call");
    if (!base || !seg_first || (n_segments && (!seg_offsets || !seg_lengths)) || (expected ? !mismatch : !digests))
        return fail(SHA1CHUNK_EINVAL, "null pointer");
    std::vector<uint32_t> len;
    int rc = message_lengths(seg_lengths, n_segments, seg_first, n, len);
    if (rc) return rc;
    Device* D;
    if ((rc = get_device(&D))) return rc;
    Stage& S = stage_of(*D);
    std::lock_guard<std::mutex> call(S.mu);
    // read per call, so that a test can force several sub-batches
    S.cap = static_cast<size_t>(std::min<uint64_t>(65536, std::max<uint64_t>(1, env_u64("SHA1CHUNK_GATHER_STAGE_MIB", 4096))))
            << 20;
    const bool device = flags & SHA1CHUNK_DEVICE, in_place = device || host_pinned(base);
    const Call c{static_cast<const uint8_t*>(base), seg_offsets, seg_lengths, seg_first, len.data(), digests, expected,
                 mismatch};
    ++g_stat[device ? kFromDevice : in_place ? kFromPinned : kFromPageable];
    for (size_t lo = 0; lo < n;) {
        size_t hi = lo, packed = 0;
        while (hi < n) {
            const size_t b = round_up(len[hi], kAlign);
            if (hi > lo && packed + b > S.cap) break;
            packed += b;
            ++hi;
        }
        ++g_stat[kSubBatches];
        if (in_place) {
            std::lock_guard<std::mutex> lk(D->mu);
            if ((rc = discard_in_flight(*D)) || (rc = run_device_sub(*D, S, c, lo, hi, packed))) return rc;
        } else if ((rc = run_pageable_sub(*D, S, c, lo, hi))) {
            return rc;
        }
        lo = hi;
    }
    return SHA1CHUNK_OK;
}
}  // namespace

// ================================================================ C ABI ====
extern "C" {

void* s1be_pinned_alloc(size_t bytes) {
    if (bytes == 0) {
        fail(SHA1CHUNK_EINVAL, "pinned allocation of 0 bytes");
        return nullptr;
    }
    Device* D;
    if (get_device(&D)) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        fail(SHA1CHUNK_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

int s1be_pinned_free(void* p) {
    if (!p) return SHA1CHUNK_OK;
    Device* D;
    if (int rc = get_device(&D)) return rc;
    if (!host_pinned(p)) return fail(SHA1CHUNK_EINVAL, "not a pointer from sha1chunk_pinned_alloc");
    HIP_TRY(hipHostFree(p));
    return SHA1CHUNK_OK;
}

int s1be_gather_device_async(const void* d_base, const uint64_t* d_seg_offsets, const uint32_t* d_seg_lengths,
                             size_t n_segments, const uint32_t* d_seg_first, size_t n, void* d_dst,
                             const uint64_t* d_dst_offsets, uint64_t dst_bytes, uint32_t* d_out_lengths, void* stream) {
    if (n == 0) return SHA1CHUNK_OK;
    if (n > kCountMax || n_segments > kCountMax)
        return fail(SHA1CHUNK_EINVAL, "n too large: at most 2^32 - 1025 messages and segments per call");
    if (!d_base || !d_seg_first || !d_dst || !d_dst_offsets || (n_segments && (!d_seg_offsets || !d_seg_lengths)))
        return fail(SHA1CHUNK_EINVAL, "null device pointer");
    Device* D;
    if (int rc = get_device(&D)) return rc;
    GatherArgs G{};
    if (int rc = skipped_counter(*D, &G.skipped)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t scratch_bytes = (n_segments + n) * 4;
    uint8_t* scratch = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&scratch), scratch_bytes, st) != hipSuccess)
        return fail(SHA1CHUNK_ENOMEM, "hipMallocAsync(%zu) failed", scratch_bytes);
    // pinned host memory: the address the device knows it by
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, d_base) == hipSuccess) {
        if (at.type == hipMemoryTypeHost && at.devicePointer) d_base = at.devicePointer;
    } else {
        (void)hipGetLastError();
    }
    G.base = static_cast<const uint8_t*>(d_base);
    G.seg_off = d_seg_offsets;
    G.seg_len = d_seg_lengths;
    G.n_segments = n_segments;
    G.seg_first = d_seg_first;
    G.n = static_cast<uint32_t>(n);
    G.dst = static_cast<uint8_t*>(d_dst);
    G.dst_off = d_dst_offsets;
    G.dst_bytes = dst_bytes;
    G.out_len = d_out_lengths;
    G.pos = reinterpret_cast<uint32_t*>(scratch);
    G.mlen = G.pos + n_segments;
    int rc = launched(launch_gather_scan(G, st), "gather scan launch");
    if (!rc) rc = launched(launch_gather_copy(G, st), "gather copy launch");
    (void)hipFreeAsync(scratch, st);
    if (!rc) ++g_stat[kLaunches];
    return rc;
}

int s1be_hash_gather_batch(const void* base, const uint64_t* seg_offsets, const uint32_t* seg_lengths,
                           size_t n_segments, const uint32_t* seg_first, size_t n, uint8_t* digests, unsigned flags) {
    return gather_batch(base, seg_offsets, seg_lengths, n_segments, seg_first, n, digests, nullptr, nullptr, flags);
}

int s1be_verify_gather_batch(const void* base, const uint64_t* seg_offsets, const uint32_t* seg_lengths,
                             size_t n_segments, const uint32_t* seg_first, size_t n, const uint8_t* expected,
                             uint8_t* mismatch, unsigned flags) {
    if (n && !expected) return fail(SHA1CHUNK_EINVAL, "null pointer");
    return gather_batch(base, seg_offsets, seg_lengths, n_segments, seg_first, n, nullptr, expected, mismatch, flags);
}

// Diagnostics (tests; no front-end entry point), added up over the process:
// out[0] sub-batches of the host-array forms, out[1] gather launches (a scan
// and a copy kernel each), out[2] messages the scan kernels skipped (read
// from the devices: waits for them), out[3..5] host-array calls whose source
// was device memory / host memory read in place / pageable memory.
void s1be_gather_stats(uint64_t out[6], int reset) {
    for (int k = 0; k < kStats; ++k) out[k] = reset ? g_stat[k].exchange(0) : g_stat[k].load();
    out[kSkippedSlot] = 0;
    if (!g_stage) return;
    for (int dev = 0; dev < device_count(); ++dev) {
        uint32_t* p = g_stage[dev].skipped;
        uint32_t v = 0;
        if (!p || hipSetDevice(g_dev[dev].id) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(&v, p, 4, hipMemcpyDeviceToHost) != hipSuccess)
            continue;
        out[kSkippedSlot] += v;
        if (reset) (void)hipMemset(p, 0, 4);
    }
}

}  // extern "C"
