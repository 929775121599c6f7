// rt_update.hip -- host side of the batched SHA1Init / SHA1Update / SHA1Final
// over arrays of SHA1Context (include/sha1chunk.h, sha1chunk_*_device_async,
// sha1chunk_update_batch, sha1chunk_final_batch; kernels in sha1_update.hip).
//
// Device forms: enqueue on the caller's stream and return; scratch comes from
// the stream-ordered allocator, as the ragged path's sort scratch does.  An
// update is pre -> (length sort when n > 64) -> bulk -> post; the bulk is one
// launch of the existing lane / fused / split kernels in update mode
// (BatchArgs::init_state = out_state = the packed chaining values), chosen by
// choose_kernel(AUTO, n, cus) so SHA1CHUNK_FORCE_KERNEL and
// SHA1CHUNK_SPLIT_UNIT apply.  Never the mixed kernel: its persistent variant
// counts an idle wave's barriers from the padded block count (group_units,
// total_blocks), while split_body in update mode runs len >> 6 blocks, so the
// waves of a job would pass different numbers of barriers.
//
// Host forms: under the device's mutex the listed contexts and the pieces are
// staged through one pinned buffer and one device arena owned by this file
// (created on first use; SHA1CHUNK_UPDATE_FILL_MIB, default 256, bytes of
// pieces per fill), the device form runs, and the contexts come back.  A
// batch larger than a fill goes in several fills, every context in one of
// them; a piece larger than a fill is cut at multiples of 64 bytes and fed as
// successive updates of its context.  Unpipelined: a fill's copy does not
// overlap the previous fill's hashing.
#include <cstring>
#include <mutex>
#include <vector>

#include "sha1_runtime_internal.h"
#include "update_split.hpp"

using namespace s1rt;

namespace {
constexpr size_t kCtx = s1up::kContextBytes;
constexpr size_t kMaxFillEntries = size_t(1) << 20;

// check_batch's limit on n (sha1_runtime.hip): grids are computed in 32 bits
int check_count(size_t n) {
    if (n > 0xffffffffu - 1024u) return fail(SHA1CHUNK_EINVAL, "batch of %zu entries: at most 2^32 - 1025 per call", n);
    return SHA1CHUNK_OK;
}

UpdateArgs context_args(void* d_contexts, size_t n_contexts, const uint32_t* d_index, size_t n) {
    UpdateArgs U{};
    U.ctx = static_cast<uint8_t*>(d_contexts);
    U.n_contexts = n_contexts;
    U.index = d_index;
    U.n = static_cast<uint32_t>(n);
    return U;
}

int launched(hipError_t e, const char* what) {
    return e == hipSuccess ? SHA1CHUNK_OK : fail(SHA1CHUNK_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// pre -> sort -> bulk -> post on st (U: contexts, index, pieces, n > 0).
int enqueue_update(Device& D, UpdateArgs U, hipStream_t st) {
    const size_t n = U.n;
    uint8_t* scratch = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&scratch), n * (8 + 4 + 20), st) != hipSuccess)
        return fail(SHA1CHUNK_ENOMEM, "hipMallocAsync(%zu) failed", n * (8 + 4 + 20));
    U.mid_off = reinterpret_cast<uint64_t*>(scratch);
    U.state = reinterpret_cast<uint32_t*>(scratch + 8 * n);
    U.mid_len = reinterpret_cast<uint32_t*>(scratch + 28 * n);
    void* sort_scratch = nullptr;
    int rc = launched(launch_update_pre(U, st), "update pre launch");
    if (!rc) {
        BatchArgs A{};
        A.base = U.base;
        A.off = U.mid_off;
        A.len = U.mid_len;
        A.n = U.n;
        A.init_state = U.state;
        A.out_state = U.state;
        if (n > 64) {  // longest first, as the ragged path hashes
            const uint32_t* sorted_len = nullptr;
            uint32_t* plan = nullptr;
            rc = launched(sort_by_length_desc(U.mid_len, U.n, &A.order, &sorted_len, &plan, &sort_scratch, nullptr, st),
                          "length sort");
        }
        if (!rc) rc = launch_checked(choose_kernel(SHA1CHUNK_KERNEL_AUTO, n, D.cus), A, st, D.cus);
        if (!rc) rc = launched(launch_update_post(U, st), "update post launch");
    }
    if (sort_scratch) (void)hipFreeAsync(sort_scratch, st);
    (void)hipFreeAsync(scratch, st);
    return rc;
}

// ------------------------------------------------------------ host forms --
struct Stage {
    PinBuf pin;
    DevBuf dev;
    size_t fill = 0;  // bytes of pieces per fill, a multiple of 64
};
Stage* g_stage;  // one per logical device, each used under its device's mutex
std::once_flag g_stage_once;

Stage& stage_of(Device& D) {
    std::call_once(g_stage_once, [] { g_stage = new Stage[std::max(1, device_count())]; });
    Stage& S = g_stage[&D - g_dev];
    if (!S.fill) {
        const uint64_t mib = std::min<uint64_t>(4096, std::max<uint64_t>(1, env_u64("SHA1CHUNK_UPDATE_FILL_MIB", 256)));
        S.fill = static_cast<size_t>(mib) << 20;
    }
    return S;
}

struct HostEntry {
    size_t ctx;          // context index in the caller's array
    const uint8_t* src;  // piece
    uint32_t len;
};

// One fill: the entries' contexts and pieces up, the device form, the
// contexts back into the caller's array.
int run_update_fill(Device& D, Stage& S, uint8_t* contexts, const HostEntry* e, size_t m, size_t data_bytes) {
    const size_t off_at = round_up(m * kCtx, 8), len_at = off_at + m * 8;
    const size_t data_at = round_up(len_at + m * 4, kAlign), bytes = data_at + data_bytes;
    int rc;
    if ((rc = S.pin.ensure(bytes)) || (rc = S.dev.ensure(bytes))) return rc;
    uint8_t* h = static_cast<uint8_t*>(S.pin.p);
    uint8_t* d = static_cast<uint8_t*>(S.dev.p);
    uint64_t* hoff = reinterpret_cast<uint64_t*>(h + off_at);
    uint32_t* hlen = reinterpret_cast<uint32_t*>(h + len_at);
    size_t cur = data_at;
    for (size_t j = 0; j < m; ++j) {
        memcpy(h + j * kCtx, contexts + e[j].ctx * kCtx, kCtx);
        hoff[j] = cur;
        hlen[j] = e[j].len;
        if (e[j].len) memcpy(h + cur, e[j].src, e[j].len);
        cur += round_up(e[j].len, 16);
    }
    hipStream_t st = D.slot[0].stream;
    HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
    UpdateArgs U = context_args(d, m, nullptr, m);
    U.base = d;
    U.off = reinterpret_cast<const uint64_t*>(d + off_at);
    U.len = reinterpret_cast<const uint32_t*>(d + len_at);
    if ((rc = enqueue_update(D, U, st))) return rc;
    HIP_TRY(hipMemcpyAsync(h, d, m * kCtx, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < m; ++j) memcpy(contexts + e[j].ctx * kCtx, h + j * kCtx, kCtx);
    return SHA1CHUNK_OK;
}

int update_host(uint8_t* contexts, size_t n_contexts, const uint32_t* index, const uint8_t* base,
                const uint64_t* offsets, const uint32_t* lengths, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if ((index ? index[i] : i) >= n_contexts)
            return fail(SHA1CHUNK_EINVAL, "entry %zu: context index outside the %zu contexts", i, n_contexts);
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    if ((rc = discard_in_flight(*D))) return rc;
    Stage& S = stage_of(*D);
    std::vector<HostEntry> fill;
    size_t bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        const HostEntry en{index ? index[i] : i, base + offsets[i], lengths[i]};
        const size_t padded = round_up(en.len, 16);
        if (!fill.empty() && (bytes + padded > S.fill || fill.size() == kMaxFillEntries)) {
            if ((rc = run_update_fill(*D, S, contexts, fill.data(), fill.size(), bytes))) return rc;
            fill.clear();
            bytes = 0;
        }
        if (padded > S.fill) {
            // a piece larger than a fill: successive updates of its context,
            // cut at multiples of 64 bytes (S.fill is one)
            for (size_t at = 0; at < en.len; at += S.fill) {
                const HostEntry seg{en.ctx, en.src + at, static_cast<uint32_t>(std::min<size_t>(S.fill, en.len - at))};
                if ((rc = run_update_fill(*D, S, contexts, &seg, 1, round_up(seg.len, 16)))) return rc;
            }
            continue;
        }
        fill.push_back(en);
        bytes += padded;
    }
    if (!fill.empty()) rc = run_update_fill(*D, S, contexts, fill.data(), fill.size(), bytes);
    return rc;
}

int final_host(uint8_t* contexts, size_t n_contexts, const uint32_t* index, size_t n, uint8_t* digests) {
    for (size_t i = 0; i < n; ++i)
        if ((index ? index[i] : i) >= n_contexts)
            return fail(SHA1CHUNK_EINVAL, "entry %zu: context index outside the %zu contexts", i, n_contexts);
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    if ((rc = discard_in_flight(*D))) return rc;
    Stage& S = stage_of(*D);
    hipStream_t st = D->slot[0].stream;
    for (size_t lo = 0; lo < n; lo += kMaxFillEntries) {
        const size_t m = std::min(kMaxFillEntries, n - lo);
        const size_t dig_at = round_up(m * kCtx, 8), bytes = dig_at + m * 20;
        if ((rc = S.pin.ensure(bytes)) || (rc = S.dev.ensure(bytes))) return rc;
        uint8_t* h = static_cast<uint8_t*>(S.pin.p);
        uint8_t* d = static_cast<uint8_t*>(S.dev.p);
        for (size_t j = 0; j < m; ++j) memcpy(h + j * kCtx, contexts + (index ? index[lo + j] : lo + j) * kCtx, kCtx);
        HIP_TRY(hipMemcpyAsync(d, h, m * kCtx, hipMemcpyHostToDevice, st));
        UpdateArgs U = context_args(d, m, nullptr, m);
        U.dig = d + dig_at;
        if ((rc = launched(launch_update_final(U, st), "final launch"))) return rc;
        HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t j = 0; j < m; ++j) memcpy(contexts + (index ? index[lo + j] : lo + j) * kCtx, h + j * kCtx, kCtx);
        if (digests) memcpy(digests + 20 * lo, h + dig_at, m * 20);
    }
    return SHA1CHUNK_OK;
}
}  // namespace

// ================================================================ C ABI ====
extern "C" {

int s1be_init_device_async(void* d_contexts, size_t n_contexts, const uint32_t* d_index, size_t n, void* stream) {
    if (n == 0) return SHA1CHUNK_OK;
    if (!d_contexts) return fail(SHA1CHUNK_EINVAL, "null device pointer");
    if (int rc = check_count(n)) return rc;
    Device* D;
    if (int rc = get_device(&D)) return rc;
    return launched(launch_update_init(context_args(d_contexts, n_contexts, d_index, n), static_cast<hipStream_t>(stream)),
                    "init launch");
}

int s1be_update_device_async(void* d_contexts, size_t n_contexts, const uint32_t* d_index, const void* d_base,
                             const uint64_t* d_offsets, const uint32_t* d_lengths, size_t n, void* stream) {
    if (n == 0) return SHA1CHUNK_OK;
    if (!d_contexts || !d_base || !d_offsets || !d_lengths) return fail(SHA1CHUNK_EINVAL, "null device pointer");
    if (int rc = check_count(n)) return rc;
    Device* D;
    if (int rc = get_device(&D)) return rc;
    UpdateArgs U = context_args(d_contexts, n_contexts, d_index, n);
    U.base = static_cast<const uint8_t*>(d_base);
    U.off = d_offsets;
    U.len = d_lengths;
    return enqueue_update(*D, U, static_cast<hipStream_t>(stream));
}

int s1be_final_device_async(void* d_contexts, size_t n_contexts, const uint32_t* d_index, size_t n, uint8_t* d_digests,
                            void* stream) {
    if (n == 0) return SHA1CHUNK_OK;
    if (!d_contexts) return fail(SHA1CHUNK_EINVAL, "null device pointer");
    if (int rc = check_count(n)) return rc;
    if (reinterpret_cast<uintptr_t>(d_digests) & 3u) return fail(SHA1CHUNK_EALIGN, "digest buffer must be 4-byte aligned");
    Device* D;
    if (int rc = get_device(&D)) return rc;
    UpdateArgs U = context_args(d_contexts, n_contexts, d_index, n);
    U.dig = d_digests;
    return launched(launch_update_final(U, static_cast<hipStream_t>(stream)), "final launch");
}

int s1be_update_batch(void* contexts, size_t n_contexts, const uint32_t* index, const void* base,
                      const uint64_t* offsets, const uint32_t* lengths, size_t n, unsigned flags) {
    if (n == 0) return SHA1CHUNK_OK;
    if (!contexts || !base || !offsets || !lengths) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (flags & ~SHA1CHUNK_DEVICE) return fail(SHA1CHUNK_EINVAL, "flags: SHA1CHUNK_HOST or SHA1CHUNK_DEVICE");
    if (int rc = check_count(n)) return rc;
    if (flags & SHA1CHUNK_DEVICE) {
        Device* D;
        int rc = get_device(&D);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(D->mu);
        hipStream_t st = D->slot[0].stream;
        if ((rc = s1be_update_device_async(contexts, n_contexts, index, base, offsets, lengths, n, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return SHA1CHUNK_OK;
    }
    return update_host(static_cast<uint8_t*>(contexts), n_contexts, index, static_cast<const uint8_t*>(base), offsets,
                       lengths, n);
}

int s1be_final_batch(void* contexts, size_t n_contexts, const uint32_t* index, size_t n, uint8_t* digests,
                     unsigned flags) {
    if (n == 0) return SHA1CHUNK_OK;
    if (!contexts) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (flags & ~SHA1CHUNK_DEVICE) return fail(SHA1CHUNK_EINVAL, "flags: SHA1CHUNK_HOST or SHA1CHUNK_DEVICE");
    if (int rc = check_count(n)) return rc;
    if (flags & SHA1CHUNK_DEVICE) {
        Device* D;
        int rc = get_device(&D);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(D->mu);
        hipStream_t st = D->slot[0].stream;
        if ((rc = s1be_final_device_async(contexts, n_contexts, index, n, digests, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return SHA1CHUNK_OK;
    }
    return final_host(static_cast<uint8_t*>(contexts), n_contexts, index, n, digests);
}

}  // extern "C"
