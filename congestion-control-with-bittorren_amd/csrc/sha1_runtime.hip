// sha1_runtime.hip -- the HIP backend of libsha1chunk.so (built into
// libsha1chunk_hip.so): the device half of the C-ABI batch entry points of
// include/sha1chunk.h, exported as s1be_* and reached only through the thin
// C front end (frontend.c), which dlopen()s this library on the first call
// that needs the GPU and handles the host small-call paths itself.
//
// Per device: one compute stream per pipeline slot, a device arena and a
// pinned host arena for each of two slots, so that packing/reading batch b+1
// on the host, its H2D copy, the kernel of batch b and the D2H of digests
// overlap.  Everything that hashes runs on the GPU; the host only moves
// bytes and bookkeeping (sorting by length, packing, scattering digests).
// The device table and error text are in rt_device.hip, the stream/fd file
// pipeline in rt_file.hip, the verify queues in vq.hip and vq_persistent.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "sha1_runtime_internal.h"

using namespace s1rt;

namespace {
// Split-kernel shape: 4-block units (1 barrier per 4 blocks, the whole 160
// KiB LDS, two producers) at one group of 64 chunks per CU; at two groups per
// CU one 8-wave workgroup holding both, 2-block units, two producers per
// consumer sharing a SIMD and each consumer alone on its own (case 11:
// 10-11 % faster than two 2-wave workgroups, profiles/split_2prod_sweep_r01.json);
// else 1-block units (40 KiB).  Up to 16 chunks per CU (4096 chunks on 256
// CUs, BASELINE config 2, down to the one-chunk call) the quad shape: four
// lanes per chunk and 16 chunks per workgroup, so the consumer fetches a
// block's W+K with 5 LDS reads instead of 20 (sha1_split.hpp kVQuad).  That
// shape spreads 4096 chunks over every CU, so it counts only the CUs that
// no persistent verify-queue drain holds (a drain workgroup keeps its CU's
// whole LDS; two quad workgroups doubling up on a free CU put both
// consumers on one SIMD and run at half speed: 10.7 against 5.85 ms beside
// busy drains); with fewer CUs free, the shapes below as before.
// SHA1CHUNK_SPLIT_UNIT forces a shape for A/B
// runs: 1, 4, 11, 416 in the product library; the study's other shapes and
// variants only in the A/B library (`make ab`, sha1_kernels.h).  Forcing a
// shape this library does not hold fails the call (SHA1CHUNK_EINVAL,
// launch_checked) instead of timing some other kernel.
int split_unit(size_t n, int cus) {
    if (const char* e = getenv("SHA1CHUNK_SPLIT_UNIT")) return atoi(e);
    if ((n + 15) / 16 <= size_t(std::max(0, cus - drain_cus_held()))) return kSplitUnitQuad;
    const size_t groups = (n + 63) / 64;
    if (groups <= size_t(cus)) return 4;
    if (groups <= size_t(cus) * 2) return 11;
    return 1;
}

hipError_t launch(int kernel, const BatchArgs& A, int cus, hipStream_t st) {
    switch (kernel) {
    case SHA1CHUNK_KERNEL_LANE: return launch_lane(A, st);
    case SHA1CHUNK_KERNEL_FUSED: return launch_fused(A, st);
    case SHA1CHUNK_KERNEL_SPLIT: return launch_split(A, split_unit(A.n, cus), st);
    default: return hipErrorInvalidValue;
    }
}

// Checks every launch path shares (plain kernels and the mixed kernel):
// grid sizes are computed in 32 bits ((n + 255) / 256, (n + 63) / 64), and
// digests are stored as 32-bit words.
int check_batch(const BatchArgs& A) {
    if (A.n > 0xffffffffu - 1024u)
        return fail(SHA1CHUNK_EINVAL, "batch of %u chunks: at most 2^32 - 1025 per call", A.n);
    if (A.n > 0 && (reinterpret_cast<uintptr_t>(A.dig) & 3u))
        return fail(SHA1CHUNK_EALIGN, "digest buffer must be 4-byte aligned");
    return SHA1CHUNK_OK;
}
}  // namespace

namespace s1rt {
// Pick the kernel for a batch of n chunks on a device with `cus` CUs
// (crossovers measured on MI355X: profiles/sweep_r01.json,
// split_2prod_sweep_r01.json; DESIGN.md section 5, kernel table):
//  - up to 2 groups of 64 chunks per CU, each chunk's serial instruction
//    stream is the bound: the split kernel (rounds-only consumer wave alone
//    on its SIMD, two producer waves on others) is ~1.4x the fused kernel
//    per chunk;
//  - beyond that the SIMDs are busy and the split kernel's LDS hand-off and
//    barriers cost more than they save: the fused kernel (schedule + rounds
//    in one wave, 4 blocks of register prefetch) wins.
int choose_kernel(int kernel, size_t n, int cus) {
    if (kernel != SHA1CHUNK_KERNEL_AUTO) return kernel;
    // A/B and test hook: force one kernel behind every AUTO call site
    if (const char* f = getenv("SHA1CHUNK_FORCE_KERNEL")) {
        if (!strcmp(f, "lane")) return SHA1CHUNK_KERNEL_LANE;
        if (!strcmp(f, "fused")) return SHA1CHUNK_KERNEL_FUSED;
        if (!strcmp(f, "split")) return SHA1CHUNK_KERNEL_SPLIT;
    }
    const size_t groups = (n + 63) / 64;
    return groups <= size_t(cus) * 2 ? SHA1CHUNK_KERNEL_SPLIT : SHA1CHUNK_KERNEL_FUSED;
}

int launch_checked(int kernel, const BatchArgs& A, hipStream_t st, int cus) {
    if (kernel < SHA1CHUNK_KERNEL_LANE || kernel > SHA1CHUNK_KERNEL_SPLIT)
        return fail(SHA1CHUNK_EINVAL, "unknown kernel id %d", kernel);
    if (int rc = check_batch(A)) return rc;
    if (kernel == SHA1CHUNK_KERNEL_SPLIT && !split_unit_built(split_unit(A.n, cus)))
        return fail(SHA1CHUNK_EINVAL, "split shape %d is not in this library (A/B shapes: `make ab`)",
                    split_unit(A.n, cus));
    hipError_t e = launch(kernel, A, cus, st);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "kernel launch: %s", hipGetErrorString(e));
    return SHA1CHUNK_OK;
}

// Mixed kernel for sorted ragged batches of more groups than CUs, unless an
// A/B hook forces a kernel behind AUTO (SHA1CHUNK_FORCE_KERNEL) or
// SHA1CHUNK_MIXED=0 turns it off (then AUTO's uniform-batch rule applies).
// SHA1CHUNK_MIXED=all also sends batches of <= CUs groups (every group its
// own CU at launch) through it (A/B).
bool use_mixed(size_t n, int cus) {
    if (getenv("SHA1CHUNK_FORCE_KERNEL")) return false;
    const char* e = getenv("SHA1CHUNK_MIXED");
    if (e && !strcmp(e, "0")) return false;
    if (e && !strcmp(e, "all")) return true;
    return (n + 63) / 64 > size_t(cus);
}

// SHA1CHUNK_MIXED_PLAN="mode,H,F" replaces the device-side plan (tests and
// A/B runs): mode 0 with H <= the model's head cap (min(groups, 4 CUs,
// 4096)) or H = groups, and F in {4, 8}; or mode 1.
// SHA1CHUNK_MIXED_DEBUG=1 prints the plan used (synchronises the stream:
// diagnostics only).
int launch_mixed_checked(const BatchArgs& A, const uint32_t* sorted_len, const BigFix* big, uint32_t* plan, int cus,
                         hipStream_t st) {
    if (int rc = check_batch(A)) return rc;
    int forced[3] = {0, 0, 0};
    bool force = false;
    if (const char* e = getenv("SHA1CHUNK_MIXED_PLAN")) {
        uint32_t hcap;
        const uint32_t groups = (A.n + 63u) / 64u;
        (void)mixed_grid(groups, cus, &hcap);
        if (sscanf(e, "%d,%d,%d", &forced[0], &forced[1], &forced[2]) != 3 || forced[0] < 0 ||
            forced[0] > 1 ||
            (forced[0] == 0 && (forced[1] < 0 || ((uint32_t)forced[1] > hcap && (uint32_t)forced[1] != groups) ||
                                (forced[2] != 4 && forced[2] != 8))))
            return fail(SHA1CHUNK_EINVAL,
                        "SHA1CHUNK_MIXED_PLAN=%s: want 0,H,F (0 <= H <= %u or H = %u, F 4|8) or 1,0,0", e,
                        hcap, groups);
        force = true;
    }
    hipError_t e = launch_mixed(A, sorted_len, big, plan, cus, force ? forced : nullptr, st);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "mixed kernel launch: %s", hipGetErrorString(e));
    if (const char* d = getenv("SHA1CHUNK_MIXED_DEBUG"); d && atoi(d)) {
        uint32_t p[28];
        HIP_TRY(hipMemcpyAsync(p, plan, sizeof p, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        fprintf(stderr, "sha1chunk mixed plan: n=%u groups=%u cus=%d mode=%u H=%u F=%u\n", A.n,
                (A.n + 63u) / 64u, cus, p[0], p[1], p[2]);
        if (!force && p[12])  // the planner's stage end times (us since its start; the first
                              // simulation sweep, pass 2's rest, pass 3's misses) and shader kcycles
            fprintf(stderr,
                    "sha1chunk mixed planner stages: scan %.1f bounds %.1f sweep %.1f pass2 %.1f pass3 %.1f us;"
                    " kcycles %.1f %.1f %.1f %.1f %.1f (bounds: run8 %.1f prefix %.1f search %.1f; first sweep:"
                    " list %.1f bounds %.1f packed %.1f, %u candidates, longest call %.1f)\n",
                    p[8] * 0.01, p[9] * 0.01, p[10] * 0.01, p[11] * 0.01, p[12] * 0.01, p[14] * 1e-3, p[15] * 1e-3,
                    p[16] * 1e-3, p[17] * 1e-3, p[18] * 1e-3, p[24] * 1e-3, p[25] * 1e-3, p[26] * 1e-3,
                    p[20] * 1e-3, p[21] * 1e-3, p[22] * 1e-3, p[23], p[27] * 1e-3);
    }
    return SHA1CHUNK_OK;
}

// Host memory the device reads in place (hipHostMalloc'd or registered).
bool host_pinned(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// Width of a device's pack pool (Device::pack), the caller included.
int pack_threads() {
    const char* e = getenv("SHA1CHUNK_COPY_THREADS");
    return e ? std::max(1, atoi(e)) : 8;
}
}  // namespace s1rt

namespace {
// ------------------------------------------------------------ host batch --
// Host batches go through two pipeline slots (own stream each), so the H2D
// copy of slot b+1 overlaps the kernel of slot b.  A slot's bytes come
// either straight from the caller's buffer (when it is pinned and the slot's
// chunks are back to back in it: one hipMemcpyAsync, no host copy) or are
// packed into the slot's pinned staging first.  Device layout of a slot:
//   [off: u64 x m][len: u32 x m] pad to 128 | chunk bytes
// Slot size scales with the batch: a pass of the kernel takes ~7 ms however
// few chunks it has (serial per chunk), so a slot must carry enough bytes
// that its PCIe copy, not the kernel, is the longer stage.
// SHA1CHUNK_HOST_SLOT_MIB (16..1024, read per call) fixes the slot size, so
// tests can wrap the two-slot ring many times over a modest batch.
size_t slot_bytes_for(uint64_t total) {
    if (const char* e = getenv("SHA1CHUNK_HOST_SLOT_MIB"))
        return std::min<size_t>(1024, std::max<size_t>(16, atoi(e))) << 20;
    const size_t lo = size_t(256) << 20, hi = size_t(1) << 30;
    return std::min(hi, std::max(lo, static_cast<size_t>(total / 4)));
}

// Pack entries [j0, j1) of a slot from pageable caller memory into pinned
// staging on the device's pack pool: one thread copies ~10 GB/s, well under
// the PCIe rate.  The entries are split into pool-width runs of about equal
// bytes.
void pack_range(PartPool& pool, uint8_t* h, const uint64_t* hoff, const uint8_t* base,
                const uint64_t* offsets, const uint32_t* lengths, const std::vector<uint32_t>& ids,
                size_t j0, size_t j1, size_t bytes) {
    const size_t T = std::min<size_t>(pool.width(), std::max<size_t>(1, bytes >> 23));
    std::vector<size_t> cut(T + 1, j1);
    cut[0] = j0;
    for (size_t t = 1, j = j0; t < T; ++t) {
        const uint64_t target = hoff[j0] + bytes * t / T;
        while (j < j1 && hoff[j] < target) ++j;
        cut[t] = j;
    }
    pool.run(T, [&](size_t t) {
        for (size_t j = cut[t]; j < cut[t + 1]; ++j)
            if (lengths[ids[j]]) memcpy(h + hoff[j], base + offsets[ids[j]], lengths[ids[j]]);
    });
}

int stage_and_launch(Device& D, Slot& s, const uint8_t* base, const uint64_t* offsets,
                     const uint32_t* lengths, const std::vector<uint32_t>& order, size_t lo,
                     size_t hi, size_t data_bytes, bool src_pinned, hipStream_t cs) {
    const size_t m = hi - lo;
    const size_t meta = round_up(m * (sizeof(uint64_t) + sizeof(uint32_t)), kAlign);
    int rc;
    s.ids.assign(order.begin() + lo, order.begin() + hi);
    // Direct mode: chunks contiguous and ascending in the pinned source, each
    // length a multiple of 16 (keeps every device chunk 16-byte aligned).
    bool direct = src_pinned;
    uint64_t span0 = offsets[s.ids[0]], span = 0;
    for (size_t j = 0; direct && j < m; ++j) {
        const uint32_t id = s.ids[j];
        direct = offsets[id] == span0 + span && (j + 1 == m || (lengths[id] & 15u) == 0);
        span += lengths[id];
    }
    const size_t dbytes = direct ? round_up(span, kAlign) : data_bytes;
    // SHA1CHUNK_HOST_DEBUG=1: one line per slot fill (tests check the mode
    // and the number of ring wraps; diagnostics only)
    if (const char* dbg = getenv("SHA1CHUNK_HOST_DEBUG"); dbg && atoi(dbg))
        fprintf(stderr, "sha1chunk host slot %d: %zu chunks %zu bytes %s\n",
                static_cast<int>(&s - D.slot), m, direct ? static_cast<size_t>(span) : data_bytes,
                direct ? "direct" : "packed");
    if ((rc = s.hpin.ensure(meta + (direct ? 0 : data_bytes))) || (rc = s.dmem.ensure(meta + dbytes)) ||
        (rc = s.hdig.ensure(m * 20)) || (rc = s.ddig.ensure(m * 20)))
        return rc;
    uint8_t* h = static_cast<uint8_t*>(s.hpin.p);
    uint64_t* hoff = reinterpret_cast<uint64_t*>(h);
    uint32_t* hlen = reinterpret_cast<uint32_t*>(h + m * sizeof(uint64_t));
    size_t cur = meta;
    for (size_t j = 0; j < m; ++j) {
        const uint32_t id = s.ids[j];
        const uint32_t L = lengths[id];
        hlen[j] = L;
        if (direct) {
            hoff[j] = meta + (offsets[id] - span0);
        } else {
            hoff[j] = cur;
            cur += round_up(L, kAlign);
        }
    }
    uint8_t* d = static_cast<uint8_t*>(s.dmem.p);
    if (direct) {
        HIP_TRY(hipMemcpyAsync(d, h, meta, hipMemcpyHostToDevice, cs));
        if (span) HIP_TRY(hipMemcpyAsync(d + meta, base + span0, span, hipMemcpyHostToDevice, cs));
    } else {
        // pack in runs of ~64 MiB and start each run's H2D as soon as it is
        // packed, so the copy engine works while the rest is packed
        if (!D.pack) D.pack.reset(new PartPool(pack_threads() - 1, near_cpus(D.id)));
        static const size_t piece = [] {  // SHA1CHUNK_PACK_PIECE_MIB, 0 = whole slot
            const char* e = getenv("SHA1CHUNK_PACK_PIECE_MIB");
            const size_t mib = e ? static_cast<size_t>(std::max(0, atoi(e))) : 64;
            return mib ? mib << 20 : ~size_t(0) >> 1;
        }();
        for (size_t j0 = 0; j0 < m;) {
            size_t j1 = j0 + 1;
            while (j1 < m && hoff[j1] - hoff[j0] < piece) ++j1;
            const size_t end = j1 < m ? hoff[j1] : cur;
            pack_range(*D.pack, h, hoff, base, offsets, lengths, s.ids, j0, j1, end - hoff[j0]);
            HIP_TRY(hipMemcpyAsync(d + hoff[j0], h + hoff[j0], end - hoff[j0], hipMemcpyHostToDevice, cs));
            j0 = j1;
        }
        HIP_TRY(hipMemcpyAsync(d, h, meta, hipMemcpyHostToDevice, cs));
    }
    if ((rc = copies_issued(s, cs))) return rc;
    BatchArgs A{};
    A.base = d;
    A.off = reinterpret_cast<const uint64_t*>(d);
    A.len = reinterpret_cast<const uint32_t*>(d + m * sizeof(uint64_t));
    A.n = static_cast<uint32_t>(m);
    A.dig = static_cast<uint8_t*>(s.ddig.p);
    // Entries are already in length order: no order[] indirection needed.
    if ((rc = launch_checked(choose_kernel(SHA1CHUNK_KERNEL_AUTO, m, D.cus), A, s.stream, D.cus)))
        return rc;
    HIP_TRY(hipMemcpyAsync(s.hdig.p, s.ddig.p, m * 20, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipEventRecord(s.done, s.stream));
    s.busy = true;
    return SHA1CHUNK_OK;
}

int drain(Slot& s, uint8_t* digests) {
    if (!s.busy) return SHA1CHUNK_OK;
    s.busy = false;
    HIP_TRY(hipEventSynchronize(s.done));
    const uint8_t* src = static_cast<const uint8_t*>(s.hdig.p);
    for (size_t j = 0; j < s.ids.size(); ++j) memcpy(digests + 20ull * s.ids[j], src + 20 * j, 20);
    return SHA1CHUNK_OK;
}

int hash_host(const uint8_t* base, const uint64_t* offsets, const uint32_t* lengths, size_t n,
              uint8_t* digests) {
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    if ((rc = discard_in_flight(*D))) return rc;
    // Longest first, so every wave of 64 gets near-equal lengths (a wave
    // runs as long as its longest lane); equal lengths keep caller order.
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return lengths[a] > lengths[b]; });
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += lengths[i];
    const size_t slot_cap = slot_bytes_for(total);
    const bool pinned = host_pinned(base);
    size_t lo = 0;
    int which = 0;
    while (lo < n) {
        size_t hi = lo, bytes = 0;
        while (hi < n) {
            const size_t b = round_up(lengths[order[hi]], kAlign);
            if (hi > lo && bytes + b > slot_cap) break;
            bytes += b;
            ++hi;
        }
        // A batch that fits one slot (a single chunk from shahash /
        // verify_hash) copies on slot 0's stream and creates no other stream;
        // larger ones share the copy stream and alternate two slots.
        const bool one_fill = lo == 0 && hi == n;
        if (!one_fill && ((rc = ensure_slots(*D, 2)) || (rc = ensure_copy(*D)))) return rc;
        Slot& s = D->slot[which];
        if ((rc = drain(s, digests))) return rc;
        if ((rc = stage_and_launch(*D, s, base, offsets, lengths, order, lo, hi, bytes, pinned,
                                   one_fill ? s.stream : D->copy)))
            return rc;
        lo = hi;
        which ^= 1;
    }
    if ((rc = drain(D->slot[which], digests))) return rc;
    return drain(D->slot[which ^ 1], digests);
}

// Shard a host batch over every device: contiguous, byte-balanced slices,
// one host thread per device, no collective.
int hash_host_all(const uint8_t* base, const uint64_t* offsets, const uint32_t* lengths, size_t n,
                  uint8_t* digests) {
    const int nd = device_count();
    if (nd <= 0) return fail(SHA1CHUNK_ENODEV, "%s", g_probe_err.c_str());
    if (nd == 1 || n < 64) return hash_host(base, offsets, lengths, n, digests);
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += lengths[i];
    std::vector<size_t> cut(nd + 1, n);
    cut[0] = 0;
    uint64_t acc = 0;
    int d = 1;
    for (size_t i = 0; i < n && d < nd; ++i) {
        acc += lengths[i];
        while (d < nd && acc >= total * (uint64_t)d / (uint64_t)nd) cut[d++] = i + 1;
    }
    std::vector<int> rcs(nd, 0);
    std::vector<std::string> errs(nd);
    std::vector<std::thread> th;
    for (int g = 0; g < nd; ++g) {
        th.emplace_back([&, g] {
            t_dev = g;
            const size_t a = cut[g], b = cut[g + 1];
            if (b > a) {
                std::vector<uint64_t> off(offsets + a, offsets + b);
                rcs[g] = hash_host(base, off.data(), lengths + a, b - a, digests + 20 * a);
                if (rcs[g]) errs[g] = s1be_last_error();
            }
        });
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < nd; ++g)
        if (rcs[g]) return fail(rcs[g], "device %d: %s", g, errs[g].c_str());
    return SHA1CHUNK_OK;
}

}  // namespace

// ================================================================ C ABI ====
extern "C" {

int s1be_hash_device_async(const void* d_base, const uint64_t* d_offsets,
                                const uint32_t* d_lengths, size_t n, uint8_t* d_digests,
                                void* stream, int kernel) {
    if (n > 0xffffffffu) return fail(SHA1CHUNK_EINVAL, "n too large");
    if (n && (!d_base || !d_offsets || !d_lengths || !d_digests))
        return fail(SHA1CHUNK_EINVAL, "null device pointer");
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    BatchArgs A{};
    A.base = static_cast<const uint8_t*>(d_base);
    A.off = d_offsets;
    A.len = d_lengths;
    A.n = static_cast<uint32_t>(n);
    A.dig = d_digests;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // AUTO on a ragged batch: hash longest-first (sha1_sort.hip); with more
    // groups of 64 than CUs, through the mixed kernel and its device-side
    // plan (sha1_kernels.hip, mixed).
    if ((rc = check_batch(A))) return rc;
    void* scratch = nullptr;
    if (kernel == SHA1CHUNK_KERNEL_AUTO && n > 64) {
        const uint32_t* sorted_len = nullptr;
        uint32_t* plan = nullptr;
        BigFix big{};
        const bool mixed = use_mixed(n, D->cus);
        // the mixed path re-ranks chunks of 4 MiB and more exactly (BigFix);
        // one group per CU or fewer hash all at once, where the grouping of
        // such chunks cannot change the batch's time
        hipError_t e = sort_by_length_desc(d_lengths, A.n, &A.order, &sorted_len, &plan, &scratch,
                                           mixed ? &big : nullptr, st);
        if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "length sort: %s", hipGetErrorString(e));
        if (mixed) {
            rc = launch_mixed_checked(A, sorted_len, &big, plan, D->cus, st);
            (void)hipFreeAsync(scratch, st);
            return rc;
        }
    }
    rc = launch_checked(choose_kernel(kernel, n, D->cus), A, st, D->cus);
    if (scratch) (void)hipFreeAsync(scratch, st);
    return rc;
}

int s1be_hash_uniform_async(const void* d_base, uint32_t chunk_len, size_t n,
                                 uint8_t* d_digests, void* stream, int kernel) {
    if (n > 0xffffffffu) return fail(SHA1CHUNK_EINVAL, "n too large");
    if (n && (!d_base || !d_digests)) return fail(SHA1CHUNK_EINVAL, "null device pointer");
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    BatchArgs A{};
    A.base = static_cast<const uint8_t*>(d_base);
    A.ulen = chunk_len;
    A.n = static_cast<uint32_t>(n);
    A.dig = d_digests;
    return launch_checked(choose_kernel(kernel, n, D->cus), A, static_cast<hipStream_t>(stream), D->cus);
}

// Diagnostics (tests; no frontend entry point): the longest-first order and
// sorted lengths AUTO's ragged path hashes a batch of lengths in
// (sha1_sort.hip), copied into the caller's device arrays of n entries.
int s1be_sort_order_async(const uint32_t* d_lengths, size_t n, uint32_t* d_order, uint32_t* d_sorted_len,
                          void* stream) {
    if (n > 0xffffffffu) return fail(SHA1CHUNK_EINVAL, "n too large");
    if (n == 0) return SHA1CHUNK_OK;
    if (!d_lengths || !d_order || !d_sorted_len) return fail(SHA1CHUNK_EINVAL, "null device pointer");
    Device* D;
    if (int rc = get_device(&D)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t *order = nullptr, *sorted_len = nullptr;
    uint32_t* plan = nullptr;
    void* scratch = nullptr;
    hipError_t e = sort_by_length_desc(d_lengths, static_cast<uint32_t>(n), &order, &sorted_len, &plan, &scratch,
                                       nullptr, st);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "length sort: %s", hipGetErrorString(e));
    (void)sorted_len;  // group heads only: every position's length is gathered below
    e = hipMemcpyAsync(d_order, order, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = gather_sorted_lengths(d_lengths, order, d_sorted_len, static_cast<uint32_t>(n), st);
    (void)hipFreeAsync(scratch, st);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "sort copy: %s", hipGetErrorString(e));
    return SHA1CHUNK_OK;
}

// Diagnostics (tests): the order the mixed path hashes a ragged batch in --
// the length sort, then the layout kernel's exact re-ranking of chunks of
// 4 MiB and more (BigFix) -- and the lengths in that order.  d_offsets: the
// batch's offsets (the layout summary reads them; no bytes are read).
int s1be_mixed_order_async(const uint32_t* d_lengths, const uint64_t* d_offsets, size_t n, uint32_t* d_order,
                           uint32_t* d_sorted_len, void* stream) {
    if (n > 0xffffffffu) return fail(SHA1CHUNK_EINVAL, "n too large");
    if (n == 0) return SHA1CHUNK_OK;
    if (!d_lengths || !d_offsets || !d_order || !d_sorted_len) return fail(SHA1CHUNK_EINVAL, "null device pointer");
    Device* D;
    if (int rc = get_device(&D)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    BatchArgs A{};
    A.base = reinterpret_cast<const uint8_t*>(d_offsets);  // addresses only, never read
    A.off = d_offsets;
    A.len = d_lengths;
    A.n = static_cast<uint32_t>(n);
    const uint32_t* sorted_len = nullptr;
    uint32_t* plan = nullptr;
    void* scratch = nullptr;
    BigFix big{};
    hipError_t e = sort_by_length_desc(d_lengths, A.n, &A.order, &sorted_len, &plan, &scratch, &big, st);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "length sort: %s", hipGetErrorString(e));
    e = launch_plan_layout(A, sorted_len, &big, plan, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_order, A.order, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = gather_sorted_lengths(d_lengths, A.order, d_sorted_len, A.n, st);
    (void)hipFreeAsync(scratch, st);
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "mixed order: %s", hipGetErrorString(e));
    return SHA1CHUNK_OK;
}

int s1be_compare_device_async(const uint8_t* d_digests, const uint8_t* d_expected, size_t n,
                                   uint8_t* d_mismatch, void* stream) {
    // 256 threads per workgroup, one per chunk: the launch rounds n up to whole
    // workgroups and holds fewer than 2^32 work-items
    if (n > 0xffffffffu - 255u) return fail(SHA1CHUNK_EINVAL, "n too large: at most 2^32 - 256 per call");
    if (n && (!d_digests || !d_expected || !d_mismatch))
        return fail(SHA1CHUNK_EINVAL, "null device pointer");
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    hipError_t e = launch_compare(d_digests, d_expected, static_cast<uint32_t>(n), d_mismatch,
                                  static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "compare launch: %s", hipGetErrorString(e));
    return SHA1CHUNK_OK;
}

int s1be_hash_batch(const void* base, const uint64_t* offsets, const uint32_t* lengths,
                         size_t n, uint8_t* digests, unsigned flags) {
    if (n == 0) return SHA1CHUNK_OK;
    if (!base || !offsets || !lengths || !digests) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (n > 0xffffffffu) return fail(SHA1CHUNK_EINVAL, "n too large");
    if (flags & SHA1CHUNK_DEVICE) {
        Device* D;
        int rc = get_device(&D);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(D->mu);
        hipStream_t st = D->slot[0].stream;
        if ((rc = s1be_hash_device_async(base, offsets, lengths, n, digests, st,
                                              SHA1CHUNK_KERNEL_AUTO)))
            return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return SHA1CHUNK_OK;
    }
    const uint8_t* b = static_cast<const uint8_t*>(base);
    if (flags & SHA1CHUNK_ALL_DEVICES) return hash_host_all(b, offsets, lengths, n, digests);
    return hash_host(b, offsets, lengths, n, digests);
}

int s1be_verify_batch(const void* base, const uint64_t* offsets, const uint32_t* lengths,
                           size_t n, const uint8_t* expected, uint8_t* mismatch, unsigned flags) {
    if (n == 0) return SHA1CHUNK_OK;
    if (!expected || !mismatch) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (flags & SHA1CHUNK_DEVICE) {
        Device* D;
        int rc = get_device(&D);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(D->mu);
        Slot& s = D->slot[0];
        if ((rc = s.ddig.ensure(n * 20))) return rc;
        if ((rc = s1be_hash_device_async(base, offsets, lengths, n,
                                              static_cast<uint8_t*>(s.ddig.p), s.stream,
                                              SHA1CHUNK_KERNEL_AUTO)))
            return rc;
        if ((rc = s1be_compare_device_async(static_cast<uint8_t*>(s.ddig.p), expected, n,
                                                 mismatch, s.stream)))
            return rc;
        HIP_TRY(hipStreamSynchronize(s.stream));
        return SHA1CHUNK_OK;
    }
    std::vector<uint8_t> dig(n * 20);
    int rc = s1be_hash_batch(base, offsets, lengths, n, dig.data(), flags);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) mismatch[i] = memcmp(&dig[20 * i], expected + 20 * i, 20) != 0;
    return SHA1CHUNK_OK;
}

int s1be_compress_blocks(uint32_t state[5], const void* blocks, size_t nblocks) {
    if (!state || (nblocks && !blocks)) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (nblocks == 0) return SHA1CHUNK_OK;
    if (nblocks * 64 > 0xffffffffull) return fail(SHA1CHUNK_EINVAL, "too many blocks");
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    const size_t bytes = nblocks * 64;
    if ((rc = D->small.ensure(64 + bytes)) || (rc = D->small_pin.ensure(64 + bytes))) return rc;
    uint8_t* h = static_cast<uint8_t*>(D->small_pin.p);
    memcpy(h, state, 20);
    memcpy(h + 64, blocks, bytes);
    hipStream_t st = D->slot[0].stream;
    HIP_TRY(hipMemcpyAsync(D->small.p, h, 64 + bytes, hipMemcpyHostToDevice, st));
    uint8_t* d = static_cast<uint8_t*>(D->small.p);
    BatchArgs A{};
    A.base = d + 64;
    A.ulen = static_cast<uint32_t>(bytes);
    A.n = 1;
    A.init_state = reinterpret_cast<const uint32_t*>(d);
    A.out_state = reinterpret_cast<uint32_t*>(d + 32);
    if ((rc = launch_checked(choose_kernel(SHA1CHUNK_KERNEL_AUTO, 1, D->cus), A, st, D->cus))) return rc;
    HIP_TRY(hipMemcpyAsync(h + 32, d + 32, 20, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(state, h + 32, 20);
    return SHA1CHUNK_OK;
}

int s1be_finish(const uint32_t state[5], uint64_t prefix_bytes, const void* tail,
                     uint32_t tail_len, uint8_t digest[20]) {
    if (!state || !digest || (tail_len && !tail) || tail_len >= 64)
        return fail(SHA1CHUNK_EINVAL, "bad argument");
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    if ((rc = D->small.ensure(256)) || (rc = D->small_pin.ensure(256))) return rc;
    uint8_t* h = static_cast<uint8_t*>(D->small_pin.p);
    memcpy(h, state, 20);
    if (tail_len) memcpy(h + 64, tail, tail_len);
    hipStream_t st = D->slot[0].stream;
    HIP_TRY(hipMemcpyAsync(D->small.p, h, 128, hipMemcpyHostToDevice, st));
    uint8_t* d = static_cast<uint8_t*>(D->small.p);
    BatchArgs A{};
    A.base = d + 64;
    A.ulen = tail_len;
    A.n = 1;
    A.init_state = reinterpret_cast<const uint32_t*>(d);
    A.prefix_bytes = prefix_bytes;
    A.dig = d + 128;
    if ((rc = launch_checked(SHA1CHUNK_KERNEL_LANE, A, st))) return rc;
    HIP_TRY(hipMemcpyAsync(h + 128, d + 128, 20, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(digest, h + 128, 20);
    return SHA1CHUNK_OK;
}

// One workgroup per chunk (launch_synth): a count one launch cannot express
// (kSynthMaxChunks, sha1_kernels.h) is refused, not truncated to 32 bits.
static int check_synth_count(uint64_t count) {
    if (count > kSynthMaxChunks)
        return fail(SHA1CHUNK_EINVAL, "synthetic fill of %llu chunks: at most %llu (2^24 - 1) per call",
                    static_cast<unsigned long long>(count), static_cast<unsigned long long>(kSynthMaxChunks));
    return SHA1CHUNK_OK;
}

int s1be_synth_fill_async(void* d_dst, uint64_t first, uint64_t count, uint32_t chunk_len,
                               uint64_t seed, void* stream) {
    if (count && !d_dst) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (int rc = check_synth_count(count)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_dst) & 7u) || (chunk_len & 7u && count > 1))
        return fail(SHA1CHUNK_EALIGN, "synthetic chunks must start 8-byte aligned");
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    hipError_t e = launch_synth(static_cast<uint8_t*>(d_dst), nullptr, nullptr, chunk_len, first,
                                count, seed, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "synth launch: %s", hipGetErrorString(e));
    return SHA1CHUNK_OK;
}

int s1be_synth_fill_ragged_async(void* d_base, const uint64_t* d_offsets,
                                      const uint32_t* d_lengths, uint64_t first, uint64_t count,
                                      uint64_t seed, void* stream) {
    if (count && (!d_base || !d_offsets || !d_lengths)) return fail(SHA1CHUNK_EINVAL, "null pointer");
    if (int rc = check_synth_count(count)) return rc;
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    hipError_t e = launch_synth(static_cast<uint8_t*>(d_base), d_offsets, d_lengths, 0, first,
                                count, seed, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(SHA1CHUNK_EHIP, "synth launch: %s", hipGetErrorString(e));
    return SHA1CHUNK_OK;
}

}  // extern "C"
