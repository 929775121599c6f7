// sha1_index.hip -- the digest index: which position of a table of m digests
// holds a queried digest (include/sha1chunk.h, "Digest index"; host side in
// rt_index.hip).  The arithmetic -- array size, home slot, probe step, insert
// and lookup -- is index_map.hpp, run on the CPU by tools/index_map_check.cc.
//
// Four plain, finite kernels (no kernel spins or waits on memory):
//   build   one lane per table entry.  The lanes of all workgroups race on the
//           slot array, and the XCDs' L2s are not coherent for plain accesses
//           inside a kernel, so EVERY access to a slot here is an agent-scope
//           atomic (a compare-and-swap of empty -> own position, a minimum
//           where the lane's own digest is in place already); the kernel has
//           no plain load or store of a slot.  The table is read only, with
//           plain loads.  The three counters are agent-scope atomics too.
//   append  the build with a base and a skip array: one lane per new entry,
//           the same insert.  The rows of a call are written by an earlier
//           operation on the stream (a copy into the table), so every table
//           row a lane reads -- its own, and those of other new entries that
//           it meets while probing -- was complete before the launch; no lane
//           reads a row that the same launch wrote.
//   rehash  growth: one lane per slot of the old array, which an earlier
//           kernel filled (plain loads); what the slot holds is inserted into
//           the new array with the same atomics.
//   lookup  a later kernel: one lane per query, five dword loads of the
//           digest, then plain loads of slots and table words.  No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_map.hpp"
#include "sha1_kernels.h"

using namespace s1ix;

namespace {

constexpr int kIndexThreads = 256;

// The build's slot array: agent-scope atomics, per lane.
struct AtomicSlots {
    uint32_t* s;
    __device__ __forceinline__ uint32_t claim(uint32_t h, uint32_t p) const {
        uint32_t held = kEmpty;  // left alone when the exchange happens
        (void)__hip_atomic_compare_exchange_strong(s + h, &held, p, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
        return held;
    }
    __device__ __forceinline__ void lower(uint32_t h, uint32_t p) const {
        (void)__hip_atomic_fetch_min(s + h, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The finished array, read by a later kernel.
struct LoadedSlots {
    const uint32_t* s;
    __device__ __forceinline__ uint32_t load(uint32_t h) const { return s[h]; }
};

// Entry p of the table into the slot array, counted in X.stats: the body of
// the build and of the append.
__device__ __forceinline__ void insert_counted(const IndexArgs& X, uint32_t p) {
    const Probe r = insert(AtomicSlots{X.slots}, X.mask, X.table, p);
    if (r.visited > 1u)  // the host starts the maximum at 1 for a table that is not empty
        (void)__hip_atomic_fetch_max(X.stats, static_cast<unsigned long long>(r.visited), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    if (r.duplicate) (void)__hip_atomic_fetch_add(X.stats + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r.wrapped) (void)__hip_atomic_fetch_add(X.stats + 2, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kIndexThreads) void index_build_kernel(IndexArgs X) {
    const uint32_t p = blockIdx.x * kIndexThreads + threadIdx.x;
    if (p >= X.m) return;
    insert_counted(X, p);
}

// The build with a base and a skip array: entry i of the call is table row
// base + i (base + k <= 2^31, so the sum fits).
__global__ __launch_bounds__(kIndexThreads) void index_append_kernel(IndexArgs X, uint32_t base, uint32_t k,
                                                                     const uint8_t* skip) {
    const uint32_t i = blockIdx.x * kIndexThreads + threadIdx.x;
    if (i >= k) return;
    if (skip && skip[i]) return;
    insert_counted(X, base + i);
}

// Growth: one lane per slot of the old array (plain loads: an earlier kernel
// filled it), agent-scope atomics on the new one.  Not counted.
__global__ __launch_bounds__(kIndexThreads) void index_rehash_kernel(IndexArgs X, const uint32_t* old_slots,
                                                                     uint32_t old_mask) {
    // at most 2^32 slots in whole workgroups: the last index still fits 32 bits
    const uint32_t s = blockIdx.x * kIndexThreads + threadIdx.x;
    if (s > old_mask) return;
    rehash_slot(LoadedSlots{old_slots}, s, AtomicSlots{X.slots}, X.mask, X.table);
}

__global__ __launch_bounds__(kIndexThreads) void index_lookup_kernel(IndexArgs X, const uint32_t* queries, uint32_t n,
                                                                     uint32_t* ids) {
    // n <= 2^32 - 256, so the rounded-up grid's last index still fits 32 bits
    const uint32_t i = blockIdx.x * kIndexThreads + threadIdx.x;
    if (i >= n) return;
    ids[i] = lookup(LoadedSlots{X.slots}, X.mask, X.table, queries + static_cast<uint64_t>(kWords) * i);
}

}  // namespace

hipError_t launch_index_build(const IndexArgs& X, hipStream_t st) {
    if (X.m == 0) return hipSuccess;
    if (X.m > kMaxEntries) return hipErrorInvalidValue;
    const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(X.m) + kIndexThreads - 1) / kIndexThreads);
    hipLaunchKernelGGL(index_build_kernel, dim3(grid), dim3(kIndexThreads), 0, st, X);
    return hipGetLastError();
}

hipError_t launch_index_lookup(const IndexArgs& X, const uint32_t* queries, uint32_t n, uint32_t* ids,
                               hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (n > kMaxQueries) return hipErrorInvalidValue;
    const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(n) + kIndexThreads - 1) / kIndexThreads);
    hipLaunchKernelGGL(index_lookup_kernel, dim3(grid), dim3(kIndexThreads), 0, st, X, queries, n, ids);
    return hipGetLastError();
}

hipError_t launch_index_append(const IndexArgs& X, uint32_t base, uint32_t k, const uint8_t* skip, hipStream_t st) {
    if (k == 0) return hipSuccess;
    if (static_cast<uint64_t>(base) + k > kMaxEntries) return hipErrorInvalidValue;
    const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(k) + kIndexThreads - 1) / kIndexThreads);
    hipLaunchKernelGGL(index_append_kernel, dim3(grid), dim3(kIndexThreads), 0, st, X, base, k, skip);
    return hipGetLastError();
}

hipError_t launch_index_rehash(const IndexArgs& X, const uint32_t* old_slots, uint32_t old_mask, hipStream_t st) {
    const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(old_mask) + kIndexThreads) / kIndexThreads);
    hipLaunchKernelGGL(index_rehash_kernel, dim3(grid), dim3(kIndexThreads), 0, st, X, old_slots, old_mask);
    return hipGetLastError();
}
