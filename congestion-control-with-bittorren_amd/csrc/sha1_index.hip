// sha1_index.hip -- the digest index: which position of a table of m digests
// holds a queried digest (include/sha1chunk.h, "Digest index"; host side in
// rt_index.hip).  The arithmetic -- array size, home slot, probe step, insert
// and lookup -- is index_map.hpp, run on the CPU by tools/index_map_check.cc.
//
// Two plain, finite kernels (no kernel spins or waits on memory):
//   build   one lane per table entry.  The lanes of all workgroups race on the
//           slot array, and the XCDs' L2s are not coherent for plain accesses
//           inside a kernel, so EVERY access to a slot here is an agent-scope
//           atomic (a compare-and-swap of empty -> own position, a minimum
//           where the lane's own digest is in place already); the kernel has
//           no plain load or store of a slot.  The table is read only, with
//           plain loads.  The three counters are agent-scope atomics too.
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

__global__ __launch_bounds__(kIndexThreads) void index_build_kernel(IndexArgs X) {
    const uint32_t p = blockIdx.x * kIndexThreads + threadIdx.x;
    if (p >= X.m) return;
    const Probe r = insert(AtomicSlots{X.slots}, X.mask, X.table, p);
    if (r.visited > 1u)  // the host starts the maximum at 1 for a table that is not empty
        (void)__hip_atomic_fetch_max(X.stats, static_cast<unsigned long long>(r.visited), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    if (r.duplicate) (void)__hip_atomic_fetch_add(X.stats + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r.wrapped) (void)__hip_atomic_fetch_add(X.stats + 2, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
