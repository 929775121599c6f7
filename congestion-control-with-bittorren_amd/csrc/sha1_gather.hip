// sha1_gather.hip -- reassembly of messages given as segment lists
// (include/sha1chunk.h, sha1chunk_gather_device_async and the hash / verify
// forms built on it; host side in rt_gather.hip).
//
// Two plain, finite kernels on one stream (no kernel spins or waits on
// memory):
//   scan  one wave per message: the exclusive prefix of its segments' lengths
//         (pos[s], 32 bits, 64 segments per step), its 64-bit total and the
//         skip decision; writes the length word (the total, or 0xFFFFFFFF for
//         a skipped message) into scratch and the caller's array;
//   copy  output-centric: a workgroup owns 4 KiB tiles of one message's
//         destination (tile t, t + gridDim.y, ...); each thread finds the
//         segment of its aligned 16-byte word by binary search in pos[] -- in
//         a copy of the message's positions in LDS, or for a message of more
//         than 2048 segments inside the tile's segment range, which two
//         threads find first -- walks forward across seams and stores the
//         word; the workgroups of tile slot 0 also store the message's head
//         and tail bytes.
// The arithmetic of `copy` -- which words are loaded and stored -- is
// gather_map.hpp (replayed on the CPU by tools/gather_map_check.cc).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gather_map.hpp"
#include "sha1_kernels.h"

using namespace s1ga;

namespace {

constexpr int kGatherThreads = 256;
constexpr uint32_t kStagedSegments = 2048;  // positions of one message kept in LDS (8 KiB)
constexpr uint32_t kMaxGridX = 1u << 20;  // messages (copy) or groups of four (scan) per launch; the rest by stride

__global__ __launch_bounds__(kGatherThreads) void gather_scan_kernel(GatherArgs G) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (kGatherThreads / 64);
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * (kGatherThreads / 64) + wave; i < G.n; i += stride) {
        const uint32_t first = __builtin_amdgcn_readfirstlane(G.seg_first[i]);
        const uint32_t end = __builtin_amdgcn_readfirstlane(G.seg_first[i + 1]);
        uint32_t word = kSkipped;
        if (!skip_range(first, end, G.n_segments)) {
            unsigned long long run = 0;
            for (uint64_t s0 = first; s0 < end; s0 += 64) {
                const uint64_t s = s0 + lane;
                const unsigned long long L = s < end ? G.seg_len[s] : 0u;
                unsigned long long inc = L;  // inclusive prefix over the wave
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned long long o = __shfl_up(inc, d, 64);
                    if (lane >= static_cast<uint32_t>(d)) inc += o;
                }
                if (s < end) G.pos[s] = static_cast<uint32_t>(run + inc - L);
                run += __shfl(inc, 63, 64);
            }
            if (!skip_total(run, G.dst_off[i], G.dst_bytes)) word = static_cast<uint32_t>(run);
        }
        if (lane == 0) {
            G.mlen[i] = word;
            if (G.out_len) G.out_len[i] = word;
            if (word == kSkipped) atomicAdd(G.skipped, 1u);
        }
    }
}

// The copy kernel's memory: addresses are global memory (device memory or
// mapped host memory), so the accesses are global_load / global_store.
#define S1GA_GLOBAL __attribute__((address_space(1)))
struct DevMem {
    __device__ __forceinline__ uint32_t load32(uint64_t a) const {
        return *reinterpret_cast<const S1GA_GLOBAL uint32_t*>(a);
    }
    __device__ __forceinline__ void store8(uint64_t a, uint32_t v) const {
        *reinterpret_cast<S1GA_GLOBAL uint8_t*>(a) = static_cast<uint8_t>(v);
    }
    __device__ __forceinline__ void store128(uint64_t a, const uint32_t (&w)[4]) const {
        typedef uint32_t word4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<S1GA_GLOBAL word4*>(a) = word4{w[0], w[1], w[2], w[3]};
    }
};

__global__ __launch_bounds__(kGatherThreads) void gather_copy_kernel(GatherArgs G) {
    __shared__ uint32_t staged_pos[kStagedSegments];
    __shared__ uint32_t seg_lo, seg_hi;
    DevMem mem;
    for (uint64_t i = blockIdx.x; i < G.n; i += gridDim.x) {
        const uint32_t total = G.mlen[i];
        if (total == kSkipped || total == 0u) continue;  // the same in every thread of the workgroup
        const uint32_t first = G.seg_first[i], count = G.seg_first[i + 1] - first;
        // A message of up to kStagedSegments segments (a 512 KiB chunk has 354)
        // keeps its positions in LDS: every thread then searches all of them on
        // its own, and the tiles need no barrier.
        const bool staged = count <= kStagedSegments;
        if (staged) {
            __syncthreads();  // the previous message's searches are over
            for (uint32_t k = threadIdx.x; k < count; k += kGatherThreads) staged_pos[k] = G.pos[first + k];
            __syncthreads();
        }
        Msg M;  // its segments renumbered 0 .. count-1
        M.base = reinterpret_cast<uint64_t>(G.base);
        M.off = G.seg_off + first;
        M.len = G.seg_len + first;
        M.pos = staged ? staged_pos : G.pos + first;
        M.first = 0;
        M.end = count;
        M.total = total;
        M.dst = reinterpret_cast<uint64_t>(G.dst) + G.dst_off[i];
        const Plan P = store_plan(M.dst, total);
        if (blockIdx.y == 0 && threadIdx.x < 32u) copy_edge(mem, M, P, threadIdx.x);
        Tile T;
        if (staged) {
            for (uint32_t t = blockIdx.y; tile_words(P, t, T); t += gridDim.y)
                if (T.w0 + threadIdx.x < T.w1) copy_word(mem, M, P, T.w0 + threadIdx.x, M.first, M.end);
            continue;
        }
        // longer lists: the tile's segments are found once, by two threads
        for (uint32_t t = blockIdx.y; tile_words(P, t, T); t += gridDim.y) {
            if (threadIdx.x == 0) seg_lo = tile_first_segment(M, P, T);
            if (threadIdx.x == 64) seg_hi = tile_end_segment(M, P, T);
            __syncthreads();
            const uint32_t lo = seg_lo, hi = seg_hi;
            if (T.w0 + threadIdx.x < T.w1) copy_word(mem, M, P, T.w0 + threadIdx.x, lo, hi);
            __syncthreads();  // seg_lo / seg_hi are rewritten by the next tile
        }
    }
}

}  // namespace

hipError_t launch_gather_scan(const GatherArgs& G, hipStream_t st) {
    if (G.n == 0) return hipSuccess;
    const uint64_t groups = (static_cast<uint64_t>(G.n) + 3u) / 4u;
    const uint32_t grid = static_cast<uint32_t>(groups < kMaxGridX ? groups : kMaxGridX);
    hipLaunchKernelGGL(gather_scan_kernel, dim3(grid), dim3(kGatherThreads), 0, st, G);
    return hipGetLastError();
}

// Tile slots per message: enough workgroups for the device when the messages
// are few (a lone message is spread over 64), one per message when they are
// many (a workgroup then walks all of its message's tiles).
hipError_t launch_gather_copy(const GatherArgs& G, hipStream_t st) {
    if (G.n == 0) return hipSuccess;
    const uint32_t gx = G.n < kMaxGridX ? G.n : kMaxGridX;
    const uint32_t want = 4096u / gx;
    const uint32_t gy = want < 1u ? 1u : want > 64u ? 64u : want;
    hipLaunchKernelGGL(gather_copy_kernel, dim3(gx, gy), dim3(kGatherThreads), 0, st, G);
    return hipGetLastError();
}
