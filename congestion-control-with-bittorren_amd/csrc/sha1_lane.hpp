// sha1_lane.hpp -- what every gfx950 SHA-1 kernel's lane starts from: batch
// entries (and the checked build's index hooks), initial state and digest
// write-out, the per-lane block loop, wave-wide min/max/any/all, per-lane
// stage loads and the loads shared across a wave (coop_*, coop4_*).
// Included by sha1_split.hpp, sha1_fused.hpp and sha1_progress_shared.hip.
// Everything here is a template or internal to the including file.
#ifndef SHA1_LANE_HPP
#define SHA1_LANE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha1_device.hpp"
#include "sha1_kernels.h"

using namespace s1;

namespace {

struct Entry {
    uint32_t id;
    const uint8_t* p;
    uint32_t len;
};

#ifdef SHA1CHUNK_CHECKED
// The bounds-checked backend (`make checked`): every
// entry index and every A.order value is checked against the batch; a
// violation is counted here (read by s1be_checked_violations, sha1_kernels.hip),
// the first few printed, and the index clamped so the access stays inside
// the batch -- the run reports the bug instead of faulting the GPU.
__device__ unsigned int g_checked_oob;

__device__ __forceinline__ uint32_t checked_index(uint32_t i, uint32_t n, const char* what) {
    if (i < n) return i;
    if (atomicAdd(&g_checked_oob, 1u) < 8u)
        printf("sha1chunk checked: %s %u >= n %u (block %u, thread %u)\n", what, i, n, blockIdx.x, threadIdx.x);
    return n ? n - 1u : 0u;
}
#endif

__device__ __forceinline__ Entry fetch_entry(const BatchArgs& A, uint32_t e) {
    Entry r;
#ifdef SHA1CHUNK_CHECKED
    e = checked_index(e, A.n, "entry index");
    r.id = A.order ? checked_index(A.order[e], A.n, "A.order value") : e;
#else
    r.id = A.order ? A.order[e] : e;
#endif
    const uint64_t off = A.off ? A.off[r.id] : (uint64_t)r.id * A.ulen;
    r.p = A.base + off;
    r.len = A.len ? A.len[r.id] : A.ulen;
    return r;
}

// The entry a lane past the batch reads instead of its own (its loads are
// valid and unused): the group's first chunk, or -- for a group wholly past
// the batch (the empty second pair of a split workgroup when the group count
// is odd) -- the batch's last entry, never group*64, which indexes past
// A.order (round 5's fault, gpurun_out/pytest_sort16_r05.log; fixed in
// 2705501).  SHA1CHUNK_AB_UNCLAMPED puts the unclamped index back: only for
// the checked build's negative test (`make checked-unclamped`).
__device__ __forceinline__ uint32_t fallback_entry(const BatchArgs& A, uint32_t group) {
#ifdef SHA1CHUNK_AB_UNCLAMPED
    return group * 64u;
#else
    return min(group * 64u, A.n - 1u);
#endif
}

// A lane's entry and whether it is one of the batch's: a lane past the batch
// takes entry `fallback` with length 0.
__device__ __forceinline__ Entry lane_entry(const BatchArgs& A, uint32_t e, uint32_t fallback, bool& valid) {
    valid = e < A.n;
    Entry en = fetch_entry(A, valid ? e : fallback);
    if (!valid) en.len = 0;
    return en;
}

__device__ __forceinline__ void load_init(const BatchArgs& A, uint32_t id, uint32_t (&h)[5]) {
    if (A.init_state) {
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = A.init_state[5 * id + i];
    } else {
        init_state(h);
    }
}

__device__ __forceinline__ void emit(const BatchArgs& A, uint32_t id, const uint32_t (&h)[5]) {
    if (A.out_state) {
#pragma unroll
        for (int i = 0; i < 5; ++i) A.out_state[5 * id + i] = h[i];
    } else {
        store_digest(A.dig + 20ull * id, h);
    }
}

// Blocks [k0, nfull) of one lane straight from global memory (one block
// prefetched), then the padded tail (unless the batch is in update mode).
__device__ __forceinline__ void lane_loop(const Entry& en, uint32_t k0, uint32_t (&h)[5]) {
    const uint32_t nfull = en.len >> 6;
    uint32_t cur[16];
    if (k0 < nfull) load_block16(en.p + 64ull * k0, cur);
    for (uint32_t k = k0; k < nfull; ++k) {
        // swap into the schedule window first (other registers), then
        // refill `cur` with the next block in flight during the compression
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = bswap_fresh(cur[j]);
        if (k + 1 < nfull) load_block16(en.p + 64ull * (k + 1), cur);
        compress(h, w);
    }
}

__device__ __forceinline__ bool wave_all(bool x) { return __ballot(!x) == 0; }
__device__ __forceinline__ bool wave_any(bool x) { return __ballot(x) != 0; }

__device__ __forceinline__ void lane_blocks(const BatchArgs& A, const Entry& en, uint32_t k0,
                                            uint32_t (&h)[5]) {
    lane_loop(en, k0, h);
    const uint32_t nfull = en.len >> 6;
    if (!A.out_state)
        finish_message(h, en.p + 64ull * nfull, en.len & 63u, A.prefix_bytes + en.len);
}

__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = min(x, (uint32_t)__shfl_xor(x, m));
    return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = max(x, (uint32_t)__shfl_xor(x, m));
    return x;
}

// Bulk stages every lane has: the wave's fewest whole 128-byte stages.
__device__ __forceinline__ uint32_t bulk_stages(const Entry& en, bool valid) {
    return wave_any(valid) ? __builtin_amdgcn_readfirstlane(wave_min(valid ? (en.len >> 7) : 0xffffffffu)) : 0u;
}

// The four words of a 16-byte vector (uint4 or u32x4u; by value: a reference
// to the align-1 u32x4u draws -Walign-mismatch).
template <typename V>
__device__ __forceinline__ void unpack4(uint32_t* dst, V x) {
    dst[0] = x.x;
    dst[1] = x.y;
    dst[2] = x.z;
    dst[3] = x.w;
}

}  // namespace

// Two blocks (128 contiguous bytes) of one lane's chunk, loaded per lane.
struct Stage {
    uint32_t w[32];
};
// V: uint4 when every lane's chunk is 16-byte aligned (hipcc then keeps
// the stage in 64-bit register pairs: 8 fewer moves per block in the fused
// loop), u32x4u at any alignment.
template <typename V = u32x4u>
__device__ __forceinline__ void load_stage(const uint8_t* p, Stage& st) {
    const V* q = reinterpret_cast<const V*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) unpack4(st.w + 4 * j, q[j]);
}

// ------------------------------------------------------- shared loads ----
// Bulk loads shared across the wave: instruction i
// (i = 0..7) of a 128-byte stage reads 128 bytes of each of the group's
// chunks 8i .. 8i+7 (lane l: chunk 8i + l/8, 16-byte piece l%8), so one load
// instruction touches 8 chunks instead of 64, and an LDS transpose hands
// each lane its own chunk's 128 bytes.  The loads take chunks at any byte
// alignment (u32x4u, sha1_device.hpp).  The lane-per-chunk pattern makes
// each load instruction translate 64 addresses; with chunks far apart that
// thrashes the CU's translation cache: scattered 512 KiB chunks read at
// 1183 GB/s lane-per-chunk and 5954 GB/s 8 chunks per instruction (5036 /
// 5980 in place; tools/coop_probe.hip).  In the hash kernels: 65536 x
// 512 KiB with permuted offsets in 11.1 ms (fused tail) and 24.3 (one-group
// split) against 28.7 and 29.3 lane-per-chunk; 32768 in the 8-wave split
// 6.62 ms against 14.8; and in place the split shapes get ~1 % faster
// (config 2: 6.019 vs 6.067 ms; profiles/mixed_r02.json "coop").
// Swizzle: piece p of chunk c at c*128 + ((p + c/2) & 7)*16, conflict-free
// for the b128 stores (8 contiguous lanes write one chunk) and for the b128
// reads (each of ds_read_b128's 16-lane groups sees 16 distinct 16-byte
// bank groups).
constexpr uint32_t kCoopStageBytes = 64u * 128u;
// A fused wave's LDS in the mixed kernel: five 4 KiB block buffers of the
// LDS-DMA loop below (eight fused waves fill the workgroup's 160 KiB).
constexpr uint32_t kCoopBlockBytes = 64u * 64u;
constexpr uint32_t kCoopBlockBufs = 5u;
constexpr uint32_t kCoopWaveBytes = kCoopBlockBufs * kCoopBlockBytes;

// Orders one wave's LDS accesses across a transpose: lane-to-lane exchange
// through LDS (coop_store -> coop_read, and the reads of a buffer before its
// next stores).  The hardware completes a wave's LDS ops in order; this pins
// the program order in the compiler too (a wavefront-scope fence and the
// wave barrier pseudo-op: neither emits an instruction).
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t coop_slot(uint32_t c, uint32_t piece) {
    return c * 128u + ((piece + (c >> 1)) & 7u) * 16u;
}

// (the in-flight stage lives in plain 32-bit words: an array of uint4
// stays in scratch memory)
__device__ __forceinline__ void coop_load(const u32x4u* const (&src)[8], uint32_t s, uint32_t (&v)[32]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) unpack4(v + 4 * i, src[i][8u * s]);
}

__device__ __forceinline__ void coop_store(uint8_t* buf, const uint32_t (&v)[32], uint32_t lane) {
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i)
        *reinterpret_cast<uint4*>(buf + coop_slot(8u * i + lane / 8u, lane & 7u)) =
            make_uint4(v[4 * i + 0], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

__device__ __forceinline__ void coop_read(const uint8_t* buf, uint32_t lane, uint32_t (&w)[32]) {
#pragma unroll
    for (uint32_t p = 0; p < 8; ++p) unpack4(w + 4 * p, *reinterpret_cast<const uint4*>(buf + coop_slot(lane, p)));
}


// The same for one 64-byte block of the wave's 64 chunks (the split
// producers that own one block per unit): instruction i (i = 0..3) reads
// block k of chunks 16i .. 16i+15 (lane l: chunk 16i + l/4, 16-byte piece
// l%4), staged through 4 KiB of LDS.  Piece p of chunk c at
// c*64 + ((p + c/4) & 3)*16: conflict-free b128 stores and reads, and a
// lane's store address is the same for every i but for an i*1024 offset.
__device__ __forceinline__ void coop4_load(const u32x4u* const (&src)[4], uint32_t k, uint32_t (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) unpack4(v + 4 * i, src[i][4u * k]);
}

__device__ __forceinline__ void coop4_store(uint8_t* buf, const uint32_t (&v)[16], uint32_t lane) {
    const uint32_t at = (lane >> 2) * 64u + (((lane & 3u) + (lane >> 4)) & 3u) * 16u;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        *reinterpret_cast<uint4*>(buf + i * 1024u + at) =
            make_uint4(v[4 * i + 0], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

__device__ __forceinline__ void coop4_read(const uint8_t* buf, uint32_t lane, uint32_t (&w)[16]) {
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p)
        unpack4(w + 4 * p, *reinterpret_cast<const uint4*>(buf + lane * 64u + ((p + (lane >> 2)) & 3u) * 16u));
}

// Per-lane source pointers of the shared-load pattern with `lanes` lanes per
// chunk: slot i is chunk group*64 + (64/lanes)*i + lane/lanes, piece
// lane%lanes; a slot past the batch reads the group's first chunk (valid,
// and at least as long as the wave's bulk region).  A group wholly past the
// batch (the second pair of a split workgroup when the group count is odd)
// takes the batch's last entry instead: never group*64, which indexes past
// A.order, and its blocks are never loaded (no bulk region).
template <int LANES>
__device__ __forceinline__ void coop_sources(const BatchArgs& A, uint32_t group, uint32_t lane,
                                             const u32x4u* (&src)[LANES]) {
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)LANES; ++i) {
        const uint32_t ej = group * 64u + (64u / LANES) * i + lane / LANES;
        src[i] = reinterpret_cast<const u32x4u*>(fetch_entry(A, ej < A.n ? ej : fallback_entry(A, group)).p) + (lane % LANES);
    }
}

#endif
