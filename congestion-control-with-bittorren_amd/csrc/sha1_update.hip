// sha1_update.hip -- batched SHA1Init / SHA1Update / SHA1Final over an array
// of SHA1Context structs in device memory (include/sha1chunk.h,
// sha1chunk_update_device_async and its siblings; host side in rt_update.hip).
//
// One lane per entry; every kernel here is plain and finite (no kernel spins
// or waits on memory).  An update is three steps on one stream:
//   pre   joins each context's 0-63 staged bytes to its piece at any byte
//         alignment: compresses the completed head block, stages the residue,
//         adds the piece's bits to totalLength, and writes the chaining value
//         (packed, 5 words per entry) and the whole-block span (mid_off,
//         mid_len) into scratch;
//   bulk  the whole blocks, through the existing lane / fused / split kernels
//         in update mode (BatchArgs::init_state = out_state = the packed
//         array, in place): rt_update.hip launches it;
//   post  copies each entry's chaining value back into its context.
// The arithmetic of `pre` is update_split.hpp (checked on the CPU by
// tools/update_split_check.cc).
//
// Skipped entries (index >= n_contexts, or a context whose bufferLength is
// above 63): nothing is read or written through them; their scratch entry is
// an empty span, so the bulk kernels touch no piece byte for them either.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha1_device.hpp"
#include "sha1_kernels.h"
#include "update_split.hpp"

using namespace s1;
using namespace s1up;

namespace {

constexpr int kUpdateThreads = 256;

// Bytes [lo, hi) of a 64-byte window from src[0 .. hi - lo), as the window's
// 16 little-endian words; the other bytes of a word that holds some of them
// are whatever shares its aligned 4-byte word in memory, and words that hold
// none are zero and never loaded (load_block_partial's rule, with a start
// inside the window: lo = 0, hi = avail is that function).
__device__ __forceinline__ void load_window(const uint8_t* src, uint32_t lo, uint32_t hi, uint32_t (&w)[16]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) - lo;  // address of window byte 0 (never read below lo)
    const uint32_t sh = static_cast<uint32_t>(a & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
    uint32_t d[17];
#pragma unroll
    for (int j = 0; j < 17; ++j) d[j] = window_word_loaded(j, lo, hi, sh) ? q[j] : 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
}

// The context of entry i, or null when the entry is skipped for its index.
__device__ __forceinline__ uint8_t* entry_context(const UpdateArgs& U, uint32_t i) {
    const uint64_t c = U.index ? U.index[i] : i;
    return skip_index(c, U.n_contexts) ? nullptr : U.ctx + c * kContextBytes;
}

__global__ __launch_bounds__(kUpdateThreads) void sha1_update_pre_kernel(UpdateArgs U) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U.n) return;
    uint32_t h[5] = {0u, 0u, 0u, 0u, 0u};
    uint64_t mid_off = 0;
    uint32_t mid_len = 0;
    uint8_t* ctx = entry_context(U, i);
    const uint32_t b = ctx ? *reinterpret_cast<const uint32_t*>(ctx + kOffBufferLength) : 64u;
    if (!skip_staged(b)) {
        const uint32_t L = U.len[i];
        const uint64_t off = U.off[i];
        const uint8_t* p = U.base + off;
        const Split s = split_piece(b, L);
        uint64_t* total = reinterpret_cast<uint64_t*>(ctx + kOffTotal);
        *total += static_cast<uint64_t>(L) * 8u;
        const uint32_t* hw = reinterpret_cast<const uint32_t*>(ctx + kOffHash);
#pragma unroll
        for (int k = 0; k < 5; ++k) h[k] = hw[k];
        // The staged bytes are read into registers here, before anything is
        // stored to the buffer: the head block below and the bytes kept under
        // a short piece both come from `staged`.
        uint32_t* buf = reinterpret_cast<uint32_t*>(ctx + kOffBuffer);
        uint32_t staged[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) staged[k] = buf[k];
        if (s.head) {
            // buffer[0 .. b) then piece[0 .. 64 - b): one block
            uint32_t w[16];
            load_window(p, b, 64u, w);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t keep = keep_mask(k, b);
                w[k] = bswap((staged[k] & keep) | (w[k] & ~keep));
            }
            compress(h, w);
        }
        if (s.copy_len) {
            const uint32_t lo = s.copy_dst, hi = s.copy_dst + s.copy_len;
            uint32_t w[16];
            load_window(p + s.copy_src, lo, hi, w);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (word_touched(k, lo, hi)) {
                    const uint32_t keep = keep_mask(k, lo);
                    buf[k] = (staged[k] & keep) | (w[k] & ~keep);
                }
            }
        }
        *reinterpret_cast<uint32_t*>(ctx + kOffBufferLength) = s.new_len;
        mid_off = off + s.head;
        mid_len = 64u * s.nb;
    }
    U.mid_off[i] = mid_off;
    U.mid_len[i] = mid_len;
#pragma unroll
    for (int k = 0; k < 5; ++k) U.state[5u * i + k] = h[k];
}

__global__ __launch_bounds__(kUpdateThreads) void sha1_update_post_kernel(UpdateArgs U) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U.n) return;
    uint8_t* ctx = entry_context(U, i);
    if (!ctx) return;
    // pre left every entry it worked on at 0..63 staged bytes; one it skipped
    // still says more
    if (skip_staged(*reinterpret_cast<const uint32_t*>(ctx + kOffBufferLength))) return;
    uint32_t* hw = reinterpret_cast<uint32_t*>(ctx + kOffHash);
#pragma unroll
    for (int k = 0; k < 5; ++k) hw[k] = U.state[5u * i + k];
}

__global__ __launch_bounds__(kUpdateThreads) void sha1_update_final_kernel(UpdateArgs U) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U.n) return;
    uint8_t* ctx = entry_context(U, i);
    if (!ctx) return;
    const uint32_t b = *reinterpret_cast<const uint32_t*>(ctx + kOffBufferLength);
    if (skip_staged(b)) return;
    uint64_t* total = reinterpret_cast<uint64_t*>(ctx + kOffTotal);
    const uint64_t bits = *total;
    uint32_t* hw = reinterpret_cast<uint32_t*>(ctx + kOffHash);
    uint32_t h[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = hw[k];
    finish_message(h, ctx + kOffBuffer, b, bits / 8u);
    if (U.dig) store_digest(U.dig + 20ull * i, h);
    // as SHA1Final leaves it (sha.c:529-558): the digest words, nothing
    // staged, the length with the padding's 0x80, zeros and 8 length bytes
#pragma unroll
    for (int k = 0; k < 5; ++k) hw[k] = h[k];
    *reinterpret_cast<uint32_t*>(ctx + kOffBufferLength) = 0u;
    *total = bits + 8ull * ((b < 56u ? 56u - b : 120u - b) + 8u);
}

__global__ __launch_bounds__(kUpdateThreads) void sha1_update_init_kernel(UpdateArgs U) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U.n) return;
    uint8_t* ctx = entry_context(U, i);
    if (!ctx) return;
    *reinterpret_cast<uint64_t*>(ctx + kOffTotal) = 0ull;
    uint32_t* hw = reinterpret_cast<uint32_t*>(ctx + kOffHash);
    hw[0] = IV0;
    hw[1] = IV1;
    hw[2] = IV2;
    hw[3] = IV3;
    hw[4] = IV4;
    *reinterpret_cast<uint32_t*>(ctx + kOffBufferLength) = 0u;
}

template <typename K>
hipError_t launch_update(K kernel, const UpdateArgs& U, hipStream_t st) {
    if (U.n == 0) return hipSuccess;
    const uint32_t grid = (U.n + kUpdateThreads - 1u) / kUpdateThreads;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kUpdateThreads), 0, st, U);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_update_pre(const UpdateArgs& U, hipStream_t st) { return launch_update(sha1_update_pre_kernel, U, st); }
hipError_t launch_update_post(const UpdateArgs& U, hipStream_t st) { return launch_update(sha1_update_post_kernel, U, st); }
hipError_t launch_update_final(const UpdateArgs& U, hipStream_t st) { return launch_update(sha1_update_final_kernel, U, st); }
hipError_t launch_update_init(const UpdateArgs& U, hipStream_t st) { return launch_update(sha1_update_init_kernel, U, st); }
