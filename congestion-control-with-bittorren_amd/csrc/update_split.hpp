// update_split.hpp -- the arithmetic of one batched SHA1Update entry
// (sha1_update.hip's pre kernel), compiled for host and device so that
// tools/update_split_check.cc can check it on the CPU.
//
// A context is the reference's SHA1Context (include/sha.h): 96 bytes,
// totalLength (bits) at 0, hash[5] at 8, bufferLength at 28, buffer at 32.
// An entry feeds a piece of L bytes to a context that holds b staged bytes:
//   - b + L < 64: the piece is appended at buffer[b ..); nothing to compress;
//   - else, with b > 0 the first head = 64 - b piece bytes complete the staged
//     block (compressed by the pre kernel), nb whole blocks follow (the bulk
//     launch), and the last rem bytes are staged at buffer[0 .. rem).
// Either way one copy of `copy_len` piece bytes from piece offset `copy_src`
// to buffer offset `copy_dst` re-stages the context, and the new
// bufferLength is copy_dst + copy_len = (b + L) % 64.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define S1UP_HD __host__ __device__
#else
#define S1UP_HD
#endif

namespace s1up {

constexpr uint32_t kContextBytes = 96;
constexpr uint32_t kOffTotal = 0, kOffHash = 8, kOffBufferLength = 28, kOffBuffer = 32;

// An entry the device kernels leave alone (no read or write through it): its
// context index is outside the array, or its context claims more staged
// bytes than the buffer's 63 (the reference would overrun its buffer).
S1UP_HD inline bool skip_index(uint64_t context, uint64_t n_contexts) { return context >= n_contexts; }
S1UP_HD inline bool skip_staged(uint32_t b) { return b > 63u; }

struct Split {
    uint32_t fits;      // 1: b + L < 64, the piece only extends the staged bytes
    uint32_t head;      // piece bytes that complete the staged block (0 when b == 0 or fits)
    uint32_t nb;        // whole 64-byte blocks after the head: the bulk launch's
    uint32_t copy_src;  // piece offset of the bytes to stage
    uint32_t copy_dst;  // buffer offset they go to (b when fits, else 0)
    uint32_t copy_len;  // how many (rem, or L when fits)
    uint32_t new_len;   // bufferLength afterwards
};

// b <= 63 (skip_staged is checked first); L is any 32-bit length.
S1UP_HD inline Split split_piece(uint32_t b, uint32_t L) {
    Split s;
    if (static_cast<uint64_t>(b) + L < 64u) {
        s.fits = 1u;
        s.head = 0u;
        s.nb = 0u;
        s.copy_src = 0u;
        s.copy_dst = b;
        s.copy_len = L;
    } else {
        s.fits = 0u;
        s.head = b ? 64u - b : 0u;
        s.nb = (L - s.head) >> 6;
        s.copy_len = (L - s.head) & 63u;
        s.copy_src = s.head + 64u * s.nb;  // = L - rem: no overflow
        s.copy_dst = 0u;
    }
    s.new_len = s.copy_dst + s.copy_len;
    return s;
}

// Word k (bytes 4k .. 4k+3) of a 64-byte window whose bytes [lo, hi) come from
// a source: does the word hold any of them (so it is loaded / stored), and
// which of its little-endian bytes lie below lo (kept from what was there).
S1UP_HD inline bool word_touched(uint32_t k, uint32_t lo, uint32_t hi) { return 4u * k + 4u > lo && 4u * k < hi; }
S1UP_HD inline uint32_t keep_mask(uint32_t k, uint32_t lo) {
    const uint32_t below = lo > 4u * k ? lo - 4u * k : 0u;  // bytes of word k before lo
    return below >= 4u ? 0xffffffffu : (1u << (8u * below)) - 1u;
}

// The window's source bytes are loaded as aligned 4-byte words: with window
// byte 0 at address a, sh = a & 3, aligned word j (j = 0..16, from a & ~3)
// holds window bytes [4j - sh, 4j - sh + 4).  It is loaded only when it holds
// a byte of [lo, hi): no word without a byte of the piece is ever read.
S1UP_HD inline bool window_word_loaded(uint32_t j, uint32_t lo, uint32_t hi, uint32_t sh) {
    return 4u * j + 4u > lo + sh && 4u * j < hi + sh;
}

}  // namespace s1up
