// gather_map.hpp -- the arithmetic of the segment gather (sha1_gather.hip),
// compiled for host and device so that tools/gather_map_check.cc can replay
// the copy kernel's loads and stores on the CPU.
//
// A message is the concatenation, in order, of segments first .. end-1 of a
// segment list: segment s is len[s] bytes at base + off[s], and pos[s] (the
// scan kernel's output) is the exclusive prefix of the lengths inside the
// message, so message byte j comes from the last segment s with pos[s] <= j
// (a zero-length segment shares its position with its successor and never
// holds a byte), at source byte off[s] + (j - pos[s]).
//
// The destination of a message of `total` bytes at address dst is cut into
//   head   the bytes before the first 16-byte boundary (or all of a message
//          that ends before it),
//   words  whole aligned 16-byte words, each one vector store,
//   tail   the bytes after the last whole word,
// so that no byte outside [dst, dst + total) is written.  Head and tail are
// byte stores.  Every source byte is read through the aligned 4-byte word
// that holds it and funnelled into place (alignbyte); a word is loaded only
// when it holds a byte of the segment being read, across a seam inside one
// store too.
//
// Everything here is bounded by the segment list itself: whatever pos[] holds
// (two messages whose segment index ranges overlap race on it, which the
// interface declares undefined), a load stays inside the words of a segment
// of the message and a store inside the message's destination.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define S1GA_HD __host__ __device__
#else
#define S1GA_HD
#endif

namespace s1ga {

constexpr uint32_t kSkipped = 0xffffffffu;      // length word of a skipped message
constexpr uint64_t kMaxMessage = 0xfffffffeull;  // 2^32 - 2 bytes
constexpr uint32_t kTileWords = 256;             // 16-byte words of one tile: one per thread, 4 KiB

// The skip rules of a message (the device form skips; the host forms refuse).
S1GA_HD inline bool skip_range(uint64_t first, uint64_t end, uint64_t n_segments) {
    return first > end || end > n_segments;
}
S1GA_HD inline bool skip_total(uint64_t total, uint64_t dst_off, uint64_t dst_bytes) {
    return total > kMaxMessage || dst_off > dst_bytes || total > dst_bytes - dst_off;
}

// (hi:lo) >> 8 * sh, the low word: v_alignbyte_b32 on the device.
S1GA_HD inline uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (8u * (sh & 3u)));
#endif
}

struct Msg {
    uint64_t base;        // address of the source base
    const uint64_t* off;  // per segment: byte offset from base
    const uint32_t* len;  // per segment: bytes
    const uint32_t* pos;  // per segment: position inside its message
    uint32_t first, end;  // the message's segments, first < end
    uint32_t total;       // its length, > 0
    uint64_t dst;         // address of its first destination byte
};

struct Plan {
    uint32_t head, words, tail;
};
S1GA_HD inline Plan store_plan(uint64_t dst, uint32_t total) {
    Plan p;
    const uint32_t to_line = static_cast<uint32_t>((16u - (dst & 15u)) & 15u);
    p.head = total < to_line ? total : to_line;
    p.words = (total - p.head) >> 4;
    p.tail = (total - p.head) & 15u;
    return p;
}

// The last segment of [lo, hi) whose position is <= j; lo when there is none
// (or when hi <= lo: bounds taken from a racing pos[], see above).
S1GA_HD inline uint32_t find_segment(const Msg& M, uint32_t lo, uint32_t hi, uint32_t j) {
    while (hi > lo && hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (M.pos[mid] <= j)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Message bytes [j, j + want) (want 1..4, inside the message) as the low
// bytes of a little-endian word.  s: a segment at or before the one that
// holds byte j; left at the one that holds the last byte taken.
template <class Mem>
S1GA_HD inline uint32_t gather_dword(Mem& m, const Msg& M, uint32_t j, uint32_t want, uint32_t& s) {
    uint32_t out = 0, filled = 0;
    while (filled < want && s < M.end) {
        const uint32_t in = j + filled - M.pos[s], L = M.len[s];
        if (in >= L) {
            ++s;
            continue;
        }
        const uint32_t take = want - filled < L - in ? want - filled : L - in;
        const uint64_t a = M.base + M.off[s] + in;
        const uint32_t sh = static_cast<uint32_t>(a & 3u);
        const uint64_t q = a & ~uint64_t(3);
        const uint32_t lo = m.load32(q);
        const uint32_t hi = sh + take > 4u ? m.load32(q + 4) : 0u;
        uint32_t v = funnel(hi, lo, sh);
        if (take < 4u) v &= (1u << (8u * take)) - 1u;
        out |= v << (8u * filled);
        filled += take;
    }
    return out;
}

// Message bytes [j, j + 16) as four words.  s: as above.  Inside one segment:
// four or five aligned words, funnelled; across a seam: word by word.
template <class Mem>
S1GA_HD inline void gather_word16(Mem& m, const Msg& M, uint32_t j, uint32_t s, uint32_t (&w)[4]) {
    const uint32_t in = j - M.pos[s], L = M.len[s];
    if (in < L && L - in >= 16u) {
        const uint64_t a = M.base + M.off[s] + in;
        const uint32_t sh = static_cast<uint32_t>(a & 3u);
        const uint64_t q = a & ~uint64_t(3);
        uint32_t d[5];
        for (int k = 0; k < 4; ++k) d[k] = m.load32(q + 4u * k);
        d[4] = sh ? m.load32(q + 16) : 0u;
        for (int k = 0; k < 4; ++k) w[k] = funnel(d[k + 1], d[k], sh);
    } else {
        for (uint32_t k = 0; k < 4; ++k) w[k] = gather_dword(m, M, j + 4u * k, 4u, s);
    }
}

// Tile t of the message's whole words: words [w0, w1) and the segments
// [s_lo, s_hi) their first bytes lie in.  False when the tile is empty.
struct Tile {
    uint32_t w0, w1;
};
S1GA_HD inline bool tile_words(const Plan& P, uint32_t t, Tile& T) {
    const uint64_t w0 = static_cast<uint64_t>(t) * kTileWords;
    if (w0 >= P.words) return false;
    T.w0 = static_cast<uint32_t>(w0);
    T.w1 = P.words - T.w0 < kTileWords ? P.words : T.w0 + kTileWords;
    return true;
}
S1GA_HD inline uint32_t word_byte(const Plan& P, uint32_t word) { return P.head + 16u * word; }
S1GA_HD inline uint32_t tile_first_segment(const Msg& M, const Plan& P, const Tile& T) {
    return find_segment(M, M.first, M.end, word_byte(P, T.w0));
}
S1GA_HD inline uint32_t tile_end_segment(const Msg& M, const Plan& P, const Tile& T) {
    return find_segment(M, M.first, M.end, word_byte(P, T.w1 - 1u)) + 1u;
}

// One thread's whole word of a tile: the vector store.
template <class Mem>
S1GA_HD inline void copy_word(Mem& m, const Msg& M, const Plan& P, uint32_t word, uint32_t s_lo, uint32_t s_hi) {
    const uint32_t j = word_byte(P, word);
    uint32_t w[4];
    gather_word16(m, M, j, find_segment(M, s_lo, s_hi, j), w);
    m.store128(M.dst + j, w);
}

// Edge byte e of a message (0..15 the head, 16..31 the tail): a byte store,
// or nothing when the message has no such byte.
template <class Mem>
S1GA_HD inline void copy_edge(Mem& m, const Msg& M, const Plan& P, uint32_t e) {
    uint32_t j;
    if (e < 16u) {
        if (e >= P.head) return;
        j = e;
    } else {
        if (e - 16u >= P.tail) return;
        j = P.head + 16u * P.words + (e - 16u);
    }
    uint32_t s = find_segment(M, M.first, M.end, j);
    m.store8(M.dst + j, gather_dword(m, M, j, 1u, s) & 0xffu);
}

}  // namespace s1ga
