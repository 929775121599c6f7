// gather_map_check -- host check of the segment gather's address arithmetic
// (congestion-control-with-bittorren_amd/csrc/gather_map.hpp, which
// sha1_gather.hip's copy kernel computes with).  The kernel's per-thread code
// (copy_edge, tile_words, tile_first_segment / tile_end_segment, copy_word) is
// replayed thread by thread on byte images -- a word's segment searched inside
// the tile's range (the kernel's path for long lists) for every other case,
// in the whole list for the rest -- with every load and store checked
// against a byte-by-byte model of the message:
//   - every load is an aligned 4-byte word that holds a byte of one of the
//     message's segments: nothing else is read;
//   - every store lies inside [dst, dst + total); a 16-byte store is aligned;
//     every message byte is stored exactly once, with the model's value, and
//     the 0xA5 guards around the destination stay intact;
//   - head + 16 * words + tail == total, and the words start on a 16-byte line.
// Enumerated, each with source start mod 16 x destination start mod 16 (every
// segment of a message starts at its own alignment, derived from the first's):
//   1 and 2 segments   every length 0..70 per segment, all 256 alignment pairs;
//   3 segments         every length triple of 0..70, the alignment pair rotating
//                      through all 256 from one triple to the next, and the full
//                      product of 12 lengths with all 256 pairs;
//   4 segments         the full product of 8 lengths with all 256 pairs, and
//                      every length quadruple of 0..70 step 3 with a rotating
//                      pair;
//   long               messages of several 4 KiB tiles (segments longer and
//                      shorter than a tile, 1-7 byte runs), all 256 pairs.
// (The full product of four lengths 0..70 with 256 pairs is 6.5e9 messages.)
// The skip rules' boundaries are checked too.  Exits 0 when all hold, 1 with
// the first violation otherwise.
//   usage: gather_map_check   (no arguments; `make tools` builds it)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../congestion-control-with-bittorren_amd/csrc/gather_map.hpp"

using namespace s1ga;

namespace {

constexpr uint32_t kMaxSegs = 4096;
constexpr uint64_t kSrcBytes = 1u << 18;
constexpr uint64_t kDstGuard = 64;

struct Case {
    uint32_t k = 0;
    uint64_t off[kMaxSegs];
    uint32_t len[kMaxSegs], pos[kMaxSegs];
    uint32_t sa = 0, da = 0;
};

[[noreturn]] void bad(const char* what, const Case& c, uint64_t x) {
    fprintf(stderr, "gather_map_check: %s (%u segments, lengths", what, c.k);
    for (uint32_t r = 0; r < c.k && r < 8; ++r) fprintf(stderr, " %u", c.len[r]);
    fprintf(stderr, ", source start %u, destination start %u: %llu)\n", c.sa, c.da, static_cast<unsigned long long>(x));
    exit(1);
}

// The images: loads come from src, stores go to dst; both are checked.
struct Image {
    const Case* c;
    std::vector<uint8_t> src, dst;
    std::vector<uint8_t> hits;     // stores per destination byte
    std::vector<uint8_t> allowed;  // per aligned source word: holds a byte of a segment of the case
    uint64_t at = 0, total = 0;  // the message's destination
    uint64_t loads = 0, stores = 0;

    uint32_t load32(uint64_t a) {
        if (a & 3u) bad("unaligned word read", *c, a);
        if (a + 4u > src.size() || !allowed[a >> 2]) bad("read of a word that holds no segment byte", *c, a);
        ++loads;
        uint32_t v;
        memcpy(&v, &src[a], 4);
        return v;
    }
    void put(uint64_t a, uint8_t v) {
        if (a < at || a >= at + total) bad("store outside the message", *c, a);
        if (hits[a]++) bad("destination byte stored twice", *c, a);
        dst[a] = v;
    }
    void store8(uint64_t a, uint32_t v) {
        ++stores;
        put(a, static_cast<uint8_t>(v));
    }
    void store128(uint64_t a, const uint32_t (&w)[4]) {
        if (a & 15u) bad("unaligned 16-byte store", *c, a);
        ++stores;
        for (uint32_t b = 0; b < 16; ++b) put(a + b, static_cast<uint8_t>(w[b >> 2] >> (8u * (b & 3u))));
    }
};

uint64_t g_cases = 0;

// Lay the case's segments out in the source image (each at its own alignment,
// a gap between them), replay the kernel and compare with the model.
void run_case(Image& im, Case& c) {
    ++g_cases;
    uint64_t cur = 64, total = 0;
    for (uint32_t r = 0; r < c.k; ++r) {
        cur = (cur + 15u) / 16u * 16u + ((c.sa + 5u * r) & 15u);
        c.off[r] = cur;
        c.pos[r] = static_cast<uint32_t>(total);
        total += c.len[r];
        cur += c.len[r] + 24u;
    }
    if (cur + 8 > im.src.size()) bad("case larger than the source image", c, cur);
    for (uint32_t r = 0; r < c.k; ++r)
        for (uint64_t w = c.off[r] >> 2; c.len[r] && w <= (c.off[r] + c.len[r] - 1u) >> 2; ++w) im.allowed[w] = 1;
    const uint64_t at = kDstGuard + c.da, span = at + total + kDstGuard;
    if (im.dst.size() < span) {
        im.dst.resize(span);
        im.hits.resize(span);
    }
    memset(im.dst.data(), 0xA5, span);
    memset(im.hits.data(), 0, span);
    im.c = &c;
    im.at = at;
    im.total = total;

    if (total) {  // the kernel leaves an empty message alone
        Msg M;
        M.base = 0;
        M.off = c.off;
        M.len = c.len;
        M.pos = c.pos;
        M.first = 0;
        M.end = c.k;
        M.total = static_cast<uint32_t>(total);
        M.dst = at;
        const Plan P = store_plan(M.dst, M.total);
        if (P.head + 16ull * P.words + P.tail != total) bad("head + words + tail is not the length", c, P.words);
        if (P.head > 15u || P.tail > 15u) bad("more than 15 edge bytes", c, P.head);
        if (P.words && ((at + P.head) & 15u)) bad("whole words off the 16-byte line", c, P.head);
        for (uint32_t e = 0; e < 32; ++e) copy_edge(im, M, P, e);
        Tile T;
        for (uint32_t t = 0; tile_words(P, t, T); ++t) {
            uint32_t lo = tile_first_segment(M, P, T), hi = tile_end_segment(M, P, T);
            if (lo >= hi || hi > c.k) bad("tile segment bounds", c, lo);
            if (g_cases & 1u) lo = M.first, hi = M.end;  // the kernel's other path: every thread searches the whole list
            for (uint32_t tid = 0; tid < kTileWords; ++tid)
                if (T.w0 + tid < T.w1) copy_word(im, M, P, T.w0 + tid, lo, hi);
        }
    }
    // the byte-by-byte model
    uint64_t j = 0;
    for (uint32_t r = 0; r < c.k; ++r)
        for (uint32_t b = 0; b < c.len[r]; ++b, ++j) {
            if (im.hits[at + j] != 1) bad("message byte not stored", c, j);
            if (im.dst[at + j] != im.src[c.off[r] + b]) bad("wrong byte", c, j);
        }
    for (uint64_t a = 0; a < at; ++a)
        if (im.dst[a] != 0xA5) bad("guard before the message changed", c, a);
    for (uint64_t a = at + total; a < span; ++a)
        if (im.dst[a] != 0xA5) bad("guard after the message changed", c, a);
    for (uint32_t r = 0; r < c.k; ++r)
        for (uint64_t w = c.off[r] >> 2; c.len[r] && w <= (c.off[r] + c.len[r] - 1u) >> 2; ++w) im.allowed[w] = 0;
}

void all_pairs(Image& im, Case& c) {
    for (c.sa = 0; c.sa < 16; ++c.sa)
        for (c.da = 0; c.da < 16; ++c.da) run_case(im, c);
}

void rotating_pair(Image& im, Case& c, uint32_t& turn) {
    c.sa = turn & 15u;
    c.da = (turn >> 4) & 15u;
    ++turn;
    run_case(im, c);
}

void check_skip_rules() {
    Case none;
    if (skip_range(0, 0, 0) || skip_range(3, 3, 3) || skip_range(2, 5, 5)) bad("a valid segment range is skipped", none, 0);
    if (!skip_range(4, 3, 9) || !skip_range(0, 10, 9) || !skip_range(0xffffffffull, 0, 9))
        bad("an invalid segment range is kept", none, 0);
    if (skip_total(0, 0, 0) || skip_total(kMaxMessage, 5, kMaxMessage + 5) || skip_total(7, 1, 8))
        bad("a message that fits is skipped", none, 0);
    if (!skip_total(kMaxMessage + 1, 0, ~0ull) || !skip_total(8, 1, 8) || !skip_total(0, 9, 8) ||
        !skip_total(2, ~0ull, ~0ull))
        bad("a message that does not fit is kept", none, 0);
}

}  // namespace

int main() {
    check_skip_rules();
    static Case c;
    Image im;
    im.src.resize(kSrcBytes);
    im.allowed.assign(kSrcBytes / 4, 0);
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (auto& b : im.src) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = static_cast<uint8_t>(x >> 56);
    }
    // 1 and 2 segments: every length, every pair
    c.k = 1;
    for (c.len[0] = 0; c.len[0] <= 70; ++c.len[0]) all_pairs(im, c);
    c.k = 2;
    for (c.len[0] = 0; c.len[0] <= 70; ++c.len[0])
        for (c.len[1] = 0; c.len[1] <= 70; ++c.len[1]) all_pairs(im, c);
    // 3 segments
    uint32_t turn = 0;
    c.k = 3;
    for (c.len[0] = 0; c.len[0] <= 70; ++c.len[0])
        for (c.len[1] = 0; c.len[1] <= 70; ++c.len[1])
            for (c.len[2] = 0; c.len[2] <= 70; ++c.len[2]) rotating_pair(im, c, turn);
    const uint32_t some3[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 33, 64, 70};
    for (uint32_t a : some3)
        for (uint32_t b : some3)
            for (uint32_t d : some3) {
                c.len[0] = a, c.len[1] = b, c.len[2] = d;
                all_pairs(im, c);
            }
    // 4 segments
    c.k = 4;
    const uint32_t some4[] = {0, 1, 2, 3, 5, 16, 17, 70};
    for (uint32_t a : some4)
        for (uint32_t b : some4)
            for (uint32_t d : some4)
                for (uint32_t e : some4) {
                    c.len[0] = a, c.len[1] = b, c.len[2] = d, c.len[3] = e;
                    all_pairs(im, c);
                }
    for (c.len[0] = 0; c.len[0] <= 70; c.len[0] += 3)
        for (c.len[1] = 0; c.len[1] <= 70; c.len[1] += 3)
            for (c.len[2] = 0; c.len[2] <= 70; c.len[2] += 3)
                for (c.len[3] = 0; c.len[3] <= 70; c.len[3] += 3) rotating_pair(im, c, turn);
    // several tiles
    c.k = 3;
    c.len[0] = 5000, c.len[1] = 3, c.len[2] = 4099;
    all_pairs(im, c);
    c.len[0] = 1, c.len[1] = 9000, c.len[2] = 0;
    all_pairs(im, c);
    c.k = 12;  // the packet shape, shortened: eleven 1484-byte packets and the 436-byte last one
    for (uint32_t r = 0; r < c.k; ++r) c.len[r] = r + 1 < c.k ? 1484 : 436;
    all_pairs(im, c);
    c.k = 2500;  // runs of 1-7 bytes across three tiles
    for (uint32_t r = 0; r < c.k; ++r) c.len[r] = 1 + (r * 5u + r / 7u) % 7u;
    all_pairs(im, c);
    printf("gather_map_check: %llu messages, %llu loads, %llu stores: ok\n", static_cast<unsigned long long>(g_cases),
           static_cast<unsigned long long>(im.loads), static_cast<unsigned long long>(im.stores));
    return 0;
}
