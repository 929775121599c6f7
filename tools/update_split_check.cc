// update_split_check -- host check of the batched SHA1Update's split
// arithmetic (congestion-control-with-bittorren_amd/csrc/update_split.hpp,
// which sha1_update.hip's pre kernel computes with).  For every staged count
// b in 0..63, every piece length L in 0..400 and every piece start mod 4 the
// pre kernel's loads and stores are replayed word by word on a byte image:
//   - head + 64 nb + rem == L, or the piece fits in the buffer (b + L < 64);
//   - the new bufferLength is (b + L) % 64;
//   - every buffer store stays in [0, 64), and stores only words that hold a
//     byte of the copy;
//   - every aligned word read from the piece holds a byte of [0, L): no read
//     of a word outside the piece;
//   - the head block is buffer[0 .. b) then piece[0 .. 64 - b), and the first
//     bufferLength bytes of the new buffer are what SHA1Update stages.
// b = 64 and b = 2^32 - 1 are skipped, an index at or above n_contexts too.
// Exits 0 when all hold, 1 with the first violation otherwise.
//   usage: update_split_check   (no arguments; `make tools` builds it)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../congestion-control-with-bittorren_amd/csrc/update_split.hpp"

namespace {

[[noreturn]] void bad(const char* what, uint32_t b, uint32_t L, uint32_t a, uint32_t x) {
    fprintf(stderr, "update_split_check: %s (b %u, L %u, start %u: %u)\n", what, b, L, a, x);
    exit(1);
}

// The piece in a byte image: bytes [at, at + L) of mem; reads are counted and
// checked against the piece.
struct Image {
    std::vector<uint8_t> mem;
    uint32_t at, L, b, start;
    uint64_t words = 0;
    uint32_t read_word(uint32_t addr) {
        if (addr & 3u) bad("unaligned word read", b, L, start, addr);
        if (!(addr + 4u > at && addr < at + L)) bad("read of a word that holds no piece byte", b, L, start, addr);
        ++words;
        uint32_t v;
        memcpy(&v, &mem[addr], 4);
        return v;
    }
};

// sha1_update.hip load_window, on the image: src is an image address.
void load_window(Image& im, uint32_t src, uint32_t lo, uint32_t hi, uint32_t (&w)[16]) {
    const uint32_t a = src - lo, sh = a & 3u, q = a & ~3u;
    uint32_t d[17];
    for (uint32_t j = 0; j < 17; ++j) d[j] = s1up::window_word_loaded(j, lo, hi, sh) ? im.read_word(q + 4u * j) : 0u;
    for (uint32_t j = 0; j < 16; ++j)
        w[j] = static_cast<uint32_t>(((static_cast<uint64_t>(d[j + 1]) << 32) | d[j]) >> (8u * sh));
}

uint64_t check_case(uint32_t b, uint32_t L, uint32_t start) {
    const s1up::Split s = s1up::split_piece(b, L);
    if (s.fits) {
        if (b + L >= 64u || s.head || s.nb || s.copy_src || s.copy_dst != b || s.copy_len != L)
            bad("fits-in-buffer case wrong", b, L, start, s.copy_len);
    } else {
        if (b + L < 64u) bad("a piece that fits was split", b, L, start, 0);
        if (s.head != (b ? 64u - b : 0u)) bad("head", b, L, start, s.head);
        if (s.head + 64u * s.nb + s.copy_len != L) bad("head + 64 nb + rem != L", b, L, start, s.copy_len);
        if (s.copy_len > 63u || s.copy_dst != 0u || s.copy_src != s.head + 64u * s.nb)
            bad("residue", b, L, start, s.copy_src);
    }
    if (s.new_len != (b + L) % 64u) bad("new bufferLength", b, L, start, s.new_len);
    if (s.copy_dst + s.copy_len > 63u) bad("copy leaves the buffer", b, L, start, s.copy_dst + s.copy_len);
    if (static_cast<uint64_t>(s.copy_src) + s.copy_len > L) bad("copy reads past the piece", b, L, start, s.copy_src);

    // replay on bytes: a staged buffer, a piece with other bytes around it
    Image im;
    im.at = 128u + start;
    im.L = L;
    im.b = b;
    im.start = start;
    im.mem.assign(128u + 8u + L + 128u, 0xEE);
    for (uint32_t i = 0; i < L; ++i) im.mem[im.at + i] = static_cast<uint8_t>(1u + (i * 7u + b) % 251u);
    uint8_t buffer[64];
    for (uint32_t i = 0; i < 64; ++i) buffer[i] = static_cast<uint8_t>(i < b ? 0x80u + i : 0x55u);  // stale above b
    std::vector<uint8_t> stream(buffer, buffer + b);  // what SHA1Update sees
    stream.insert(stream.end(), im.mem.begin() + im.at, im.mem.begin() + im.at + L);

    uint32_t staged[16];
    memcpy(staged, buffer, 64);
    if (s.head) {
        uint32_t w[16];
        load_window(im, im.at, b, 64u, w);
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t keep = s1up::keep_mask(k, b);
            w[k] = (staged[k] & keep) | (w[k] & ~keep);
        }
        if (memcmp(w, stream.data(), 64)) bad("head block is not buffer then piece", b, L, start, s.head);
    }
    if (s.copy_len) {
        const uint32_t lo = s.copy_dst, hi = s.copy_dst + s.copy_len;
        uint32_t w[16];
        load_window(im, im.at + s.copy_src, lo, hi, w);
        for (uint32_t k = 0; k < 16; ++k) {
            if (!s1up::word_touched(k, lo, hi)) continue;
            if (4u * k + 4u > 64u) bad("buffer store outside [0, 64)", b, L, start, k);
            const uint32_t keep = s1up::keep_mask(k, lo);
            const uint32_t v = (staged[k] & keep) | (w[k] & ~keep);
            memcpy(buffer + 4u * k, &v, 4);
        }
    }
    // the words of every store hold a byte of the copy; the others are intact
    for (uint32_t i = 0; i < 64; ++i) {
        const bool in_touched = s.copy_len && s1up::word_touched(i / 4u, s.copy_dst, s.copy_dst + s.copy_len);
        if (!in_touched && buffer[i] != static_cast<uint8_t>(i < b ? 0x80u + i : 0x55u))
            bad("a buffer byte outside the stored words changed", b, L, start, i);
    }
    const uint32_t done = static_cast<uint32_t>(stream.size()) - s.new_len;  // bytes in whole blocks
    if (done % 64u) bad("compressed bytes are not whole blocks", b, L, start, done);
    if (s.new_len && memcmp(buffer, stream.data() + done, s.new_len)) bad("staged bytes differ from SHA1Update's", b, L, start, s.new_len);
    if (done / 64u != s.nb + (s.head ? 1u : 0u)) bad("block count", b, L, start, s.nb);
    return im.words;
}

}  // namespace

int main() {
    uint64_t cases = 0, words = 0;
    for (uint32_t b = 0; b < 64; ++b)
        for (uint32_t L = 0; L <= 400; ++L)
            for (uint32_t start = 0; start < 4; ++start) {
                words += check_case(b, L, start);
                ++cases;
            }
    // lengths up to 2^32 - 1: the arithmetic alone
    static const uint32_t kLong[] = {0xffffffffu, 0xffffffc0u, 0xffffffbfu, 0x80000000u, 0x7fffffffu, 1u << 20};
    for (uint32_t b = 0; b < 64; ++b)
        for (uint32_t L : kLong) {
            const s1up::Split s = s1up::split_piece(b, L);
            if (s.fits || static_cast<uint64_t>(s.head) + 64ull * s.nb + s.copy_len != L ||
                s.new_len != static_cast<uint32_t>((static_cast<uint64_t>(b) + L) % 64u) ||
                static_cast<uint64_t>(s.copy_src) + s.copy_len != L)
                bad("long piece", b, L, 0, s.nb);
            ++cases;
        }
    if (!s1up::skip_staged(64u) || !s1up::skip_staged(0xffffffffu) || s1up::skip_staged(63u) || s1up::skip_staged(0u))
        bad("skip on bufferLength", 64, 0, 0, 0);
    if (!s1up::skip_index(5, 5) || !s1up::skip_index(0xffffffffull, 5) || !s1up::skip_index(0, 0) || s1up::skip_index(4, 5))
        bad("skip on index", 0, 0, 0, 0);
    printf("update_split_check: ok (%llu cases, %llu piece words read)\n", (unsigned long long)cases,
           (unsigned long long)words);
    return 0;
}
