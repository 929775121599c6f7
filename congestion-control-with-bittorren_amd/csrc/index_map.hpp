// index_map.hpp -- the arithmetic of the digest index (sha1_index.hip),
// compiled for host and device so that tools/index_map_check.cc can run the
// build and the lookup on the CPU.
//
// The index over a table of m digests (digest p = words table[5p .. 5p+4], its
// position p) is an open-addressed array of `slots` position words, kEmpty
// where nothing lives:
//   slots   the smallest power of two >= 2 m, at least 8: the array is at most
//           half full, so every probe sequence reaches an empty slot;
//   home    a fixed integer mix of a digest's FIRST TWO words, masked to the
//           array.  SHA-1 output is uniform already; the mix only keeps a table
//           of strings that are no hashes from being pathological by accident.
//           Digests that share their first 8 bytes share a home: deliberate,
//           it gives the tests a chain of known length;
//   probe   linear, (h + 1) & (slots - 1);
//   no tag  a slot holds a position and nothing else: every occupied probe
//           compares all five words against table[slot].
//
// insert() and lookup() are written over a slot accessor, so the kernels
// (agent-scope atomics in the build, plain loads in the lookup) and the host
// check (plain memory, one entry after the other) run the same statements.
// insert: claim the slot if it is empty; if it holds the entry's own digest,
// lower it to the smaller position and stop -- duplicates collapse into one
// slot that ends holding the lowest position; else step.  An occupant read
// once may have been lowered since, but only to another position of the same
// digest, so the comparison's answer stands and racing lanes build the same
// array, whatever their order.
//
// The set grows after the build (include/sha1chunk.h, "Digest index"): the
// table has room for `capacity` digests, the array slots_for(capacity) slots,
// and appended entries are inserted by the same insert().  An appended entry
// may be skipped: its row is written, it is never inserted, and as nothing
// but a slot leads to a row, no lookup answers it.  A larger array is filled
// from a smaller one by rehash_slot(): the old slots hold exactly the admitted
// distinct digests at their lowest positions, so inserting what they hold
// rebuilds the set without a record of which rows were skipped.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define S1IX_HD __host__ __device__
#else
#define S1IX_HD
#endif

namespace s1ix {

constexpr uint32_t kEmpty = 0xffffffffu;        // an empty slot; SHA1CHUNK_NO_MATCH as an answer
constexpr uint64_t kMaxEntries = 1ull << 31;    // positions stay below kEmpty, slots within 2^32
constexpr uint64_t kMaxQueries = 0xffffffffull - 255u;  // one lane per query, whole workgroups of 256
constexpr int kWords = 5;                       // 32-bit words of a digest

S1IX_HD inline uint64_t slots_for(uint64_t m) {
    uint64_t s = 8;
    while (s < 2 * m) s <<= 1;
    return s;
}

// The finaliser of MurmurHash3 over the digest's first two words.
S1IX_HD inline uint32_t home(uint32_t w0, uint32_t w1, uint32_t mask) {
    uint64_t x = (static_cast<uint64_t>(w1) << 32) | w0;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return static_cast<uint32_t>(x) & mask;
}

S1IX_HD inline uint32_t next_slot(uint32_t h, uint32_t mask) { return (h + 1u) & mask; }

S1IX_HD inline bool same_digest(const uint32_t* a, const uint32_t* b) {
    uint32_t diff = 0;
    for (int k = 0; k < kWords; ++k) diff |= a[k] ^ b[k];
    return diff == 0;
}

// What one entry's insertion did (s1be_index_stats adds these up).
struct Probe {
    uint32_t visited;  // slots visited, 1 = the home slot was free
    bool duplicate;    // its digest was in place already
    bool wrapped;      // the probe stepped from the last slot to slot 0
};

// Slots: uint32_t claim(h, p) -- if slot h is empty it becomes p; returns what
//                                 the slot held before (kEmpty: claimed);
//        void lower(h, p)     -- slot h = min(slot h, p).
template <class Slots>
S1IX_HD inline Probe insert(const Slots& slots, uint32_t mask, const uint32_t* table, uint32_t p) {
    const uint32_t* mine = table + static_cast<uint64_t>(kWords) * p;
    Probe r{1u, false, false};
    for (uint32_t h = home(mine[0], mine[1], mask);; ++r.visited) {
        const uint32_t held = slots.claim(h, p);
        if (held == kEmpty) return r;
        if (same_digest(table + static_cast<uint64_t>(kWords) * held, mine)) {
            slots.lower(h, p);
            r.duplicate = true;
            return r;
        }
        h = next_slot(h, mask);
        if (h == 0u) r.wrapped = true;
    }
}

// The lowest position whose digest equals q[0..4], or kEmpty.  Slots:
// uint32_t load(h).  Only after every insert is over.
template <class Slots>
S1IX_HD inline uint32_t lookup(const Slots& slots, uint32_t mask, const uint32_t* table, const uint32_t* q) {
    const uint32_t w[kWords] = {q[0], q[1], q[2], q[3], q[4]};
    for (uint32_t h = home(w[0], w[1], mask);; h = next_slot(h, mask)) {
        const uint32_t held = slots.load(h);
        if (held == kEmpty || same_digest(table + static_cast<uint64_t>(kWords) * held, w)) return held;
    }
}

// Growth: what slot s of the old array holds, inserted into the new array over
// the same table rows.  Old: uint32_t load(s); New: claim and lower.
template <class Old, class New>
S1IX_HD inline void rehash_slot(const Old& old_slots, uint32_t s, const New& new_slots, uint32_t new_mask,
                                const uint32_t* table) {
    const uint32_t p = old_slots.load(s);
    if (p != kEmpty) (void)insert(new_slots, new_mask, table, p);
}

// The sequential slot array of the host check.
struct PlainSlots {
    uint32_t* s;
    uint32_t claim(uint32_t h, uint32_t p) const {
        const uint32_t held = s[h];
        if (held == kEmpty) s[h] = p;
        return held;
    }
    void lower(uint32_t h, uint32_t p) const {
        if (p < s[h]) s[h] = p;
    }
    uint32_t load(uint32_t h) const { return s[h]; }
};

}  // namespace s1ix
