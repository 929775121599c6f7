// sha1_split.hpp -- the split and quad-split kernels of the gfx950 SHA-1
// engine (consumer + producer waves over an LDS W+K ring) as templates over
// their shape.  Included by sha1_kernels.hip (the product's kernels and
// launchers) and by tools/ab_kernels.hip (the other split shapes of the
// study, built only into the A/B library).  Everything here is a template or
// internal to the including file.
#ifndef SHA1_SPLIT_HPP
#define SHA1_SPLIT_HPP

#include "sha1_lane.hpp"

// --------------------------------------------------------------- split ----
// Workgroup = consumer wave (wave 0) + producer wave (wave 1) on the same 64
// chunks.  The producer streams the wave's blocks from HBM (two blocks or
// stages in flight in registers; in the product shapes with loads shared
// across the wave, kVCoop), byte-swaps them and
// expands the 80-word schedule into an LDS ring; the consumer runs only the
// 80 rounds, so each chunk's serial instruction stream (the bound when
// there are too few chunks to fill the SIMDs) drops from ~630 to ~440
// instructions per block.
//
// The ring has 2 slots of U blocks (U*20 KiB each).  W slot layout: group q
// (q = 0..19) of four schedule words of block j of lane r at
// j*20K + q*1K + r*16, so every ds_write_b128 / ds_read_b128 touches one
// contiguous KiB (conflict-free).  Protocol, one s_barrier per unit of U
// blocks (each wave executes ceil(Tmax/U)+1 of them):
//   producer: write unit m (blocks mU..mU+U-1) into slot m&1 -> B_m
//   consumer: B_0, read W(0); per block k: [if k+1 starts unit m+1: B_{m+1}]
//             stream W(k+1) into the spare register set, rounds of block k.
//   RAW: unit m+1 is complete before B_{m+1}; its reads come after it.
//   WAR: the producer rewrites slot m&1 (unit m+2) only after B_{m+1}; every
//        read of unit m was issued before B_{m+1} and drained by its lgkmcnt(0).
// Fewer barriers per block (U > 1) is worth ~10% at low occupancy (U = 4,
// the whole 160 KiB LDS, is ~1.5% ahead of U = 3); U = 1 keeps LDS at 40 KiB
// for higher occupancy.
constexpr int kWBlockBytes = 20 * 1024;

// Shape flags: the V parameter of every template below (defaults in
// kSplitV), each with the product units (launch_split, sha1_kernels.hip) and
// A/B units (tools/ab_kernels.hip) that set it.  The values are part of the
// kernels' mangled names (tools/dpp_parity.py looks one up, the study's unit
// numbers 500 + V are built from them) and do not change; the measurements
// behind a flag stand next to the code it selects.
constexpr int kVWK = 1;           // producer ships W+K: product, all; A/B all but 3, 20, 24, 30, 34, 44, 504, 87
constexpr int kVUnmask = 4;       // unmasked commit while every lane is live: product, all; A/B all but 20, 21, 30, 31
constexpr int kVRead10 = 8;       // schedule reads in two bursts of 10, not four of 5: product 4; A/B 12, 16, 17, 92, 99, 577
constexpr int kVSkipWave2 = 64;   // wave 2 empty: product 4, 416; A/B 16, 17, 99, 417, 569, 577, 585, 816, 817
constexpr int kVLayout8 = 128;    // two pairs in 8 waves, a SIMD to each consumer: product 11; A/B 10, 12, 13, 92, 97
constexpr int kVCross = 256;      // kVLayout8 with the pairs' producer SIMDs swapped: product 11; A/B 13, 92, 97
constexpr int kVProbe = 2048;     // waves write barrier-wait and loop cycles over the digests: A/B 97, 99, 417, 817
constexpr int kVCoop = 8192;      // producers share loads: product 4, 11 (ragged), 416; A/B 16, 86, 87, 99, 417, 585, 816, 817
constexpr int kVQuad = 8192 * 4;  // four lanes per chunk (`quad split`): product 416; A/B 417, 816, 817
// (512, 1024, 4096 and 8192 * 2 were round-5 study flags, see below.)

// The shapes by name: U-block units with one producer (U = 1: product 1) or,
// for U = 4, two (product 4); the 8-wave two-pair shape (product 11, the
// mixed kernel's mode 1); the quad shape (product 416).
template <int U>
constexpr int kSplitV = U == 4 ? (kVWK | kVUnmask | kVSkipWave2 | kVRead10 | kVCoop)
                               : U == 3 ? kVUnmask : (kVWK | kVUnmask);
template <int U>
constexpr int kSplitNProd = U == 4 ? 2 : 1;
constexpr int kSplit8V = kVWK | kVUnmask | kVLayout8 | kVCross | kVCoop;
constexpr int kSplitQuadV = kVWK | kVUnmask | kVSkipWave2 | kVCoop | kVQuad;
// Threads per workgroup: what the kernel is compiled for (__launch_bounds__)
// and what launch_shape launches it with.
template <int PAIRS, int V, int NPROD>
constexpr int kSplitThreads = (V & kVLayout8) ? 512 : 64 * PAIRS * (1 + NPROD) + ((V & kVSkipWave2) ? 64 : 0);

// The studies that chose these shapes also built variants that lost.  A
// variant that needed a code path of its own and lost leaves the source
// (round 4's rule; results stay in profiles/, code in git history).  Rounds
// 1-3 (code in git history before round 4): the slot address computed at
// run time, the consumer at s_setprio 3, all 20 schedule reads in one burst,
// the W+K ring in global memory instead of LDS, wave 1 left empty instead of
// wave 2, the 8-wave layout split over the LDS store-path halves, and
// variants in which the consumer skipped its LDS reads or one side idled at
// the barriers (wrong digests by design); round 4: one schedule read every 4
// rounds instead of bursts (6.49 against 6.03 ms at 4096 chunks in the
// one-group shape, 6.60 against 6.31 at 32768 in the 8-wave one:
// spread_read_ab_r04.json).  profiles/issue_r01.json,
// split_variants_r01.json, split_2prod_sweep_r01.json,
// split_prio_read_r02.json, global_w_ab_r02.json, halves_ab_r03.json,
// spread_read_ab_r04.json.  Round 5, against the 8-wave shape's LDS
// contention at two groups per CU (code in git history up to commit
// b770692; DESIGN.md "Two groups per CU"): the second pair's schedule-read
// bursts issued half a burst interval after the first's (-0.7 %; with
// bursts of 10: -1.6 .. +0.3 %), one burst of 20 shifted the same way
// (+4.6 %), bursts of 10 at rounds 10/50 and 30/70 (+7.5 %;
// profiles/phase_ab_r05a.log .. c); and two 4-wave one-pair workgroups per
// CU, each with its own s_barrier, whose waves took their roles from the
// SIMD they landed on through a per-CU counter in device memory (6.36-6.42
// against 6.32 ms, profiles/simdrole_ab_r05.log; without the SIMD roles the
// dispatcher put both consumers on one SIMD on many CUs: 10.67 ms at 32768
// chunks, profiles/split_unit_ab_r03.json).  Shapes other than the
// product's 1 / 4 / 11 / 416 are built only into the A/B library
// (tools/ab_kernels.hip, `make ab`).

// The lgkmcnt(0) goes through the builtin so hipcc knows every LDS access
// before the barrier has completed (it then stops waiting for them later);
// the barrier itself is asm with a memory clobber so no LDS access moves
// across it.
__device__ __forceinline__ void split_barrier() {
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only (gfx9 encoding)
    asm volatile("s_barrier" ::: "memory");
}

// Study probe (A/B library only, kVProbe): the same barrier, with the
// shader-clock cycles the wave spends in it added to `acc`.
__device__ __forceinline__ void split_barrier_timed(uint64_t& acc) {
    __builtin_amdgcn_s_waitcnt(0xC07F);
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_barrier" ::: "memory");
    acc += __builtin_amdgcn_s_memtime() - t0;
}

// Producer: the 80-word schedule of one block, plus K, into its W block slot.
template <int T, bool WK>
struct SchedWrite {
    __device__ __forceinline__ static void run(uint32_t (&w)[16], uint8_t* slot, int lane) {
        if constexpr (T < 80) {
            if constexpr (T >= 16) sched_step<T>(w);
            if constexpr ((T & 3) == 3) {
                // ship W + K (K is constant over each group of 4: the round
                // ranges 0/20/40/60 are multiples of 4)
                constexpr int j = (T - 3) & 15;
                constexpr uint32_t k = WK ? round_k<T>() : 0u;
                *reinterpret_cast<uint4*>(slot + (T >> 2) * 1024 + lane * 16) =
                    make_uint4(w[j] + k, w[j + 1] + k, w[j + 2] + k, w[j + 3] + k);
            }
            SchedWrite<T + 1, WK>::run(w, slot, lane);
        }
    }
};

__device__ __forceinline__ uint32_t total_blocks(uint32_t len) {
    // nfull data blocks + 1 padded block (+1 more when len % 64 >= 56)
    return (len >> 6) + (((len & 63u) < 56u) ? 1u : 2u);
}

// Message words of block k for the producer's tail region (any block of any
// lane: full, partial+pad, length-only), big-endian, padding applied.
__device__ __forceinline__ void tail_block_words(const Entry& en, uint32_t k, uint32_t (&w)[16]) {
    const uint32_t nfull = en.len >> 6, rem = en.len & 63u;
    const uint64_t bits = (uint64_t)en.len * 8ull;
    if (k < nfull) {
        load_block16(en.p + 64ull * k, w);
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = bswap(w[j]);
    } else if (k == nfull) {
        if (rem) {
            load_block_partial(en.p + 64ull * k, rem, w);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = 0u;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = pad_word(bswap(w[j]), j, (int)rem);
        if (rem < 56u) {
            w[14] = (uint32_t)(bits >> 32);
            w[15] = (uint32_t)bits;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 14; ++j) w[j] = 0u;
        w[14] = (uint32_t)(bits >> 32);
        w[15] = (uint32_t)bits;
    }
}

// NPROD producer waves share a unit's blocks.  NPROD = 2 (U = 4): each
// producer owns one stage (2 blocks) per unit and ends the unit with its
// barrier after that stage's odd block.  NPROD = U = 2: each producer owns
// one block per unit and ends the unit after it.  A single producer ends the
// unit after block U-1.
template <int U, bool WK, int NPROD = 1>
__device__ __forceinline__ void produce_block(uint32_t k, uint32_t (&w)[16], uint8_t* ring, int lane,
                                              uint64_t* bw = nullptr) {
    const uint32_t m = k / U, j = k - m * U;
    SchedWrite<0, WK>::run(w, ring + ((m & 1u) * U + j) * kWBlockBytes, lane);
    // U == NPROD: each producer writes one block of every unit
    if (NPROD == 1 ? j == U - 1 : (U == NPROD || (k & 1u) == 1u)) {
        if (bw)
            split_barrier_timed(*bw);
        else
            split_barrier();
    }
}


// Producer side of one bulk stage: blocks 2s, 2s+1 from `cur`; once the
// second block's words are taken, `cur` is refilled with this producer's
// stage after next, s + 2 NPROD.
template <int U, bool WK, int NPROD = 1>
__device__ __forceinline__ void produce_stage(const Entry& en, uint32_t s, uint32_t S, Stage& cur,
                                              uint8_t* ring, int lane) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = bswap(cur.w[16 * half + j]);
        if (half == 1 && s + 2 * NPROD < S) load_stage(en.p + 128ull * (s + 2 * NPROD), cur);
        produce_block<U, WK, NPROD>(2 * s + half, w, ring, lane);
    }
}

// Shared-load producers (kVCoop): the raw 128 bytes (stage) or 64 bytes
// (own block) of the wave's 64 chunks go through the first bytes of the W
// slot they are about to fill (free at that point, as for the W writes that
// follow; the wave's LDS accesses complete in order, so the transposing
// reads precede the W writes over them).
template <int U, bool WK, int NPROD = 1>
__device__ __forceinline__ void produce_stage_coop(const u32x4u* const (&src)[8], uint32_t s, uint32_t S,
                                                   uint32_t (&cur)[32], uint8_t* ring, uint32_t lane) {
    const uint32_t k0 = 2 * s, m = k0 / U, j = k0 - m * U;
    uint8_t* raw = ring + ((m & 1u) * U + j) * kWBlockBytes;
    coop_store(raw, cur, lane);
    if (s + 2 * NPROD < S) coop_load(src, s + 2 * NPROD, cur);
    uint32_t x[32];
    wave_lds_order();
    coop_read(raw, lane, x);
    wave_lds_order();  // the W writes below overwrite what was just read
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t w[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] = bswap(x[16 * half + q]);
        produce_block<U, WK, NPROD>(k0 + half, w, ring, (int)lane);
    }
}

template <int U, bool WK, int NPROD>
__device__ __forceinline__ void produce_own_block_coop(const u32x4u* const (&src)[4], uint32_t k, uint32_t K,
                                                       uint32_t (&cur)[16], uint8_t* ring, uint32_t lane,
                                                       uint64_t* bw = nullptr) {
    const uint32_t m = k / U, j = k - m * U;
    uint8_t* raw = ring + ((m & 1u) * U + j) * kWBlockBytes;
    coop4_store(raw, cur, lane);
    if (k + 2 * NPROD < K) coop4_load(src, k + 2 * NPROD, cur);
    uint32_t w[16];
    wave_lds_order();
    coop4_read(raw, lane, w);
    wave_lds_order();  // the W writes below overwrite what was just read
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = bswap(w[q]);
    produce_block<U, WK, NPROD>(k, w, ring, (int)lane, bw);
}

// Producer that owns one block per unit (U == NPROD): block k from `cur`,
// which is then refilled with this producer's block after next, k + 2 NPROD.
template <int U, bool WK, int NPROD>
__device__ __forceinline__ void produce_own_block(const Entry& en, uint32_t k, uint32_t K,
                                                  uint32_t (&cur)[16], uint8_t* ring, int lane,
                                                  uint64_t* bw = nullptr) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = bswap(cur[j]);
    if (k + 2 * NPROD < K) load_block16(en.p + 64ull * (k + 2 * NPROD), cur);
    produce_block<U, WK, NPROD>(k, w, ring, lane, bw);
}

// Read groups P0 .. P1 - 1 (five ds_read_b128 each) of a block's 20.
template <int P0, int P1>
__device__ __forceinline__ void read_w_groups(const uint8_t* slot, uint32_t (&W)[80]) {
#pragma unroll
    for (int q = 5 * P0; q < 5 * P1; ++q) unpack4(W + 4 * q, *reinterpret_cast<const uint4*>(slot + q * 1024));
}

template <int V>
__device__ __forceinline__ void split_barrier_or_timed(uint64_t& acc) {
    if constexpr ((V & kVProbe) != 0)
        split_barrier_timed(acc);
    else
        split_barrier();
}

// The feed-forward of one block: masked (a lane past its last block keeps
// its state) or, while every lane is live, unmasked.
template <bool MASK>
__device__ __forceinline__ void commit(uint32_t (&h)[5], const uint32_t (&v)[5], bool live) {
    if constexpr (MASK) {
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = live ? h[i] + v[i] : h[i];
    } else {
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] += v[i];
    }
}

// A probing wave's (kVProbe) write-out over digest row `row` (wrong digests
// by design; A/B library only): the shader-clock cycles it waited in
// barriers, those of its whole loop, and the blocks it ran.
__device__ __forceinline__ void probe_store(const BatchArgs& A, uint32_t row, uint64_t waited, uint64_t total,
                                            uint32_t blocks) {
    uint32_t* o = reinterpret_cast<uint32_t*>(A.dig + 20ull * row);
    o[0] = (uint32_t)waited;
    o[1] = (uint32_t)(waited >> 32);
    o[2] = (uint32_t)total;
    o[3] = (uint32_t)(total >> 32);
    o[4] = blocks;
}

// Bursts B .. NB - 1 of a block's NB: each the burst's 20 / NB schedule reads
// of the next block, fenced so that hipcc keeps them together, then the
// 80 / NB rounds that run while they land.
template <int B, int NB, bool WK>
struct BurstRounds {
    __device__ __forceinline__ static void run(uint32_t (&v)[5], const uint32_t (&Wc)[80], uint32_t (&Wn)[80],
                                               const uint8_t* slot) {
        if constexpr (B < NB) {
            __builtin_amdgcn_sched_barrier(0);
            read_w_groups<4 * B / NB, 4 * (B + 1) / NB>(slot, Wn);
            __builtin_amdgcn_sched_barrier(0);
            RoundsW<80 * B / NB, 80 * (B + 1) / NB, WK>::run(v, Wc);
            BurstRounds<B + 1, NB, WK>::run(v, Wc, Wn, slot);
        }
    }
};

// Consumer: rounds of block k from Wc while W(k+1) streams into Wn.  All of
// it is straight-line (the barrier position is a compile-time function of
// the unrolled block index), so hipcc inserts no waits inside the rounds.
// Why W+K matters: the consumer's x = e + W + K as a VOP3 v_add3 (K in an
// SGPR or a VGPR alike) runs the one-wave round stream at ~4.98 cycles per
// instruction, the VOP2 v_add on a shipped W+K at the 4-cycle issue floor
// (tools/consumer_probe, profiles/issue_r01.json).  With ONE producer the
// extra 80 adds per block make the producer the slower wave (1878 vs 1757
// cycles per block), so single-producer kernels with 3- and 4-block units
// keep K in the consumer; the 4-block default has TWO producers (kSplitNProd)
// and ships W+K.  Measured on MI355X (profiles/split_variants_r01.json):
// 2-block units W+K ~5% ahead; unmasked commit helps every shape.
template <int U, int J, int V, bool MASK>
__device__ __forceinline__ void consume_block(uint32_t k, uint32_t T, uint32_t (&h)[5],
                                              const uint32_t (&Wc)[80], uint32_t (&Wn)[80],
                                              const uint8_t* ring, int lane, uint64_t& bw) {
    // Block k+1 (k = k0 + J, k0 a multiple of 2U) is unit (k0/U + (J+1)/U),
    // whose parity is that of (J+1)/U since k0/U is even, and sub-block
    // (J+1) % U: the slot address is a compile-time offset.  A barrier goes
    // in front of the first read of every new unit.
    constexpr int jn = (J + 1) % U;
    constexpr int slot_idx = (((J + 1) / U) & 1) * U + jn;
    const uint8_t* slot = ring + slot_idx * kWBlockBytes + lane * 16;
    uint32_t v[5] = {h[0], h[1], h[2], h[3], h[4]};
    if constexpr (jn == 0) split_barrier_or_timed<V>(bw);
    // two bursts of 10 reads (kVRead10), before rounds 0 and 40, or four of
    // 5, before rounds 0, 20, 40 and 60
    BurstRounds<0, (V & kVRead10) ? 2 : 4, (V & kVWK) != 0>::run(v, Wc, Wn, slot);
    commit<MASK>(h, v, k < T);
}

// 2U blocks (two units) per consumer iteration, unrolled, so Wa/Wb keep
// their parity and every barrier position is a compile-time constant.
template <int U, int J, int V, bool MASK>
struct ConsumeUnits {
    __device__ __forceinline__ static void run(uint32_t k0, uint32_t T, uint32_t (&h)[5],
                                               uint32_t (&Wa)[80], uint32_t (&Wb)[80],
                                               const uint8_t* ring, int lane, uint64_t& bw) {
        if constexpr (J < 2 * U) {
            consume_block<U, J, V, MASK>(k0 + J, T, h, Wa, Wb, ring, lane, bw);
            ConsumeUnits<U, J + 1, V, MASK>::run(k0, T, h, Wb, Wa, ring, lane, bw);
        }
    }
};

// The consumer wave of a split pair: every block's 80 rounds, W+K from the
// ring (see split_body).
template <int U, int V>
__device__ __forceinline__ void consume_all(const BatchArgs& A, const Entry& en, bool valid, uint32_t T,
                                            uint32_t units, const uint8_t* ring, int lane) {
    uint32_t h[5];
    load_init(A, en.id, h);
    uint32_t Wa[80], Wb[80];
    split_barrier();  // B_0
    read_w_groups<0, 4>(ring + lane * 16, Wa);
    // Iterations in which every valid lane is still inside its chunk
    // commit without the per-lane select (all of them for equal lengths).
    const uint32_t Tmin = __builtin_amdgcn_readfirstlane(wave_min(valid ? T : 0xffffffffu));
    const uint32_t full = (V & kVUnmask) ? min(Tmin, units * U) / (2 * U) * (2 * U) : 0u;
    uint32_t k = 0;
    uint64_t bw = 0;
    const uint64_t t0 = (V & kVProbe) ? __builtin_amdgcn_s_memtime() : 0;
    for (; k < full; k += 2 * U) ConsumeUnits<U, 0, V, false>::run(k, T, h, Wa, Wb, ring, lane, bw);
    for (; k < units * U; k += 2 * U) ConsumeUnits<U, 0, V, true>::run(k, T, h, Wa, Wb, ring, lane, bw);
    if constexpr ((V & kVProbe) != 0) {
        const uint64_t tot = __builtin_amdgcn_s_memtime() - t0;
        if (lane == 0) probe_store(A, en.id & ~63u, bw, tot, units * U);  // the group's first digest row
        return;
    }
    if (valid) emit(A, en.id, h);
}

// ---------------------------------------------------------- quad split ----
// kVQuad: four lanes (a quad) own one chunk, so a workgroup serves 16 chunks
// (lane l: chunk l >> 2 of the group) and a batch of n chunks spreads over
// ceil(n / 16) CUs.  A wave's issue cost does not depend on how many lanes
// are live, so the redundant rounds are free; what the layout buys is the
// schedule hand-off: one ds_read_b128 brings the quad 16 of a block's 80
// W+K words (lane j of the quad holds words 16 q + 4 j .. + 3 of read q), 5
// reads per block instead of 20, and round t takes its word from register
// 4 (t >> 4) + (t & 3) of lane (t >> 2) & 3 through a DPP quad_perm
// broadcast folded into the VOP2 add (v_add_u32_dpp: no extra instruction).
// Measured alone on a SIMD (tools/gen_quad_probe.py, gen_quad_hoist_probe.py;
// profiles/quad_consumer_probe.json, quad_hoist_probe.json): the DPP add
// issues at the 4-cycle floor (4.016 cycles per instruction, as the plain
// VOP2 add) when its 8-byte encoding starts at an 8-byte boundary, and takes
// ~5 cycles more at an address that is 4 mod 8 (the round stream alone: 1646.5
// cycles per block aligned, 2043 with every DPP add shifted by one s_nop).
// The other 8-byte instructions of a round do not care.  Every 4-byte
// instruction in the stream (an s_waitcnt, a VOP2 feed-forward add) flips the
// parity of what follows, so the rounds are kept free of them: the burst's
// lgkmcnt(0) comes after round 79 (the set is not read before the next block;
// with the five 4-byte feed-forward adds that makes six) and quad_align() pads
// to the boundary in front of round 0 where it still has to.  The
// whole block then takes 1678.5 cycles, as with a plain VOP2 add (1679),
// against 1698.5 with an s_waitcnt four rounds after the burst, which put
// those four rounds' DPP adds at the other parity than the rest.
//
// Ring: a block slot is 16 chunks x 80 words = 5 KiB, [q][lane][4 words] with
// q = 0..4, so each read and each write is one contiguous conflict-free KiB;
// 2 slots of U blocks are 40 KiB (U = 4) or 80 KiB (U = 8).  Wave roles,
// barriers and the masked commit are those of the 4-block-unit shape (consumer
// on wave 0, producers on waves 1 and 3, which take the stages of a unit in
// turn and join its barrier after their last stage in it).  Producers: one
// 16-byte load per lane brings the quad a whole block (lane j: piece j), the
// other three pieces come over DPP, every lane expands the whole schedule
// (redundant, the producers have the slack) and writes only the four words
// of each group of 16 that its ring position holds: 5 ds_write_b128 per
// block instead of 20.
constexpr int kQuadBlockBytes = 5 * 1024;

// x of lane SEL of the caller's quad (DPP quad_perm:[SEL,SEL,SEL,SEL]).
template <int SEL>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, SEL * 0x55, 0xf, 0xf, true);
}

// What follows starts at an 8-byte boundary (the assembler pads with one
// s_nop where it has to): see the DPP add's address parity above.
__device__ __forceinline__ void quad_align() { asm volatile(".p2align 3"); }

template <int T, int END>
struct RoundsQ {
    __device__ __forceinline__ static void run(uint32_t (&v)[5], const uint32_t (&W)[20]) {
        if constexpr (T < END) {
            round_step<T, true, true>(v, quad_bcast<(T >> 2) & 3>(W[4 * (T >> 4) + (T & 3)]));
            RoundsQ<T + 1, END>::run(v, W);
        }
    }
};

__device__ __forceinline__ void quad_read_w(const uint8_t* slot, uint32_t (&W)[20]) {
#pragma unroll
    for (int q = 0; q < 5; ++q) unpack4(W + 4 * q, *reinterpret_cast<const uint4*>(slot + q * 1024));
}

template <int U, int J, int V, bool MASK>
__device__ __forceinline__ void quad_consume_block(uint32_t k, uint32_t T, uint32_t (&h)[5],
                                                   const uint32_t (&Wc)[20], uint32_t (&Wn)[20],
                                                   const uint8_t* ring, int lane, uint64_t& bw) {
    // slot of block k + 1: as consume_block
    constexpr int jn = (J + 1) % U;
    constexpr int slot_idx = (((J + 1) / U) & 1) * U + jn;
    const uint8_t* slot = ring + slot_idx * kQuadBlockBytes + lane * 16;
    uint32_t v[5] = {h[0], h[1], h[2], h[3], h[4]};
    if constexpr (jn == 0) split_barrier_or_timed<V>(bw);
    __builtin_amdgcn_sched_barrier(0);
    quad_read_w(slot, Wn);
    __builtin_amdgcn_sched_barrier(0);
    // 80 rounds of 8-byte instructions from an 8-byte boundary; the fences
    // keep hipcc from moving a 4-byte instruction (a feed-forward add, a
    // wait) in between them
    quad_align();
    __builtin_amdgcn_sched_barrier(0);
    RoundsQ<0, 80>::run(v, Wc);
    __builtin_amdgcn_sched_barrier(0);
    // lgkmcnt(0): Wn has landed (80 rounds after its burst).  In front of the
    // feed-forward, where it also separates round 79's v_add3 from the add
    // that reads its result (hipcc otherwise puts an s_nop there, and with
    // it an odd number of 4-byte instructions into the block).
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    commit<MASK>(h, v, k < T);
    __builtin_amdgcn_sched_barrier(0);
}

template <int U, int J, int V, bool MASK>
struct QuadConsumeUnits {
    __device__ __forceinline__ static void run(uint32_t k0, uint32_t T, uint32_t (&h)[5], uint32_t (&Wa)[20],
                                               uint32_t (&Wb)[20], const uint8_t* ring, int lane, uint64_t& bw) {
        if constexpr (J < 2 * U) {
            quad_consume_block<U, J, V, MASK>(k0 + J, T, h, Wa, Wb, ring, lane, bw);
            QuadConsumeUnits<U, J + 1, V, MASK>::run(k0, T, h, Wb, Wa, ring, lane, bw);
        }
    }
};

// Producer: the 80-word schedule of one block; after every 16 words the
// window holds words 16 q .. 16 q + 15, of which lane j of the quad ships
// words 4 j .. 4 j + 3 (+ K of their rounds: K is constant over each group of
// 4 rounds, kq[q] is this lane's).
template <int T>
struct QuadSchedWrite {
    __device__ __forceinline__ static void run(uint32_t (&w)[16], uint8_t* slot, bool j1, bool j2,
                                               const uint32_t (&kq)[5]) {
        if constexpr (T < 80) {
            if constexpr (T >= 16) sched_step<T>(w);
            if constexpr ((T & 15) == 15) {
                constexpr int q = T >> 4;
                uint32_t o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t lo = j1 ? w[4 + i] : w[i], hi = j1 ? w[12 + i] : w[8 + i];
                    o[i] = (j2 ? hi : lo) + kq[q];
                }
                *reinterpret_cast<uint4*>(slot + q * 1024) = make_uint4(o[0], o[1], o[2], o[3]);
            }
            QuadSchedWrite<T + 1>::run(w, slot, j1, j2, kq);
        }
    }
};

// As produce_block with two producers: the producers take a unit's U / 2
// stages in turn, and each ends the unit with its barrier after the odd
// block of its last stage in it (one of the unit's last two stages; with
// U = 4 that is every stage).  U = 8 is an A/B-only shape (tools/ab_kernels.hip
// 816 / 817): it lost its gate to U = 4 by 39 cycles per block
// (profiles/quad_unit_probe.json), the product never launches it and no
// committed test runs it; it was checked against hashlib once, when that
// record was made, and is kept so that the measurement can be repeated.
template <int U>
__device__ __forceinline__ void quad_produce_block(uint32_t k, uint32_t (&w)[16], uint8_t* ring, int lane,
                                                   const uint32_t (&kq)[5]) {
    const uint32_t m = k / U, j = k - m * U;
    QuadSchedWrite<0>::run(w, ring + ((m & 1u) * U + j) * kQuadBlockBytes + lane * 16, (lane & 1) != 0,
                           (lane & 2) != 0, kq);
    if ((k & 1u) == 1u && ((k >> 1) % (U / 2)) + 2 >= U / 2) split_barrier();
}

// A lane's piece (16 bytes) of the quad's block -> the block's 16 big-endian
// words in every lane of the quad.
__device__ __forceinline__ void quad_block_words(const uint32_t (&x)[4], uint32_t (&w)[16]) {
    uint32_t y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = bswap(x[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = quad_bcast<0>(y[i]);
        w[4 + i] = quad_bcast<1>(y[i]);
        w[8 + i] = quad_bcast<2>(y[i]);
        w[12 + i] = quad_bcast<3>(y[i]);
    }
}

// Stage s (blocks 2s, 2s + 1) of the quad's chunk: this lane's 16 bytes of each.
__device__ __forceinline__ void quad_load_stage(const u32x4u* src, uint32_t s, uint32_t (&x)[8]) {
#pragma unroll
    for (int b = 0; b < 2; ++b) unpack4(x + 4 * b, src[8u * s + 4u * b]);
}

// Producer side of one bulk stage from `cur`, which is then refilled with
// this producer's stage after next (s + 4).
template <int U>
__device__ __forceinline__ void quad_produce_stage(const u32x4u* src, uint32_t s, uint32_t S, uint32_t (&cur)[8],
                                                   uint8_t* ring, int lane, const uint32_t (&kq)[5]) {
    uint32_t x0[4] = {cur[0], cur[1], cur[2], cur[3]}, x1[4] = {cur[4], cur[5], cur[6], cur[7]};
    if (s + 4 < S) quad_load_stage(src, s + 4, cur);
    uint32_t w[16];
    quad_block_words(x0, w);
    quad_produce_block<U>(2 * s, w, ring, lane, kq);
    quad_block_words(x1, w);
    quad_produce_block<U>(2 * s + 1, w, ring, lane, kq);
}

template <int U, int V>
__device__ __forceinline__ void quad_consume_all(const BatchArgs& A, const Entry& en, bool valid, uint32_t T,
                                                 uint32_t units, const uint8_t* ring, int lane, uint32_t wg) {
    uint32_t h[5];
    load_init(A, en.id, h);
    uint32_t Wa[20], Wb[20];
    split_barrier();  // B_0
    quad_read_w(ring + lane * 16, Wa);
    // waited for here (and the initial state's loads), so that hipcc puts no
    // s_waitcnt of its own in front of their first use in the loop, in between
    // the aligned rounds
    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
    const uint32_t Tmin = __builtin_amdgcn_readfirstlane(wave_min(valid ? T : 0xffffffffu));
    const uint32_t full = min(Tmin, units * U) / (2 * U) * (2 * U);
    uint32_t k = 0;
    uint64_t bw = 0;
    const uint64_t t0 = (V & kVProbe) ? __builtin_amdgcn_s_memtime() : 0;
    for (; k < full; k += 2 * U) QuadConsumeUnits<U, 0, V, false>::run(k, T, h, Wa, Wb, ring, lane, bw);
    for (; k < units * U; k += 2 * U) QuadConsumeUnits<U, 0, V, true>::run(k, T, h, Wa, Wb, ring, lane, bw);
    if constexpr ((V & kVProbe) != 0) {
        const uint64_t tot = __builtin_amdgcn_s_memtime() - t0;
        // the group's first digest row (uniform batches: id = position)
        if (lane == 0) probe_store(A, wg * 16u, bw, tot, units * U);
        return;
    }
    // the quad's four lanes hold the same state: one of them writes it
    if (valid && (lane & 3) == 0) emit(A, en.id, h);
}

// The body of one quad workgroup: chunks wg*16 .. wg*16 + 15 over 2 U x 5 KiB of LDS.
template <int U, int V, int NPROD>
__device__ __forceinline__ void quad_split_body(const BatchArgs& A, uint8_t* ring, uint32_t wg) {
    static_assert((U == 4 || U == 8) && NPROD == 2 && (V & kVSkipWave2) != 0 && (V & kVWK) != 0 &&
                      (V & kVUnmask) != 0,
                  "quad shape: 4- or 8-block units, two producers on waves 1 and 3, W+K shipped");
    int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave == 2) return;  // never joins a barrier: an ended wave is not waited for
    const bool producer = wave != 0;
    const uint32_t pidx = wave == 3 ? 1u : 0u;
    const int lane = threadIdx.x & 63;
    // a quad past the batch reads the group's first chunk (wg*16 < n for
    // every launched workgroup; clamped all the same)
    bool valid;
    const Entry en = lane_entry(A, wg * 16u + ((uint32_t)lane >> 2), min(wg * 16u, A.n - 1u), valid);
    const uint32_t T = valid ? (A.out_state ? (en.len >> 6) : total_blocks(en.len)) : 0u;
    const uint32_t Tmax = __builtin_amdgcn_readfirstlane(wave_max(T));
    const uint32_t units = (Tmax + 2 * U - 1) / (2 * U) * 2;
    if (!producer) {
        quad_consume_all<U, V>(A, en, valid, T, units, ring, lane, wg);
        return;
    }
    // this lane's K per group of 16 rounds: rounds 16 q + 4 (lane & 3) ..
    uint32_t kq[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const uint32_t t = 16u * q + 4u * ((uint32_t)lane & 3u);
        kq[q] = t < 20 ? K0 : t < 40 ? K1 : t < 60 ? K2 : K3;
    }
    // bulk: the stages every chunk of the group has; this producer's are
    // s = pidx, pidx + 2, ..: two in flight in registers
    const uint32_t S = bulk_stages(en, valid);
    const u32x4u* src = reinterpret_cast<const u32x4u*>(en.p) + (lane & 3);
    uint32_t C0[8], C1[8];
    uint32_t s = pidx;
    if (s < S) quad_load_stage(src, s, C0);
    if (s + 2 < S) quad_load_stage(src, s + 2, C1);
    for (; s + 2 < S; s += 4) {
        quad_produce_stage<U>(src, s, S, C0, ring, lane, kq);
        quad_produce_stage<U>(src, s + 2, S, C1, ring, lane, kq);
    }
    if (s < S) {
        quad_produce_stage<U>(src, s, S, C0, ring, lane, kq);
        s += 2;
    }
    // tail and padding stages (whole units: blocks past a lane's T are never
    // committed by the consumer); every lane of a quad builds the same words
    for (; 2 * s < units * U; s += 2) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const uint32_t k = 2 * s + half;
            uint32_t w[16];
            if (k < T) tail_block_words(en, k, w);
            quad_produce_block<U>(k, w, ring, lane, kq);
        }
    }
    split_barrier();  // matches the consumer's last (unused) read
}

// PAIRS consumer/producer pairs per workgroup: waves 0..PAIRS-1 consume,
// waves PAIRS..2*PAIRS-1 produce, pair p = (wave p, wave p+PAIRS).  Waves of
// a workgroup are dealt to the CU's SIMDs cyclically, so with PAIRS = 4 each
// SIMD hosts exactly one consumer and its own producer (the consumer keeps
// the SIMD's issue slots it needs; the producer fills the rest).  All waves
// share one s_barrier sequence, so the unit count is the workgroup maximum.
//
// NPROD = 2 (one pair, U = 4): wave 0 consumes, waves 1 and 2 produce,
// each writing one of the unit's two stages.  The producer's schedule work
// per block (byte swap, 64-word expansion, W+K, 20 ds_write_b128) is then
// half as long as the consumer's rounds, so the W+K hand-off, whose
// VOP2-add consumer issues at the 4-cycle floor, is no longer producer-bound
// (tools/consumer_probe, tools/replay_probe).
// The body of one split workgroup `wg` (groups wg*PAIRS ..) over the LDS
// array `lds` (PAIRS * 2 * U * kWBlockBytes bytes): sha1_split_kernel runs
// it on blockIdx.x, the mixed-batch kernel on the workgroups its plan gives
// to this shape.
template <int U, int PAIRS, int V, int NPROD>
__device__ __forceinline__ void split_body(const BatchArgs& A, uint8_t* lds, uint32_t wg) {
    if constexpr ((V & kVQuad) != 0) {
        static_assert(PAIRS == 1, "quad shape: one consumer per workgroup");
        quad_split_body<U, V, NPROD>(A, lds, wg);
        return;
    }
    // (what follows is instantiated for the quad shapes too, which the two
    // assertions therefore let pass: their 8-block unit meets neither)
    constexpr bool WK = (V & kVWK) != 0;
    static_assert((V & kVQuad) != 0 || PAIRS * 2 * U * kWBlockBytes <= 160 * 1024, "LDS");
    // Two producers for 2-block units (each owning one block per unit) were
    // measured slower at two groups per CU: 6 waves on 4 SIMDs put producers
    // on the consumers' SIMDs (profiles/split_2prod_sweep_r01.json).
    static_assert((V & kVQuad) != 0 || NPROD == 1 || (PAIRS == 1 && (U == 2 * NPROD || U == NPROD)) ||
                      (PAIRS == 2 && U == NPROD && (V & kVLayout8) != 0),
                  "two producers: one stage (U = 4) or one block (U = 2, 8-wave layout) each per unit");
    int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // With two producers, launch 4 waves and leave wave 2 empty, so both
    // producers (waves 1, 3) sit on the other LDS store-path half than the
    // consumer (a workgroup's waves alternate halves, SIMDs {0,1} / {2,3}):
    // measured 2-3% faster than 3 waves (profiles/split_2prod_sweep_r01.json).
    if constexpr ((V & kVSkipWave2) != 0) {
        static_assert(NPROD == 2 && PAIRS == 1, "skip-wave layout is for two producers");
        if (wave == 2) return;  // never joins a barrier: an ended wave is not waited for
        if (wave > 2) wave -= 1;
    }
    int pair = wave % PAIRS;
    bool producer = wave >= PAIRS;
    uint32_t pidx = producer ? (uint32_t)(wave - PAIRS) / PAIRS : 0u;  // producer index
    // Two pairs per workgroup with two producers each, 2-block units (one
    // block per producer per unit), 8 waves: a workgroup's waves w and w + 4
    // share a SIMD and waves 0-3 sit on four different SIMDs
    // (tools/wave_placement_probe), so the consumers go on waves 0 and 2 with
    // waves 4 and 6 left empty (each consumer alone on its SIMD), and each
    // pair's producers share one of the other two SIMDs: waves 1 + 5 and 3 + 7.
    // kVCross swaps which producer SIMD serves which consumer.
    if constexpr ((V & kVLayout8) != 0) {
        static_assert(PAIRS == 2 && NPROD == 2, "8-wave layout: two pairs, two producers each");
        if (wave == 4 || wave == 6) return;  // never joins a barrier
        producer = (wave & 1) != 0;
        pair = producer ? (((wave >> 1) & 1) ^ ((V & kVCross) ? 1 : 0)) : (wave >> 1);
        pidx = producer ? (uint32_t)(wave >> 2) : 0u;
    }
    const int lane = threadIdx.x & 63;
    uint8_t* ring = lds + pair * (2 * U * kWBlockBytes);
    const uint32_t group = wg * PAIRS + (uint32_t)pair;
    bool valid;
    const Entry en = lane_entry(A, group * 64u + (uint32_t)lane, fallback_entry(A, group), valid);
    // update mode (A.out_state): whole blocks only, no padding
    const uint32_t T = valid ? (A.out_state ? (en.len >> 6) : total_blocks(en.len)) : 0u;
    uint32_t Tmax = __builtin_amdgcn_readfirstlane(wave_max(T));
    if constexpr (PAIRS > 1) {
        // workgroup max through the (not yet used) ring; the second barrier
        // keeps producers from overwriting it before every wave has read it
        uint32_t* slots = reinterpret_cast<uint32_t*>(lds);
        if (!producer && lane == 0) slots[pair] = Tmax;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) Tmax = max(Tmax, slots[q]);
        Tmax = __builtin_amdgcn_readfirstlane(Tmax);
        __syncthreads();
    }
    // Both waves run whole units (2U blocks per consumer iteration); blocks
    // past a lane's T are computed on stale data and never committed.
    const uint32_t units = (Tmax + 2 * U - 1) / (2 * U) * 2;

    if (producer) {
        // ----------------------------- producer -------------------------
        // Bulk: stages (2 full blocks) that every lane has, with
        // branch-free loads hipcc can count (of any alignment); registers
        // hold the current stage and the next one in flight.
        const uint32_t S = bulk_stages(en, valid);
        if constexpr (U == NPROD) {
            // this producer's blocks: k = pidx, pidx + NPROD, ... (one per unit);
            // bulk over the full blocks every lane has, then tail/padding
            const uint32_t K = S * 2u;
            uint32_t B0[16], B1[16];
            uint32_t k = pidx;
            uint64_t pbw = 0;
            uint64_t* const pb = (V & kVProbe) ? &pbw : nullptr;
            const uint64_t pt0 = (V & kVProbe) ? __builtin_amdgcn_s_memtime() : 0;
            if constexpr ((V & kVCoop) != 0) {
                const u32x4u* src[4];
                coop_sources<4>(A, group, (uint32_t)lane, src);
                if (pidx < K) coop4_load(src, pidx, B0);
                if (pidx + NPROD < K) coop4_load(src, pidx + NPROD, B1);
                for (; k + NPROD < K; k += 2 * NPROD) {
                    produce_own_block_coop<U, WK, NPROD>(src, k, K, B0, ring, (uint32_t)lane, pb);
                    produce_own_block_coop<U, WK, NPROD>(src, k + NPROD, K, B1, ring, (uint32_t)lane, pb);
                }
                if (k < K) {
                    produce_own_block_coop<U, WK, NPROD>(src, k, K, B0, ring, (uint32_t)lane, pb);
                    k += NPROD;
                }
            } else {
                if (pidx < K) load_block16(en.p + 64ull * pidx, B0);
                if (pidx + NPROD < K) load_block16(en.p + 64ull * (pidx + NPROD), B1);
                for (; k + NPROD < K; k += 2 * NPROD) {
                    produce_own_block<U, WK, NPROD>(en, k, K, B0, ring, lane, pb);
                    produce_own_block<U, WK, NPROD>(en, k + NPROD, K, B1, ring, lane, pb);
                }
                if (k < K) {
                    produce_own_block<U, WK, NPROD>(en, k, K, B0, ring, lane, pb);
                    k += NPROD;
                }
            }
            for (; k < units * U; k += NPROD) {
                uint32_t w[16];
                if (k < T) tail_block_words(en, k, w);
                produce_block<U, WK, NPROD>(k, w, ring, lane, pb);
            }
            if constexpr ((V & kVProbe) != 0) {
                const uint64_t tot = __builtin_amdgcn_s_memtime() - pt0;
                // the group's digest row 1 + pidx
                if (lane == 0) probe_store(A, group * 64u + 1u + pidx, pbw, tot, units * U);
            }
            split_barrier();  // matches the consumer's last (unused) read
            return;
        }
        // this producer's stages: s = pidx, pidx + NPROD, ...
        uint32_t s = pidx;
        if constexpr ((V & kVCoop) != 0) {
            const u32x4u* src[8];
            coop_sources<8>(A, group, (uint32_t)lane, src);
            uint32_t C0[32], C1[32];
            if (pidx < S) coop_load(src, pidx, C0);
            if (pidx + NPROD < S) coop_load(src, pidx + NPROD, C1);
            for (; s + NPROD < S; s += 2 * NPROD) {
                produce_stage_coop<U, WK, NPROD>(src, s, S, C0, ring, (uint32_t)lane);
                produce_stage_coop<U, WK, NPROD>(src, s + NPROD, S, C1, ring, (uint32_t)lane);
            }
            if (s < S) {
                produce_stage_coop<U, WK, NPROD>(src, s, S, C0, ring, (uint32_t)lane);
                s += NPROD;
            }
        } else {
            Stage A0, A1;
            if (pidx < S) load_stage(en.p + 128ull * pidx, A0);
            if (pidx + NPROD < S) load_stage(en.p + 128ull * (pidx + NPROD), A1);
            for (; s + NPROD < S; s += 2 * NPROD) {
                produce_stage<U, WK, NPROD>(en, s, S, A0, ring, lane);
                produce_stage<U, WK, NPROD>(en, s + NPROD, S, A1, ring, lane);
            }
            if (s < S) {
                produce_stage<U, WK, NPROD>(en, s, S, A0, ring, lane);
                s += NPROD;
            }
        }
        // tail and padding stages (whole units: blocks past a lane's T are
        // never committed by the consumer)
        for (; 2 * s < units * U; s += NPROD) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const uint32_t k = 2 * s + half;
                uint32_t w[16];
                if (k < T) tail_block_words(en, k, w);
                produce_block<U, WK, NPROD>(k, w, ring, lane);
            }
        }
        split_barrier();  // matches the consumer's last (unused) read
    } else {
        // ----------------------------- consumer -------------------------
        consume_all<U, V>(A, en, valid, T, units, ring, lane);
    }
}

template <int U, int PAIRS, int V>
constexpr int kSplitLdsBytes = (V & kVQuad) ? 2 * U * kQuadBlockBytes : PAIRS * 2 * U * kWBlockBytes;

template <int U, int PAIRS, int V = kSplitV<U>, int NPROD = 1>
__global__ __launch_bounds__((kSplitThreads<PAIRS, V, NPROD>)) void sha1_split_kernel(
    BatchArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kSplitLdsBytes<U, PAIRS, V>];
    split_body<U, PAIRS, V, NPROD>(A, lds, blockIdx.x);
}

// Host side: every shape is launched with the block size its kernel was
// compiled for (with any other, the waves its body expects never meet at
// s_barrier).
template <int U, int PAIRS, int V = kSplitV<U>, int NPROD = 1>
void launch_shape(const BatchArgs& A, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL((sha1_split_kernel<U, PAIRS, V, NPROD>), dim3(grid), dim3(kSplitThreads<PAIRS, V, NPROD>), 0,
                       st, A);
}

#endif
