// sha1_fused.hpp -- the one-wave bodies of the gfx950 SHA-1 kernels: schedule
// and rounds of 64 chunks in one wave's registers, each lane streaming its own
// chunk (fused_body) or the wave sharing its loads through LDS-DMA
// (fused_coop_body, glds*).  Included by sha1_kernels.hip and, for glds16, by
// sha1_progress_shared.hip.  Everything here is internal to the including file.
#ifndef SHA1_FUSED_HPP
#define SHA1_FUSED_HPP

#include "sha1_lane.hpp"

// --------------------------------------------------------------- fused ----
// One wave, 64 chunks, schedule and rounds in registers (~630 VALU per
// block).  Best once there are enough chunks for two or more waves per SIMD:
// then the SIMD, not one wave's issue rate, is the limit and the split
// kernel's LDS hand-off is pure overhead.  Each lane streams its own chunk
// with 16-byte loads (dword loads shifted at use when the wave's chunks are
// not all 16-byte aligned), two 128-byte stages (4 blocks) in flight in VGPRs so
// HBM latency under full load stays covered.
template <typename V>
__device__ __forceinline__ void fused_stage(uint32_t s, uint32_t S, const Entry& en, Stage& cur,
                                            uint32_t (&h)[5]) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = bswap_fresh(cur.w[16 * half + j]);
        if (half == 1 && s + 2 < S) load_stage<V>(en.p + 128ull * (s + 2), cur);
        compress(h, w);
    }
}

// Stages 0 .. S-1 of every lane's chunk, each lane loading its own.
template <typename V>
__device__ __forceinline__ void fused_lane_stages_v(const Entry& en, uint32_t S, uint32_t (&h)[5]) {
    Stage A0, A1;
    if (S > 0) load_stage<V>(en.p, A0);
    if (S > 1) load_stage<V>(en.p + 128, A1);
    uint32_t s = 0;
    for (; s + 1 < S; s += 2) {
        fused_stage<V>(s, S, en, A0, h);
        fused_stage<V>(s + 1, S, en, A1, h);
    }
    if (s < S) fused_stage<V>(s, S, en, A0, h);
}

// The same for a wave whose chunks are not all 16-byte aligned: dword loads
// (RawSpan, from p & ~3) two stages ahead, funnel-shifted by p & 3 at use.
// Lane-per-chunk byte-unaligned 16-byte loads were slower here (65536 x
// 512 KiB 1..15 bytes off: 13.6 ms against 11.2; profiles/misaligned_r02.json).
__device__ __forceinline__ void fused_stage_any(uint32_t s, uint32_t S, const Entry& en, RawSpan<32>& cur,
                                                uint32_t (&h)[5]) {
    const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(en.p) & 3u);
    uint32_t w[16];
    shift_raw<32, 0, 16>(cur, sh, w);
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = bswap_fresh(w[j]);
    compress(h, w);
    shift_raw<32, 16, 16>(cur, sh, w);
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = bswap_fresh(w[j]);
    if (s + 2 < S) load_raw<32>(en.p + 128ull * (s + 2), cur);
    compress(h, w);
}

__device__ __forceinline__ void fused_lane_stages_any(const Entry& en, uint32_t S, uint32_t (&h)[5]) {
    RawSpan<32> A0, A1;
    if (S > 0) load_raw<32>(en.p, A0);
    if (S > 1) load_raw<32>(en.p + 128, A1);
    uint32_t s = 0;
    for (; s + 1 < S; s += 2) {
        fused_stage_any(s, S, en, A0, h);
        fused_stage_any(s + 1, S, en, A1, h);
    }
    if (s < S) fused_stage_any(s, S, en, A0, h);
}

__device__ __forceinline__ void fused_lane_stages(const Entry& en, bool valid, uint32_t S, uint32_t (&h)[5]) {
    if (wave_all(!valid || (reinterpret_cast<uintptr_t>(en.p) & 15u) == 0))
        fused_lane_stages_v<uint4>(en, S, h);
    else
        fused_lane_stages_any(en, S, h);
}

// The body of one fused wave: message e's lane (group e / 64).
__device__ __forceinline__ void fused_body(const BatchArgs& A, uint32_t e) {
    bool valid;
    const Entry en = lane_entry(A, e, fallback_entry(A, e / 64u), valid);
    uint32_t h[5];
    load_init(A, en.id, h);
    const uint32_t S = bulk_stages(en, valid);
    fused_lane_stages(en, valid, S, h);
    if (valid) {
        lane_blocks(A, en, 2u * S, h);
        emit(A, en.id, h);
    }
}


// ---------------------------------------------------------- coop fused ----
// The fused wave with its stage loads shared across the wave
// (coop_load / coop_store / coop_read, sha1_lane.hpp).  Used by the
// mixed kernel, whose workgroups own the CU's LDS anyway (16 KiB per wave:
// two stage buffers).
__device__ __forceinline__ void coop_compress(const uint32_t (&cur)[32], uint32_t (&h)[5]) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = bswap_fresh(cur[16 * half + j]);
        compress(h, w);
    }
}

// LDS-DMA (global_load_lds_dwordx4): each lane's 16 bytes from its own
// global address land at the wave-uniform LDS byte address `lds_dst` +
// 16 x lane, with no VGPR and no ds_write.  M0 carries the LDS address and is
// saved and restored in the same statement (hipcc reserves it).  hipcc does
// not count these loads: the caller waits for them with an explicit
// s_waitcnt vmcnt (and drains them before any load hipcc counts).
typedef __attribute__((address_space(3))) uint8_t lds_u8;
__device__ __forceinline__ uint32_t lds_addr(const uint8_t* p) {
    return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((const lds_u8*)p));
}
__device__ __forceinline__ void glds16(const void* src, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds_dst)
                 : "memory");
}

// Block k of the group's 64 chunks into the 4 KiB buffer at LDS address
// `buf`: instruction i reads block k of chunks 16i .. 16i+15 (4 lanes per
// chunk), lane l writing buf + i KiB + 16 l.  p[i] is lane l's source in
// chunk 16i + l/4 at byte 16 x ((l%4 - l/16) & 3) of the block, so the LDS
// image is coop4_store's swizzled one (piece q of chunk c at
// c*64 + ((q + c/4) & 3)*16) and coop4_read hands each lane its chunk.
__device__ __forceinline__ void glds_block(const uint8_t* const (&p)[4], uint32_t k, uint32_t buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(p[i] + 64ull * k, buf + 1024u * (uint32_t)i);
}

// Block k of the LDS-DMA fused loop: `cur` holds block k (its LDS read
// issued during block k-1); block k+1's read is issued into `nxt` once its
// DMA has landed, block k+4's DMA goes into block k-1's buffer (read during
// block k-2, consumed during block k-1), then block k is compressed while
// block k+1's read is in flight.  At the start of block k the DMAs of
// blocks k+1..k+3 are outstanding (12 loads): vmcnt(8) retires block k+1.
__device__ __forceinline__ void glds_stage_step(const uint8_t* const (&p)[4], uint32_t k, uint32_t K,
                                                const uint8_t* lds, uint32_t base, uint32_t lane, uint32_t& b,
                                                const uint32_t (&cur)[16], uint32_t (&nxt)[16],
                                                uint32_t (&h)[5]) {
    const uint32_t b1 = b + 1u == kCoopBlockBufs ? 0u : b + 1u;      // block k+1's buffer
    const uint32_t bp = b == 0u ? kCoopBlockBufs - 1u : b - 1u;      // block k-1's buffer
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    coop4_read(lds + b1 * kCoopBlockBytes, lane, nxt);
    glds_block(p, min(k + kCoopBlockBufs - 1u, K - 1u), base + bp * kCoopBlockBytes);
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = bswap_fresh(cur[j]);
    compress(h, w);
    b = b1;
}

// lds: this wave's kCoopWaveBytes.  Same contract as fused_body.  The
// wave's LDS accesses complete in order, so a stage's stores precede its
// reads and the reads of a buffer precede its next stores; hipcc keeps the
// program order of these lane-dependent accesses it cannot prove disjoint.
// One stage in flight in registers: a second (as fused_body keeps) was
// slower -- hipcc moved its loads next to their LDS stores (65536 x 512 KiB
// 13.1 against 10.4 ms, profiles/coop_split_ab_r02.json).
__device__ __forceinline__ void fused_coop_body(const BatchArgs& A, uint32_t e, uint8_t* lds) {
    const uint32_t group = e / 64u, lane = e & 63u;
    bool valid;
    const Entry en = lane_entry(A, e, fallback_entry(A, group), valid);
    uint32_t h[5];
    load_init(A, en.id, h);
    const uint32_t S = bulk_stages(en, valid);
    // A group whose chunks lie together (in place, or permuted within a
    // span of about their own bytes) streams lane-per-chunk: no UTCL1
    // thrash to avoid there, and the shared loads' LDS round trip costs
    // 1-4 % (profiles/coop_split_ab_r02.json).
    uint64_t lo = valid ? reinterpret_cast<uint64_t>(en.p) : ~0ull;
    uint64_t hi = valid ? reinterpret_cast<uint64_t>(en.p) + en.len : 0ull;
    uint64_t bytes = valid ? en.len : 0ull;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = min(lo, (uint64_t)__shfl_xor(lo, m));
        hi = max(hi, (uint64_t)__shfl_xor(hi, m));
        bytes += (uint64_t)__shfl_xor(bytes, m);
    }
    const bool together = hi - lo <= 2 * bytes + (2ull << 20);
    if (S > 0 && together && wave_all(!valid || (reinterpret_cast<uintptr_t>(en.p) & 15u) == 0)) {
        fused_lane_stages_v<uint4>(en, S, h);
    } else if (S > 0) {  // scattered or not 16-byte aligned: shared loads (any alignment)
        // Block loads shared across the wave go straight to LDS
        // (global_load_lds), four blocks ahead in five 4 KiB buffers; each
        // lane then reads its own chunk's block back (coop4_read).  Round 4
        // staged 128-byte stages through VGPRs (8 global loads + 8
        // ds_write_b128 per stage) with one stage in flight: this wave IS its
        // chunks' chain (alone on its SIMD at F = 4), so a scattered load that
        // had not landed one stage (~4900 cycles) later stalled it, and a
        // second register stage did not fit the mixed kernel's 256 VGPRs
        // (65536 uniform chunks permuted: 11.4 ms against 10.1 in place).
        const uint32_t K = 2u * S;
        const uint8_t* p[4];
        const uint32_t piece = ((lane & 3u) - (lane >> 4)) & 3u;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t ej = group * 64u + 16u * i + (lane >> 2);
            p[i] = fetch_entry(A, ej < A.n ? ej : fallback_entry(A, group)).p + 16u * piece;
        }
        const uint32_t base = lds_addr(lds);
        // blocks 0..3 in flight (past the bulk region: the last block again,
        // a harmless repeat that keeps the count of loads in flight fixed)
#pragma unroll
        for (uint32_t d = 0; d < kCoopBlockBufs - 1u; ++d) glds_block(p, min(d, K - 1u), base + d * kCoopBlockBytes);
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // block 0 landed
        uint32_t wa[16], wb[16];
        coop4_read(lds, lane, wa);
        uint32_t b = 0;  // buffer of block k
        uint32_t k = 0;
        for (; k + 1 < K; k += 2) {
            glds_stage_step(p, k, K, lds, base, lane, b, wa, wb, h);
            glds_stage_step(p, k + 1, K, lds, base, lane, b, wb, wa, h);
        }
        if (k < K) glds_stage_step(p, k, K, lds, base, lane, b, wa, wb, h);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing of ours in flight past the loop
    }
    if (valid) {
        lane_blocks(A, en, 2u * S, h);
        emit(A, en.id, h);
    }
}

#endif
