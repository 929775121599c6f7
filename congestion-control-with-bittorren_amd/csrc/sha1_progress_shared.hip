// sha1_progress_shared.hip -- the progressive-verify kernel for many
// sessions at once: sha1_progress_kernel (sha1_progress.hip) with the bulk
// blocks' loads shared across the wave.  Same PvArgs / PvEntry, same
// midstate, verdict, `done` and generation protocol; the host side
// (sha1_pv.hip) picks one of the two per launch.
//
// The lane kernel reads 16 bytes of each of 64 session buffers per load
// instruction, `stride` bytes apart in pinned host memory: 64 small reads
// over PCIe.  Here a workgroup is one wave and the wave is its 64 entries'
// chain (lane l owns entry 64 wg + l: midstate in, compressions, midstate or
// verdict out), but the loads of a block step are laid out four lanes per
// entry: instruction i reads the whole 64-byte block of entries 16i .. 16i+15
// (pv_shared_map.hpp), so one instruction touches 16 sessions' full blocks.
// The blocks go straight to LDS (LDS-DMA, global_load_lds_dwordx4; glds16 of
// sha1_fused.hpp) in coop4_store's swizzled image -- the swizzle is on the
// source address -- five 4 KiB buffers, four block steps ahead (a PCIe round
// trip is ~2 us each way, a block ~1.25 us of compression), and each lane
// takes its own block back with coop4_read: the LDS-DMA loop of
// fused_coop_body with per-entry block counts.  LDS-DMA rather than register
// staging: the load is an ordinary vector memory read whose data returns to
// LDS instead of VGPRs -- translation and caching follow the page, as for the
// lane kernel's loads of the same buffers -- and the issuing wave's counted
// vmcnt orders its own ds_read behind it; register staging four steps ahead
// would hold 64 more VGPRs and 4 ds_write_b128 per step for nothing.
//
// Block counts differ per lane: the wave loops to its longest, a lane past
// its own count discards the compression.  The loads are never predicated
// and never skipped -- the explicit s_waitcnt vmcnt(8) needs the same number
// in flight on every trip: past an entry's last block its four loaders read
// that block again (never a byte at or above the entry's upto, which the host
// may be writing), and a slot with nothing to load (no entry, a dropped
// entry, no whole block) reads the object's 64-byte dummy line in device
// memory.  No lane leaves before the loop: one with an invalid entry still
// loads for its neighbours.
//
// Resources (`make isa`, build/resource-usage-progress-shared.txt): 75 VGPRs,
// 28 SGPRs, 20480 bytes of LDS per workgroup (8 waves per CU by LDS), no
// scratch; the lane kernel at depth 4 takes 106 VGPRs.  In the loop, per
// block: s_waitcnt vmcnt(8), 4 ds_read_b128, 4 global_load_lds_dwordx4, the
// compression; the LDS reads are waited for one at a time (lgkmcnt 7..4) as
// the next block's byte swaps consume them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pv_shared_map.hpp"
#include "sha1_fused.hpp"

namespace {

__device__ __forceinline__ void st_sys(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

static_assert(pvmap::kBufBytes == kCoopBlockBytes && pvmap::kBufs == kCoopBlockBufs, "the LDS-DMA loop's buffers");

struct SharedSrc {
    const uint8_t* p[4];  // per instruction: the served slot's first block, at this lane's piece
    uint32_t nb[4];       // that slot's block count (1 for the dummy line)
};

// Block step k of every slot into the buffer at LDS address `buf`: four
// loads, always.
__device__ __forceinline__ void shared_load_step(const SharedSrc& s, uint32_t k, uint32_t buf) {
#pragma unroll
    for (uint32_t i = 0; i < pvmap::kInstr; ++i)
        glds16(s.p[i] + 64ull * pvmap::clamped_block(k, s.nb[i]), buf + pvmap::lds_instr_base(i));
}

// Block k: `cur` holds it (its LDS read was issued during block k-1).  At
// entry the loads of steps k+1 .. k+3 are outstanding (12): vmcnt(8) retires
// step k+1, whose read goes into `nxt`; step k+4's loads go into step k-1's
// buffer (read during block k-2, consumed during block k-1); then block k is
// compressed while the read is in flight.
__device__ __forceinline__ void shared_step(const SharedSrc& s, uint32_t k, uint32_t nb_own, const uint8_t* lds,
                                            uint32_t base, uint32_t lane, uint32_t& b, const uint32_t (&cur)[16],
                                            uint32_t (&nxt)[16], uint32_t (&h)[5]) {
    const uint32_t b1 = b + 1u == pvmap::kBufs ? 0u : b + 1u;
    const uint32_t bp = b == 0u ? pvmap::kBufs - 1u : b - 1u;
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    coop4_read(lds + b1 * pvmap::kBufBytes, lane, nxt);
    shared_load_step(s, k + pvmap::kAhead, base + bp * pvmap::kBufBytes);
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = bswap_fresh(cur[j]);
    uint32_t t[5] = {h[0], h[1], h[2], h[3], h[4]};
    compress(t, w);
    const bool live = k < nb_own;
#pragma unroll
    for (int i = 0; i < 5; ++i) h[i] = live ? t[i] : h[i];
    b = b1;
}

__global__ __launch_bounds__(64) void sha1_progress_shared_kernel(PvArgs P) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kCoopWaveBytes];
    const uint32_t lane = threadIdx.x;
    const uint32_t e = blockIdx.x * 64u + lane;
    uint4 e0 = make_uint4(0u, 0u, 0u, 0u), e1 = e0;
    if (e < P.n) {
        const uint4* ev = reinterpret_cast<const uint4*>(P.work + e);
        e0 = ev[0];
        e1 = ev[1];
    }
    const uint32_t session = e0.x, from = e0.y & ~63u, upto = e0.z, len = e0.w;
    const uint32_t final = e1.x, gen = e1.y;
    // the host builds the list; an entry outside its session's buffer is
    // dropped rather than followed (the lane kernel's conditions) -- its lane
    // stays, loading for the slots it serves
    const bool valid = e < P.n && session < P.sessions && len <= P.stride && upto <= len && from <= upto &&
                       !(final && upto != len);
    const uint8_t* base = P.data + P.stride * (valid ? session : 0u);
    uint32_t* st = P.state + 5u * (valid ? session : 0u);
    uint32_t h[5];
    init_state(h);
    if (valid && from != 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = st[i];
    }
    const uint32_t bulk_end = upto & ~63u;
    const uint32_t nb = valid ? (bulk_end - from) / 64u : 0u;
    const uint32_t K = __builtin_amdgcn_readfirstlane(wave_max(nb));

    if (K) {
        // what this lane's slot offers its four loaders, and what this lane
        // loads for the four slots it serves
        const pvmap::Offer o = pvmap::offer(valid, from, nb);
        const uint64_t own = reinterpret_cast<uint64_t>((o.dummy ? P.dummy : base) + o.first);
        const uint32_t own_lo = static_cast<uint32_t>(own), own_hi = static_cast<uint32_t>(own >> 32);
        const uint32_t own_nb = o.nb;
        SharedSrc s;
#pragma unroll
        for (uint32_t i = 0; i < pvmap::kInstr; ++i) {
            const int j = static_cast<int>(pvmap::slot(lane, i));
            const uint64_t lo = static_cast<uint32_t>(__shfl(own_lo, j)), hi = static_cast<uint32_t>(__shfl(own_hi, j));
            s.p[i] = reinterpret_cast<const uint8_t*>(lo | (hi << 32)) + pvmap::kPieceBytes * pvmap::piece(lane);
            s.nb[i] = __shfl(own_nb, j);
        }
        // every load the compiler counts (the entry, the midstate) has landed
        // before the first one it does not
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only (gfx9 encoding)
#pragma unroll
        for (int i = 0; i < 5; ++i) asm volatile("" : "+v"(h[i]));
        const uint32_t lbase = lds_addr(lds);
#pragma unroll
        for (uint32_t d = 0; d < pvmap::kAhead; ++d) shared_load_step(s, d, lbase + d * pvmap::kBufBytes);
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // step 0 landed
        uint32_t wa[16], wb[16];
        coop4_read(lds, lane, wa);
        uint32_t b = 0, k = 0;
        for (; k + 1 < K; k += 2) {
            shared_step(s, k, nb, lds, lbase, lane, b, wa, wb, h);
            shared_step(s, k + 1, nb, lds, lbase, lane, b, wb, wa, h);
        }
        if (k < K) shared_step(s, k, nb, lds, lbase, lane, b, wa, wb, h);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing of ours in flight past the loop
    }

    if (!valid) return;
    if (!final) {
#pragma unroll
        for (int i = 0; i < 5; ++i) st[i] = h[i];
        return;
    }
    finish_message(h, base + bulk_end, len & 63u, len);
    const uint32_t* x = P.expected + 8u * session;
    uint32_t* r = P.result + 8u * session;
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint32_t d = bswap(h[i]);  // the digest's bytes as a little-endian word
        diff |= d ^ x[i];
        r[i] = d;
    }
    r[5] = diff ? 1u : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    st_sys(P.done + session, gen);
}

}  // namespace

hipError_t launch_progress_shared(const PvArgs& P, hipStream_t st) {
    if (P.n == 0) return hipSuccess;
    if (!P.dummy) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sha1_progress_shared_kernel, dim3((P.n + 63u) / 64u), dim3(64), 0, st, P);
    return hipGetLastError();
}
