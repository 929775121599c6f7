// sha1_progress.hip -- the progressive-verify kernel (sha1chunk_pv,
// include/sha1chunk.h; host side: sha1_pv.hip).
//
// The peer accepts a chunk only after its SHA-1 matches (packet_handler.c:
// 469-472 -> job.c:217-228), and every other entry point starts that hash
// when the chunk is complete: one serial chain of 8192 compressions after the
// last packet.  The reference's reliable UDP layer knows long before that
// which bytes are final: cumulative_ack (reliable_udp.c:300-324) keeps
// last_packet_acked, so bytes [0, 1484 x last_packet_acked) of
// recv_session->data no longer change.  This kernel hashes those bytes while
// the rest of the chunk is still arriving.
//
// One lane per work-list entry {session, from, upto, len, final} (PvEntry,
// sha1_kernels.h), 256-thread workgroups, no LDS, no barrier, no waiting: a
// lane resumes its session's midstate (the IV when from == 0, so a reused
// session slot needs no reset), compresses the whole blocks of [from, upto)
// straight out of the session's pinned host buffer and writes the midstate
// back -- or, on the final entry, pads, compares with the expected digest
// and publishes the verdict to host memory.
//
// The host owns the byte accounting, the device only the midstates: a lane
// reads no byte at or above its entry's upto (the final partial block is
// read by dwords that each hold a message byte, finish_message; what such a
// dword holds past len is masked by the padding), so the host may write the
// rest of the buffer while the kernel runs.
//
// Loads cross PCIe (~2 us each way), so a lane keeps DEPTH 64-byte blocks in
// flight ahead of the block it compresses, in registers, refilled without a
// branch: past its last block a lane re-reads that block (never a byte
// beyond it) and discards the result.  Lanes of a wave have different block
// counts; the wave loops to its longest lane's count and the others are
// masked off by the loop condition.  Stages are single blocks, not the
// fused kernel's 128 bytes, because a mark may leave an odd block count.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha1_device.hpp"
#include "sha1_kernels.h"

namespace {
using namespace s1;

__device__ __forceinline__ void st_sys(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A whole block at a 16-byte aligned address (buffers start on 128-byte
// lines, from is a multiple of 64): 4 x global_load_dwordx4.
__device__ __forceinline__ void load_block_aligned(const uint8_t* p, uint32_t (&w)[16]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint4 x = q[j];
        w[4 * j + 0] = x.x;
        w[4 * j + 1] = x.y;
        w[4 * j + 2] = x.z;
        w[4 * j + 3] = x.w;
    }
}

template <int DEPTH>
__global__ __launch_bounds__(256) void sha1_progress_kernel(PvArgs P) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= P.n) return;
    const uint4* ev = reinterpret_cast<const uint4*>(P.work + e);
    const uint4 e0 = ev[0], e1 = ev[1];
    const uint32_t session = e0.x, from = e0.y & ~63u, upto = e0.z, len = e0.w;
    const uint32_t final = e1.x, gen = e1.y;
    // the host builds the list; an entry outside its session's buffer is
    // dropped rather than followed
    if (session >= P.sessions || len > P.stride || upto > len || from > upto || (final && upto != len)) return;

    const uint8_t* base = P.data + P.stride * session;
    uint32_t* st = P.state + 5u * session;
    uint32_t h[5];
    if (from == 0) {
        init_state(h);
    } else {
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = st[i];
    }

    const uint32_t bulk_end = upto & ~63u;
    const uint32_t nb = (bulk_end - from) / 64u;
    if (nb) {
        const uint8_t* q = base + from;
        const uint32_t last = nb - 1u;
        uint32_t buf[DEPTH][16];
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            // in block order, as the loop refills them: the loop's waits can
            // then be partial (the oldest block's loads, vmcnt(4 (DEPTH - 1)))
            load_block_aligned(q + 64ull * min(static_cast<uint32_t>(j), last), buf[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (uint32_t k = 0; k < nb; k += DEPTH) {
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                uint32_t w[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) w[i] = bswap_fresh(buf[j][i]);
                // The refill stays here, ahead of this block's compression:
                // without the two fences hipcc merges it with the loads
                // before the loop into one load at the top of the next trip
                // and waits for all of them there (vmcnt(0) once per trip,
                // the PCIe latency exposed every DEPTH blocks).
                __builtin_amdgcn_sched_barrier(0);
                load_block_aligned(q + 64ull * min(k + j + DEPTH, last), buf[j]);
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                uint32_t t[5] = {h[0], h[1], h[2], h[3], h[4]};
                compress(t, w);
                const bool live = k + j < nb;
#pragma unroll
                for (int i = 0; i < 5; ++i) h[i] = live ? t[i] : h[i];
            }
        }
    }

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

hipError_t launch_progress(const PvArgs& P, int depth, hipStream_t st) {
    if (P.n == 0) return hipSuccess;
    const dim3 grid((P.n + 255u) / 256u), block(256);
    switch (depth) {
    case 2: hipLaunchKernelGGL(sha1_progress_kernel<2>, grid, block, 0, st, P); break;
    case 4: hipLaunchKernelGGL(sha1_progress_kernel<4>, grid, block, 0, st, P); break;
    case 8: hipLaunchKernelGGL(sha1_progress_kernel<8>, grid, block, 0, st, P); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
