#!/usr/bin/env python3
"""Diagnostic only: generate tools/quad_probe.hip, the gate for a split
consumer in which a quad of four lanes owns one chunk.  One `ds_read_b128`
then brings the quad 16 of a block's 80 W+K words (5 reads per block instead
of 20), and round t takes its word from lane (t >> 2) & 3 of the quad through
a DPP `quad_perm` broadcast on the VOP2 add: register 4 (t >> 4) + (t & 3) of
a 20-register set.  Like tools/gen_consumer_probe.py (whose round and block
generators this reuses for the lane-per-chunk stream), every variant is one
wave running 8 blocks straight-line as explicit-register inline asm.

Variants, all timed in the same run:
    lane_wk_burst10   today's stream: VOP2 add, 20 reads in two bursts of 10
    lane_wk_none      the same without LDS reads (the round stream alone)
    quad_dpp_none     DPP add, no reads: the DPP add's issue cost
    quad_dpp_b5       DPP add, 5 reads in one burst before round 0
    quad_dpp_b5r40    ... before round 40
    quad_dpp_b3b2     ... 3 before round 0, 2 before round 40
    quad_dpp_spread   ... one before rounds 0, 16, 32, 48, 64
    quad_dpp_b5dummy  ... before round 0, landing in registers no round reads
    quad_dpp_b5wait   ... before round 0, s_waitcnt lgkmcnt(0) right after it
    quad_dpp_b5wN     ... before round 0, s_waitcnt lgkmcnt(0) before round N
    quad_dpp_b5rN     ... before round N (72, 76), the wait at the next block's top
    quad_dpp40_b5     DPP add in rounds 0..39 only, plain VOP2 add after
    quad_dppbc_b5     DPP add with bound_ctrl:0
    quad_vop2_*       the quad's 5 reads with a plain VOP2 add on the same
                      registers (wrong words, same issue): reads saved and DPP
                      cost apart

What they showed on MI355X (profiles/quad_consumer_probe.json; DESIGN.md
section 5, fact 5): the DPP add alone issues like the VOP2 add, but between a
ds_read and the next s_waitcnt lgkmcnt(0) each one costs ~5 cycles more, so
the burst needs an explicit lgkmcnt(0) a few rounds after it (b5w4).
That reading was wrong: what costs the 5 cycles is a DPP add at an address
that is 4 mod 8, and the 4-byte s_waitcnt instructions of these variants move
the adds behind them from one parity to the other
(tools/gen_quad_hoist_probe.py, profiles/quad_hoist_probe.json).

Each variant is launched REPS + 1 times (the first discarded); the probe
prints min / median / max cycles per block, so the spread of repeated runs
stands next to the difference between variants.

    python3 tools/gen_quad_probe.py && \\
    hipcc --offload-arch=gfx950 -O3 tools/quad_probe.hip -o tools/quad_probe
"""
from __future__ import annotations

import os

from gen_consumer_probe import ADDR, F, H, R5, ST, X, block_asm

HERE = os.path.dirname(os.path.abspath(__file__))
QSET = [8, 28]   # two 20-register W+K sets
DUMMY = 48       # b5dummy: the reads land in registers no round reads
REPS = 20
NBLK = 8


def quad_round(t: int, wbase: int, dpp: bool) -> list[str]:
    ia = (5 - t % 5) % 5
    a, b, c, d, e = (f"v{ST[(ia + i) % 5]}" for i in range(5))
    if t < 20:
        f = f"v_bfi_b32 v{F}, {b}, {c}, {d}"
    elif t < 40 or t >= 60:
        f = f"v_bitop3_b32 v{F}, {b}, {c}, {d} bitop3:0x96"
    else:
        f = f"v_bitop3_b32 v{F}, {b}, {c}, {d} bitop3:0xe8"
    w = f"v{wbase + 4 * (t >> 4) + (t & 3)}"
    s = (t >> 2) & 3
    use_dpp = dpp and not (dpp == "half" and t >= 40)
    x = (f"v_add_u32_dpp v{X}, {w}, {e} quad_perm:[{s},{s},{s},{s}] row_mask:0xf bank_mask:0xf"
         + (" bound_ctrl:0" if dpp == "bc" else "")
         if use_dpp else f"v_add_u32 v{X}, {e}, {w}")
    return [f"v_alignbit_b32 v{R5}, {a}, {a}, 27", f, x,
            f"v_add3_u32 {e}, v{R5}, v{F}, v{X}", f"v_alignbit_b32 {b}, {b}, {b}, 2"]


def quad_block(blk: int, sched: str, dpp: bool) -> list[str]:
    cur, nxt = QSET[blk % 2], QSET[(blk + 1) % 2]
    slot = (blk + 1) % 2  # two 5 KiB slots: [q][lane][4 words]
    dst = DUMMY if sched == "b5dummy" else nxt
    reads = [f"ds_read_b128 v[{dst + 4 * q}:{dst + 4 * q + 3}], v{ADDR} offset:{slot * 5120 + q * 1024}"
             for q in range(5)]
    at = {"none": {}, "b5": {0: reads}, "b5r40": {40: reads}, "b5dummy": {0: reads},
          "b5wait": {0: reads + ["s_waitcnt lgkmcnt(0)"]},
          "b3b2": {0: reads[0:3], 40: reads[3:5]},
          "spread": {16 * q: [reads[q]] for q in range(5)},
          # the burst before round 0, an s_waitcnt lgkmcnt(0) before round r
          **{f"b5w{r}": {0: reads, r: ["s_waitcnt lgkmcnt(0)"]} for r in (2, 4, 6, 8, 12)},
          # the burst before round r, the s_waitcnt lgkmcnt(0) at the next block's top
          **{f"b5r{r}": {r: reads} for r in (72, 76)}}[sched]
    first = at.get(0, [])
    out = list(first)
    if sched != "none":
        # the set filled during the previous block has landed; the reads
        # issued just now need not
        out.append(f"s_waitcnt lgkmcnt({sum(1 for r in first if r.startswith('ds_read'))})")
    for t in range(80):
        if t and t in at:
            out += at[t]
        out += quad_round(t, cur, dpp)
    for i in range(5):
        out.append(f"v_add_u32 v{H[i]}, v{H[i]}, v{ST[i]}")
    for i in range(5):
        out.append(f"v_mov_b32 v{ST[i]}, v{H[i]}")
    return out


def kernel(name: str, body: list[str], lds_bytes: int) -> str:
    body = body + ["s_waitcnt lgkmcnt(0)"]
    asm = "\\n".join(body)
    clobbers = ", ".join(f'"v{i}"' for i in list(range(0, 168)) + H)
    return f'''
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void {name}(uint64_t* st) {{
    __shared__ __attribute__((aligned(16))) uint8_t lds[{lds_bytes}];
    for (int i = threadIdx.x; i < {lds_bytes} / 4; i += 64) reinterpret_cast<uint32_t*>(lds)[i] = i * 2654435761u;
    __syncthreads();
    const uint32_t a = (uint32_t)(uintptr_t)lds + threadIdx.x * 16;
    uint64_t t0, t1, q0, q1;
    asm volatile("v_mov_b32 v{ADDR}, %0\\n"
                 "v_mov_b32 v0, 1\\n v_mov_b32 v1, 2\\n v_mov_b32 v2, 3\\n v_mov_b32 v3, 4\\n v_mov_b32 v4, 5\\n"
                 "v_mov_b32 v180, 1\\n v_mov_b32 v181, 2\\n v_mov_b32 v182, 3\\n v_mov_b32 v183, 4\\n v_mov_b32 v184, 5"
                 :: "v"(a) : "v{ADDR}", "v0", "v1", "v2", "v3", "v4", "v180", "v181", "v182", "v183", "v184");
    asm volatile("s_memtime %0\\n s_memrealtime %1\\n s_waitcnt lgkmcnt(0)" : "=s"(t0), "=s"(q0));
    asm volatile("{asm}" ::: {clobbers}, "memory");
    asm volatile("s_memtime %0\\n s_memrealtime %1\\n s_waitcnt lgkmcnt(0)" : "=s"(t1), "=s"(q1));
    if (threadIdx.x == 0) {{ st[0] = t1 - t0; st[1] = q1 - q0; }}
}}
'''


def variants():
    out = []
    for sched in ("burst10", "none"):
        body = []
        for blk in range(NBLK):
            body += block_asm(blk, sched, "bfi", "O1", True)
        out.append((f"lane_wk_{sched}", body, 2 * 20480))
    for dpp, tag, scheds in ((True, "dpp", ("none", "b5", "b5r40", "b3b2", "spread", "b5dummy", "b5wait",
                                           "b5w2", "b5w4", "b5w6", "b5w8", "b5w12", "b5r72", "b5r76")),
                             ("half", "dpp40", ("b5",)), ("bc", "dppbc", ("b5",)),
                             (False, "vop2", ("none", "b5", "b3b2", "b5dummy", "b5w6"))):
        for sched in scheds:
            body = []
            for blk in range(NBLK):
                body += quad_block(blk, sched, dpp)
            out.append((f"quad_{tag}_{sched}", body, 2 * 5120))
    return out


def main(vs=None, out="quad_probe.hip"):
    parts = ['''// GENERATED by tools/gen_quad_probe.py or a sibling generator (diagnostic only).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { \\
    fprintf(stderr, "%s: %s\\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
''']
    vs = vs or variants()
    for name, body, lds in vs:
        parts.append(kernel(name, body, lds))
    parts.append(f'''
static void run(const char* name, void (*k)(uint64_t*), int ninstr, int nvalu, int nread) {{
    const int reps = {REPS}, nblk = {NBLK};
    uint64_t* st;
    CHECK(hipMalloc(&st, 32));
    double c[reps], ghz = 0;
    for (int rep = 0; rep <= reps; ++rep) {{
        hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, st);
        CHECK(hipDeviceSynchronize());
        uint64_t h[2];
        CHECK(hipMemcpy(h, st, 16, hipMemcpyDeviceToHost));
        if (rep > 0) {{ c[rep - 1] = (double)h[0] / nblk; ghz = h[0] / (h[1] * 10.0); }}
    }}
    std::sort(c, c + reps);
    printf("{{\\"quad_probe\\": \\"%s\\", \\"instr_per_block\\": %.2f, \\"valu_per_block\\": %d, "
           "\\"reads_per_block\\": %d, \\"cycles_per_block\\": {{\\"min\\": %.1f, \\"median\\": %.1f, \\"max\\": %.1f}}, "
           "\\"cycles_per_instr\\": %.3f, \\"clock_ghz\\": %.3f, \\"reps\\": %d}}\\n", name,
           (double)ninstr / nblk, nvalu / nblk, nread / nblk, c[0], c[reps / 2], c[reps - 1],
           c[reps / 2] * nblk / ninstr, ghz, reps);
    CHECK(hipFree(st));
}}
int main() {{
''')
    for name, body, _ in vs:
        nvalu = sum(1 for l in body if l.startswith("v_"))
        nread = sum(1 for l in body if l.startswith("ds_read"))
        ninstr = sum(1 for l in body if not l.startswith("."))  # directives are not instructions
        parts.append(f'    run("{name}", {name}, {ninstr}, {nvalu}, {nread});\n')
    parts.append("    return 0;\n}\n")
    with open(os.path.join(HERE, out), "w") as f:
        f.write("".join(parts))


if __name__ == "__main__":
    main()
