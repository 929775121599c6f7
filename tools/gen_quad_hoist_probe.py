#!/usr/bin/env python3
"""Diagnostic only: generate tools/quad_hoist_probe.hip.  It began as the gate
for moving the quad consumer's first DPP adds out of the window between its
5-read burst and the burst's `s_waitcnt lgkmcnt(0)`, on the belief that a
`v_add_u32_dpp` issued inside that window costs ~5 cycles more.  What it
found instead (profiles/quad_hoist_probe.json):
a DPP add costs ~5 cycles more when its 8-byte encoding starts at an address
that is 4 mod 8, whatever the LDS reads do, and every 4-byte instruction in
the stream (an s_waitcnt, an s_nop, a VOP2 add or move) flips the parity of
what follows it.  tools/dump_isa.sh on the built probe shows the addresses.

The hoist: x_t = e_t + WK_t of rounds 0..3 depends only on the state at the
top of the block (e, d, c, rol30(b)) and on the W+K set that landed one block
earlier, so those four adds can be issued before the burst; round 4's needs
rol30(a) in a register of its own (a is still read by round 0's rotate and
round 1's F).  From round 5 on e_t is a round's output: no later round can be
hoisted without extra instructions.  The instruction count does not change:
round 0's F and its rol30(b) (and round 1's rol30 for 5 rounds) are issued
early.

Variants, with the protocol of tools/gen_quad_probe.py (one wave, 8 blocks,
20 timed launches, min / median / max) and its `quad_dpp_b5w4` (the stream
shipped first), `quad_vop2_b5` and `quad_dpp_none` timed in the same run:
    quad_dpp_hoist4[_wN]    x0..x3 before the burst, lgkmcnt(0) before round 4
                            (or N = 2, 3, 6)
    quad_dpp_hoist5[_wN]    x0..x4 before the burst, the wait before round 5
                            (or N = 4, 6, 8)
    quad_dpp_hoist6/7/8     hoist5, plus the W+K words of rounds 5.. broadcast
                            into plain registers before the burst (one
                            v_mov_dpp MORE per round) and added with a plain
                            4-byte VOP2 add; the wait before round 6 / 7 / 8
                            (not the equal-instruction-count hoist of 8 rounds
                            one might want: from round 5 on e_t is a round's
                            output, so there is none; with the parity
                            finding the question of a later wait is moot)
    ..._c5                  an `s_waitcnt lgkmcnt(5)` (a no-op) after the burst
    hoist5_nop1/_nop3/_n5   1 or 3 `s_nop` before the burst, or 1 after it
    hoist5_vmov3, hoist4_vmov3   3 plain (4-byte) v_mov before the burst
    hoist5[_w8]_movdpp3     3 (8-byte) v_mov_dpp before the burst
    quad_dpp_b5_aligned_e64 no hoist: burst, 80 DPP rounds, feed-forward,
                            lgkmcnt(0); the probe's state moves as 8-byte
                            VOP3, so a block holds 6 four-byte instructions
    quad_dpp_b5_aligned_p2  the same with 4-byte moves (11 per block) and
                            `.p2align 3` in front of round 0
    quad_dpp_none_shift4    the round stream alone behind one s_nop: every
                            DPP add at 4 mod 8
Fast (1678.5..1698.5 cycles per block) are exactly the variants whose blocks
hold an even number of 4-byte instructions between one block's DPP adds and
the next's; the others alternate parity by block (1875..1907).

    python3 tools/gen_quad_hoist_probe.py && \\
    hipcc --offload-arch=gfx950 -O3 tools/quad_hoist_probe.hip -o tools/quad_hoist_probe
"""
from __future__ import annotations

from gen_consumer_probe import ADDR, F, H, R5, ST, X
from gen_quad_probe import NBLK, QSET, main as emit, quad_block, quad_round

XH = 60   # v60..v67: hoisted x values (or pre-broadcast W+K words)
F0 = 68   # round 0's F, computed before the burst
RA = 69   # rol30(a) for round 4's x


def dpp(dst: int, w: str, src: str | None, t: int) -> str:
    s = (t >> 2) & 3
    perm = f"quad_perm:[{s},{s},{s},{s}] row_mask:0xf bank_mask:0xf"
    if src is None:
        return f"v_mov_b32_dpp v{dst}, {w} {perm}"
    return f"v_add_u32_dpp v{dst}, {w}, {src} {perm}"


def hoist_block(blk: int, nh: int, wait: int, extra: int = 0, pad: str = "") -> list[str]:
    cur, nxt = QSET[blk % 2], QSET[(blk + 1) % 2]
    slot = (blk + 1) % 2
    st = list(ST)  # slot -> register; slot 0 is renamed to RA when nh == 5

    def regs(t):
        ia = (5 - t % 5) % 5
        return [f"v{st[(ia + i) % 5]}" for i in range(5)]

    def wreg(t):
        return f"v{cur + 4 * (t >> 4) + (t & 3)}"

    def fop(t, dst):
        _, b, c, d, _ = regs(t)
        if t < 20:
            return f"v_bfi_b32 v{dst}, {b}, {c}, {d}"
        return f"v_bitop3_b32 v{dst}, {b}, {c}, {d} bitop3:{'0xe8' if 40 <= t < 60 else '0x96'}"

    a, b, c, d, e = regs(0)
    out = [fop(0, F0), f"v_alignbit_b32 {b}, {b}, {b}, 2"]
    for t, src in zip(range(4), (e, d, c, b)):
        out.append(dpp(XH + t, wreg(t), src, t))
    if nh == 5:
        out += [f"v_alignbit_b32 v{RA}, {a}, {a}, 2", dpp(XH + 4, wreg(4), f"v{RA}", 4)]
    for t in range(nh, nh + extra):
        out.append(dpp(XH + t, wreg(t), None, t))
    # pad: what separates the hoisted DPP adds from the burst, or follows it
    out += {"": [], "c5": [], "movdpp3": [dpp(70 + i, wreg(8 + i), None, 8 + i) for i in range(3)],
            "nop3": ["s_nop 0"] * 3, "nop1": ["s_nop 0"], "n5": [], "vmov3": [f"v_mov_b32 v{70 + i}, {wreg(8 + i)}" for i in range(3)]}[pad]
    out += [f"ds_read_b128 v[{nxt + 4 * q}:{nxt + 4 * q + 3}], v{ADDR} offset:{slot * 5120 + q * 1024}"
            for q in range(5)]
    if pad == "c5":
        out.append("s_waitcnt lgkmcnt(5)")
    if pad == "n5":
        out.append("s_nop 0")
    for t in range(80):
        if t == wait:
            out.append("s_waitcnt lgkmcnt(0)")
        a, b, c, d, e = regs(t)
        out.append(f"v_alignbit_b32 v{R5}, {a}, {a}, 27")
        if t == 0:
            out.append(f"v_add3_u32 {e}, v{R5}, v{F0}, v{XH}")
            continue
        out.append(fop(t, F))
        if t < nh:
            x = XH + t
        else:
            x = X
            out.append(f"v_add_u32 v{X}, {e}, v{XH + t}" if t < nh + extra else dpp(X, wreg(t), e, t))
        out.append(f"v_add3_u32 {e}, v{R5}, v{F}, v{x}")
        if t == 1 and nh == 5:
            st[0] = RA  # b of round 1 is a of round 0: its rol30 is already in RA
        else:
            out.append(f"v_alignbit_b32 {b}, {b}, {b}, 2")
    for i in range(5):
        out.append(f"v_add_u32 v{H[i]}, v{H[i]}, v{st[i]}")
    for i in range(5):
        out.append(f"v_mov_b32 v{ST[i]}, v{H[i]}")
    return out


def aligned_block(blk: int, kind: str) -> list[str]:
    """The shipped order (burst, 80 DPP rounds, feed-forward) with every DPP add
    at the same address parity: no s_waitcnt inside the rounds, the
    lgkmcnt(0) after the feed-forward adds.
      e64   the probe's five state moves as 8-byte VOP3: 6 four-byte
            instructions per block (5 adds + the wait), parity kept
      p2    four-byte moves (11 four-byte instructions per block: every other
            block would flip) and `.p2align 3` in front of round 0
    """
    cur, nxt = QSET[blk % 2], QSET[(blk + 1) % 2]
    slot = (blk + 1) % 2
    out = [f"ds_read_b128 v[{nxt + 4 * q}:{nxt + 4 * q + 3}], v{ADDR} offset:{slot * 5120 + q * 1024}"
           for q in range(5)]
    if kind == "p2":
        out.append(".p2align 3")
    for t in range(80):
        out += quad_round(t, cur, True)
    for i in range(5):
        out.append(f"v_add_u32 v{H[i]}, v{H[i]}, v{ST[i]}")
    out.append("s_waitcnt lgkmcnt(0)")
    for i in range(5):
        out.append(f"v_mov_b32{'' if kind == 'p2' else '_e64'} v{ST[i]}, v{H[i]}")
    return out


def variants():
    out = []
    for kind in ("e64", "p2"):
        body = []
        for blk in range(NBLK):
            body += aligned_block(blk, kind)
        out.append((f"quad_dpp_b5_aligned_{kind}", body, 2 * 5120))
    # the round stream alone (no LDS reads) with every DPP add at the other parity
    body = []
    for blk in range(NBLK):
        body += quad_block(blk, "none", True)
    out.append(("quad_dpp_none_shift4", ["s_nop 0"] + body, 2 * 5120))
    for sched, use_dpp, tag in (("none", True, "dpp"), ("b5w4", True, "dpp"), ("b5", False, "vop2")):
        body = []
        for blk in range(NBLK):
            body += quad_block(blk, sched, use_dpp)
        out.append((f"quad_{tag}_{sched}", body, 2 * 5120))
    for name, nh, wait, extra, pad in (
            ("hoist4", 4, 4, 0, ""), ("hoist4_w2", 4, 2, 0, ""), ("hoist4_w3", 4, 3, 0, ""),
            ("hoist4_w6", 4, 6, 0, ""), ("hoist5", 5, 5, 0, ""), ("hoist5_w4", 5, 4, 0, ""),
            ("hoist5_w6", 5, 6, 0, ""), ("hoist5_w8", 5, 8, 0, ""), ("hoist8", 5, 8, 3, ""),
            ("hoist8_w5", 5, 5, 3, ""), ("hoist5_c5", 5, 5, 0, "c5"), ("hoist5_movdpp3", 5, 5, 0, "movdpp3"),
            ("hoist5_w8_movdpp3", 5, 8, 0, "movdpp3"), ("hoist5_nop3", 5, 5, 0, "nop3"),
            ("hoist5_vmov3", 5, 5, 0, "vmov3"), ("hoist4_vmov3", 4, 4, 0, "vmov3"),
            ("hoist5_c5_w4", 5, 4, 0, "c5"), ("hoist5_c5_w6", 5, 6, 0, "c5"), ("hoist5_c5_w8", 5, 8, 0, "c5"),
            ("hoist4_c5", 4, 4, 0, "c5"), ("hoist4_c5_w6", 4, 6, 0, "c5"), ("hoist8_c5", 5, 8, 3, "c5"),
            ("hoist6", 5, 6, 1, ""), ("hoist7", 5, 7, 2, ""), ("hoist6_c5", 5, 6, 1, "c5"),
            ("hoist7_c5", 5, 7, 2, "c5"), ("hoist5_nop1", 5, 5, 0, "nop1"), ("hoist5_n5", 5, 5, 0, "n5")):
        body = []
        for blk in range(NBLK):
            body += hoist_block(blk, nh, wait, extra, pad)
        out.append((f"quad_dpp_{name}", body, 2 * 5120))
    return out


if __name__ == "__main__":
    emit(variants(), "quad_hoist_probe.hip")
