#!/usr/bin/env python3
"""Hashing messages given as segment lists (sha1chunk_gather_device_async,
sha1chunk_hash_gather_batch, sha1chunk_verify_gather_batch): N chunks (default
4096) of 512 KiB in the packet shape -- 354 segments each, 353 x 1484 B + 436 B
at offset 16 of 1500-byte slots, the slots of the whole ring permuted by a
seeded shuffle.  Every figure is a median with min-max over --reps (>= 7)
repetitions in one run, the compared paths alternated inside each repetition.

(a) device-resident (HIP events on torch's current stream): the gather alone,
    the gather followed by the hash of the reassembled bytes
    (sha1chunk_hash_device_async, offset / length arrays), that hash alone,
    and sha1chunk_hash_uniform_async on the same bytes laid contiguously.
    The overhead of gather + hash over the uniform hash is the figure to
    report.  Also the synchronous sha1chunk_hash_gather_batch(DEVICE) as the
    host sees it (wall clock: its array upload and the wait included).
(b) from sha1chunk_pinned_alloc memory read in place: the gather alone (HIP
    events) beside hipMemcpyAsync H2D of the same byte count from the same
    memory; sha1chunk_verify_gather_batch against sha1chunk_verify_batch from
    pinned contiguous memory (wall clock).
(c) the pageable path: sha1chunk_hash_gather_batch from an ordinary host
    array (wall clock).

Every digest is checked against the uniform hash's.

  python tools/gather_bench.py [--out profiles/gather.jsonl]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK, BODY, NPACK, SLOT, HEADER = 524288, 1484, 354, 1500, 16
LAST = CHUNK - (NPACK - 1) * BODY
GIB = float(1 << 30)


def timed(torch, fn) -> float:
    """Milliseconds of what fn enqueues on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(torch, fn) -> float:
    """Milliseconds of a synchronous call."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def spread(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits),
            "max": round(max(xs), digits)}


def rate(nbytes, ms_spread):
    """GiB/s for a spread of milliseconds (the slowest time is the min rate)."""
    return {"median": round(nbytes / GIB / ms_spread["median"] * 1e3, 2),
            "min": round(nbytes / GIB / ms_spread["max"] * 1e3, 2),
            "max": round(nbytes / GIB / ms_spread["min"] * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather.jsonl"))
    a = ap.parse_args()
    assert a.reps >= 7, "at least 7 repetitions"
    import torch
    pkg = importlib.import_module("congestion-control-with-bittorren_amd")
    S = pkg.sha1chunk
    torch.cuda.set_device(0)
    pkg.set_device(0)
    n, nslots = a.chunks, a.chunks * NPACK
    nbytes = n * CHUNK

    # the chunks laid contiguously, and the same bytes as packets in a permuted ring
    contig = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    pkg.synth_fill_device(contig, 0, n, CHUNK)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    slot_of = torch.randperm(nslots, device="cuda", generator=gen).view(n, NPACK)
    ring = torch.zeros(nslots * SLOT, dtype=torch.uint8, device="cuda")
    ring2 = ring.view(nslots, SLOT)
    rows2 = contig.view(n, CHUNK)
    ring2[slot_of[:, :NPACK - 1].reshape(-1), HEADER:HEADER + BODY] = \
        rows2[:, :(NPACK - 1) * BODY].reshape(n * (NPACK - 1), BODY)
    ring2[slot_of[:, NPACK - 1], HEADER:HEADER + LAST] = rows2[:, (NPACK - 1) * BODY:]
    seg_off = (slot_of.to(torch.int64) * SLOT + HEADER).reshape(-1).contiguous()
    seg_len = torch.full((n, NPACK), BODY, dtype=torch.int32, device="cuda")
    seg_len[:, -1] = LAST
    seg_len = seg_len.reshape(-1).contiguous()
    seg_first = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * NPACK).to(torch.int32)
    csr = (seg_off.cpu().numpy().view(np.uint64), seg_len.cpu().numpy().view(np.uint32),
           seg_first.cpu().numpy().view(np.uint32))
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst_off = torch.arange(n, dtype=torch.int64, device="cuda") * CHUNK
    out_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    base_dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    new_dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def gather(src):
        S.gather_device(src, seg_off, seg_len, seg_first, dst, dst_off, out_lengths=out_len)

    # ---- (a) device-resident ----------------------------------------------
    pkg.hash_uniform_device(contig, CHUNK, n, base_dig)  # warm-up of every path
    gather(ring)
    S.hash_device(dst, dst_off, out_len, new_dig)
    torch.cuda.synchronize()
    assert torch.equal(dst, contig), "the gather does not reassemble the chunks"
    assert torch.equal(base_dig, new_dig), "gather + hash differs from sha1chunk_hash_uniform_async"
    want = base_dig.cpu().numpy()
    assert np.array_equal(S.hash_gather(ring, csr), want)
    t_uni, t_gather, t_both, t_arrays, t_sync = [], [], [], [], []
    for _ in range(a.reps):
        t_uni.append(timed(torch, lambda: pkg.hash_uniform_device(contig, CHUNK, n, base_dig)))
        t_gather.append(timed(torch, lambda: gather(ring)))
        t_both.append(timed(torch, lambda: (gather(ring), S.hash_device(dst, dst_off, out_len, new_dig))))
        t_arrays.append(timed(torch, lambda: S.hash_device(dst, dst_off, out_len, new_dig)))
        t_sync.append(wall(torch, lambda: S.hash_gather(ring, csr)))
    assert torch.equal(base_dig, new_dig)
    g = spread(t_gather)
    emit({"run": "a_device", "chunks": n, "segments": nslots, "reps": a.reps, "hash_uniform_ms": spread(t_uni),
          "gather_ms": g, "gather_gib_per_s": rate(nbytes, g), "gather_then_hash_ms": spread(t_both),
          "hash_arrays_ms": spread(t_arrays),
          "overhead_over_uniform_ms": round(statistics.median(t_both) - statistics.median(t_uni), 3),
          "hash_gather_batch_device_wall_ms": spread(t_sync)})

    # ---- (b) pinned memory read in place -----------------------------------
    pinned = S.pinned_alloc(ring.numel())
    pinned_t = torch.from_numpy(pinned)
    pinned_t.copy_(ring)
    contig_pin = S.pinned_alloc(nbytes)
    torch.from_numpy(contig_pin).copy_(contig)
    torch.cuda.synchronize()
    offsets = np.arange(n, dtype=np.uint64) * CHUNK
    lengths = np.full(n, CHUNK, np.uint32)
    gather(pinned)  # warm-up
    torch.cuda.synchronize()
    assert torch.equal(dst, contig), "the gather from pinned memory does not reassemble the chunks"
    assert not S.verify_gather(pinned, csr, want).any() and not S.verify_batch(contig_pin, offsets, lengths, want).any()
    h2d_src = pinned_t[:nbytes]
    t_pg, t_h2d, t_vg, t_vb = [], [], [], []
    for _ in range(a.reps):
        t_h2d.append(timed(torch, lambda: dst.copy_(h2d_src, non_blocking=True)))
        t_pg.append(timed(torch, lambda: gather(pinned)))
        t_vb.append(wall(torch, lambda: S.verify_batch(contig_pin, offsets, lengths, want)))
        t_vg.append(wall(torch, lambda: S.verify_gather(pinned, csr, want)))
    torch.cuda.synchronize()
    assert torch.equal(dst, contig)
    pg, h2d = spread(t_pg), spread(t_h2d)
    emit({"run": "b_pinned", "chunks": n, "segments": nslots, "reps": a.reps, "gather_ms": pg,
          "gather_gib_per_s": rate(nbytes, pg), "h2d_same_bytes_ms": h2d, "h2d_gib_per_s": rate(nbytes, h2d),
          "gather_over_h2d": round(statistics.median(t_h2d) / statistics.median(t_pg), 3),
          "verify_gather_wall_ms": spread(t_vg), "verify_batch_pinned_contiguous_wall_ms": spread(t_vb)})

    # ---- (c) the pageable path ----------------------------------------------
    pageable = np.array(pinned, copy=True)
    S.pinned_free(pinned)
    S.pinned_free(contig_pin)
    assert np.array_equal(S.hash_gather(pageable, csr), want)
    t_pp = [wall(torch, lambda: S.hash_gather(pageable, csr)) for _ in range(a.reps)]
    pp = spread(t_pp)
    emit({"run": "c_pageable", "chunks": n, "segments": nslots, "reps": a.reps, "hash_gather_wall_ms": pp,
          "gib_per_s": rate(nbytes, pp)})

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
