#!/usr/bin/env python3
"""The digest index (sha1chunk_index_*, include/sha1chunk.h "Digest index") at
m = n = 16384 and 262144 random digests, every query a hit in shuffled order.
Every figure is a median with min-max over --reps (default 20) repetitions in
one run after a warm-up, the compared paths alternated inside each repetition.

(a) sha1chunk_index_create from device memory (wall clock: the call is
    synchronous -- table copy, build kernel and wait included), with the build's
    counters, beside building a Python dict from the same digests on the host.
(b) the lookup kernel alone (HIP events on torch's current stream) beside the
    parent commit's way to the same answer: the digests copied to the host and
    matched in that Python dict (wall clock, the D2H copy included); and
    sha1chunk_index_lookup from host arrays (wall clock).
(c) 4096 x 512 KiB (config 2): sha1chunk_hash_uniform_async alone, followed by
    the lookup, and followed by sha1chunk_compare_device_async (what a verify
    queues behind the hash), all HIP events.

Every answer is checked against the dict.

  python tools/index_bench.py [--out profiles/index.jsonl]
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
CHUNK = 524288


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


def spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits),
            "max": round(max(xs), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 262144])
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index.jsonl"))
    a = ap.parse_args()
    import ctypes as C

    import torch
    pkg = importlib.import_module("congestion-control-with-bittorren_amd")
    S = pkg.sha1chunk
    torch.cuda.set_device(0)
    pkg.set_device(0)
    be = C.CDLL(os.path.join(os.path.dirname(S.LIB_PATH), "libsha1chunk_hip.so"))
    be.s1be_index_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    rng = np.random.default_rng(11)
    lines = []

    for m in a.sizes:
        table = rng.integers(0, 256, (m, 20), dtype=np.uint8)
        perm = rng.permutation(m)
        queries = np.ascontiguousarray(table[perm])
        d_table = torch.from_numpy(table).cuda()
        d_q = torch.from_numpy(queries).cuda()
        d_ids = torch.zeros(m, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def make_dict():
            return {row: p for p, row in enumerate(table.view("V20").reshape(-1).tolist())}

        def via_host(d):
            rows = d_q.cpu().numpy().view("V20").reshape(-1).tolist()
            return [d[r] for r in rows]

        d = make_dict()
        t_create, t_dict, t_lookup, t_host_dict, t_host_form = [], [], [], [], []
        stats = None
        ix = pkg.DigestIndex(d_table)
        for rep in range(-2, a.reps):  # two warm-up rounds
            holder = []
            tc = wall(torch, lambda: holder.append(pkg.DigestIndex(d_table)))
            out = (C.c_uint64 * 4)()
            be.s1be_index_stats(holder[0]._ix, out)
            stats = list(out)
            holder[0].close()
            td = wall(torch, make_dict)
            tl = timed(torch, lambda: ix.lookup_device(d_q, d_ids))
            got = []
            th = wall(torch, lambda: got.append(via_host(d)))
            host_ids = []
            tf = wall(torch, lambda: host_ids.append(ix.lookup(queries)))
            if rep < 0:
                assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), perm.astype(np.uint32))
                assert got[0] == perm.tolist() and np.array_equal(host_ids[0], perm.astype(np.uint32))
                continue
            t_create.append(tc)
            t_dict.append(td)
            t_lookup.append(tl)
            t_host_dict.append(th)
            t_host_form.append(tf)
        ix.close()
        lines.append({"bench": "index", "m": m, "n": m, "reps": a.reps, "unit": "ms",
                      "create_device_wall": spread(t_create), "python_dict_build_wall": spread(t_dict),
                      "lookup_kernel_events": spread(t_lookup), "d2h_plus_python_dict_wall": spread(t_host_dict),
                      "lookup_host_form_wall": spread(t_host_form),
                      "build_stats": {"slots": stats[0], "longest_probe": stats[1], "duplicates": stats[2],
                                      "wrapped": stats[3]}})
        print(json.dumps(lines[-1]), flush=True)

    # (c) behind a config-2 hash
    n = a.chunks
    buf = torch.empty(n * CHUNK, dtype=torch.uint8, device="cuda")
    dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    mis = torch.zeros(n, dtype=torch.uint8, device="cuda")
    pkg.synth_fill_device(buf, 0, n, CHUNK)
    pkg.hash_uniform_device(buf, CHUNK, n, dig)
    torch.cuda.synchronize()
    want = dig.cpu().numpy()
    perm = rng.permutation(n)
    expected = dig.clone()
    t_hash, t_hash_lookup, t_hash_compare = [], [], []
    with pkg.DigestIndex(want[perm]) as ix:
        def hash_only():
            pkg.hash_uniform_device(buf, CHUNK, n, dig)

        def hash_lookup():
            pkg.hash_uniform_device(buf, CHUNK, n, dig)
            ix.lookup_device(dig, ids)

        def hash_compare():
            pkg.hash_uniform_device(buf, CHUNK, n, dig)
            S.compare_device(dig, expected, mis)

        for rep in range(-2, a.reps):
            x, y, z = timed(torch, hash_only), timed(torch, hash_lookup), timed(torch, hash_compare)
            if rep < 0:
                assert np.array_equal(ids.cpu().numpy().view(np.uint32), np.argsort(perm).astype(np.uint32))
                assert not mis.cpu().numpy().any()
                continue
            t_hash.append(x)
            t_hash_lookup.append(y)
            t_hash_compare.append(z)
    lines.append({"bench": "index_behind_hash", "chunks": n, "chunk_len": CHUNK, "m": n, "reps": a.reps, "unit": "ms",
                  "hash_uniform_events": spread(t_hash), "hash_then_lookup_events": spread(t_hash_lookup),
                  "hash_then_compare_events": spread(t_hash_compare),
                  "lookup_over_hash": round(statistics.median(t_hash_lookup) - statistics.median(t_hash), 4),
                  "compare_over_hash": round(statistics.median(t_hash_compare) - statistics.median(t_hash), 4)})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
