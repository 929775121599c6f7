#!/usr/bin/env python3
"""Appending to the digest index (sha1chunk_index_append*, include/sha1chunk.h
"Digest index"): k = 1, 64 and 4096 random digests appended to an index of
m = 16384 and 262144 random digests.  Every figure is a median with min-max
over --reps (default 20) repetitions in one run after a warm-up, the compared
paths alternated inside each repetition, each on a fresh index of m digests
(created and reserved outside the timed region).

(a) sha1chunk_index_append_device_async of k device digests, capacity reserved
    (HIP events on torch's current stream: the row copy and the append kernel).
(b) sha1chunk_index_append of k host digests, capacity reserved (wall clock:
    the call is synchronous -- rows up, kernel, wait).
(c) the same without a reserve: the call that grows the index (wall clock:
    device wait, two allocations, row copy, rehash, wait, two frees included).
(d) the parent commit's only way to the same set: sha1chunk_index_destroy plus
    sha1chunk_index_create over all m + k digests from device memory (wall
    clock).

After the warm-up rounds every index is checked: all m + k digests at their
positions.

  python tools/index_append_bench.py [--out profiles/index_append.jsonl]
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
    ap.add_argument("--appends", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_append.jsonl"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("congestion-control-with-bittorren_amd")
    torch.cuda.set_device(0)
    pkg.set_device(0)
    rng = np.random.default_rng(12)
    lines = []

    for m in a.sizes:
        for k in a.appends:
            both = rng.integers(0, 256, (m + k, 20), dtype=np.uint8)
            new = np.ascontiguousarray(both[m:])
            d_both = torch.from_numpy(both).cuda()
            d_table, d_new = d_both[:m], d_both[m:]
            want = np.arange(m + k, dtype=np.uint32)
            torch.cuda.synchronize()

            def fresh(reserve):
                ix = pkg.DigestIndex(d_table, m)
                if reserve:
                    ix.reserve(m + k)
                return ix

            t_async, t_host, t_grow, t_create = [], [], [], []
            old = pkg.DigestIndex(d_table, m)  # what the parent commit destroys
            for rep in range(-2, a.reps):  # two warm-up rounds
                ix_a, ix_h, ix_g = fresh(True), fresh(True), fresh(False)
                ta = timed(torch, lambda: ix_a.append_device(d_new, k))
                th = wall(torch, lambda: ix_h.append(new))
                tg = wall(torch, lambda: ix_g.append(new))
                holder = []

                def recreate():
                    old.close()
                    holder.append(pkg.DigestIndex(d_both, m + k))
                tc = wall(torch, recreate)
                if rep < 0:
                    for ix in (ix_a, ix_h, ix_g, holder[0]):
                        assert ix.size == m + k and np.array_equal(ix.lookup(both), want)
                    assert ix_g.capacity >= max(2 * m, m + k) and ix_a.capacity == ix_h.capacity == m + k
                for ix in (ix_a, ix_h, ix_g):
                    ix.close()
                old = holder[0]
                if rep >= 0:
                    t_async.append(ta)
                    t_host.append(th)
                    t_grow.append(tg)
                    t_create.append(tc)
            old.close()
            lines.append({"bench": "index_append", "m": m, "k": k, "reps": a.reps, "unit": "ms",
                          "append_device_async_events": spread(t_async), "append_host_wall": spread(t_host),
                          "append_host_growing_wall": spread(t_grow),
                          "destroy_plus_create_device_wall": spread(t_create)})
            print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
