#!/usr/bin/env python3
"""Batched SHA1Update / SHA1Final over arrays of SHA1Context
(sha1chunk_update_device_async and its siblings), device-resident, timed with
HIP events on torch's current stream.

(a) bulk parity: N contexts (default 4096), each fed its whole 512 KiB in one
    update from a fresh context, then final -- against
    sha1chunk_hash_uniform_async on the same bytes in the same run, runs
    alternated.  Also timed: the update call's own kernels with nothing to
    hash (every piece of length 0: pre, the sort, an empty bulk launch, post)
    and final alone.  The new path's time should exceed the baseline's by no
    more than those plus the baseline's min-max spread; the line says whether
    it did (`within`).
(b) cost of a call: 64, 256 and 4096 contexts fed 1484-byte pieces, one call
    per round, every round enqueued back to back: us per call and aggregate
    MB/s, beside the sha1chunk_burst_advance figures of
    profiles/pv_shared.jsonl (one burst per round, `auto`) for orientation.

Every digest is checked: (a) against the baseline's, (b) a sample with hashlib.

  python tools/update_batch_bench.py [--out profiles/update_batch.jsonl]
"""
from __future__ import annotations

import argparse
import hashlib
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 524288
PACKET = 1484


def timed(torch, fn) -> float:
    """Milliseconds of what fn enqueues on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def pv_burst_figures():
    """Aggregate MB/s of sha1chunk_burst_advance, one burst per round, kernel
    auto, by session count (profiles/pv_shared.jsonl)."""
    out = {}
    path = os.path.join(ROOT, "profiles", "pv_shared.jsonl")
    if not os.path.exists(path):
        return out
    by = {}
    for line in open(path):
        try:
            d = json.loads(line)
        except ValueError:
            continue
        if d.get("run") == "C" and d.get("feed") == "burst" and d.get("kernel") == "auto":
            by.setdefault(d["sessions"], []).append(d["bytes_per_s"] / 1e6)
    for s, xs in sorted(by.items()):
        out[str(s)] = {k: round(v) for k, v in spread(xs).items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_batch.jsonl"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("congestion-control-with-bittorren_amd")
    S = pkg.sha1chunk
    torch.cuda.set_device(0)
    pkg.set_device(0)
    n = a.contexts
    buf = torch.empty(n * CHUNK, dtype=torch.uint8, device="cuda")
    pkg.synth_fill_device(buf, 0, n, CHUNK)
    ctx = torch.zeros(n * S.CONTEXT_BYTES, dtype=torch.uint8, device="cuda")
    off = torch.arange(n, dtype=torch.int64, device="cuda") * CHUNK
    whole = torch.full((n,), CHUNK, dtype=torch.int32, device="cuda")
    empty = torch.zeros(n, dtype=torch.int32, device="cuda")
    base_dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    new_dig = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    rows = []

    # ---- (a) bulk parity -------------------------------------------------
    def new_path():
        S.update_contexts_device(ctx, buf, off, whole)
        S.final_contexts_device(ctx, new_dig)

    pkg.hash_uniform_device(buf, CHUNK, n, base_dig)  # warm-up of both paths
    S.init_contexts_device(ctx)
    new_path()
    torch.cuda.synchronize()
    assert torch.equal(base_dig, new_dig), "update + final differs from sha1chunk_hash_uniform_async"
    t_base, t_new, t_empty, t_final = [], [], [], []
    for _ in range(a.reps):
        t_base.append(timed(torch, lambda: pkg.hash_uniform_device(buf, CHUNK, n, base_dig)))
        S.init_contexts_device(ctx)
        t_new.append(timed(torch, new_path))
        assert torch.equal(base_dig, new_dig)
        S.init_contexts_device(ctx)
        t_empty.append(timed(torch, lambda: S.update_contexts_device(ctx, buf, off, empty)))
        t_final.append(timed(torch, lambda: S.final_contexts_device(ctx, new_dig)))
    extra = statistics.median(t_empty) + statistics.median(t_final)
    allowed = statistics.median(t_base) + extra + (max(t_base) - min(t_base))
    rows.append({"run": "a_bulk_parity", "contexts": n, "piece_bytes": CHUNK, "reps": a.reps,
                 "hash_uniform_ms": spread(t_base), "update_final_ms": spread(t_new),
                 "update_of_empty_pieces_ms": spread(t_empty), "final_alone_ms": spread(t_final),
                 "excess_ms": round(statistics.median(t_new) - statistics.median(t_base), 4),
                 "allowed_excess_ms": round(allowed - statistics.median(t_base), 4),
                 "within": statistics.median(t_new) <= allowed,
                 "gb_per_s": {"hash_uniform": round(n * CHUNK / statistics.median(t_base) / 1e6, 1),
                              "update_final": round(n * CHUNK / statistics.median(t_new) / 1e6, 1)}})
    print(json.dumps(rows[-1]), flush=True)

    # ---- (b) cost of a call ------------------------------------------------
    pv = pv_burst_figures()
    for m in (64, 256, 4096):
        if m > n:
            continue
        rounds = min(a.rounds, CHUNK // PACKET)
        offs = [torch.arange(m, dtype=torch.int64, device="cuda") * CHUNK + r * PACKET for r in range(rounds)]
        lens = torch.full((m,), PACKET, dtype=torch.int32, device="cuda")
        sub = ctx[: m * S.CONTEXT_BYTES]
        dig = torch.zeros((m, 20), dtype=torch.uint8, device="cuda")
        per_call, rate = [], []
        for _ in range(a.reps):
            S.init_contexts_device(sub)
            torch.cuda.synchronize()

            def feed():
                for r in range(rounds):
                    S.update_contexts_device(sub, buf, offs[r], lens)

            ms = timed(torch, feed)
            per_call.append(ms * 1e3 / rounds)
            rate.append(m * PACKET * rounds / ms / 1e3)
        S.final_contexts_device(sub, dig)
        torch.cuda.synchronize()
        got = dig.cpu().numpy()
        for i in sorted({0, 1, m // 2, m - 1}):
            msg = buf[i * CHUNK: i * CHUNK + rounds * PACKET].cpu().numpy().tobytes()
            assert got[i].tobytes() == hashlib.sha1(msg).digest(), f"context {i} of {m}"
        rows.append({"run": "b_call_cost", "contexts": m, "piece_bytes": PACKET, "rounds": rounds, "reps": a.reps,
                     "us_per_call": spread(per_call), "mb_per_s": {k: round(v) for k, v in spread(rate).items()},
                     "pv_burst_advance_mb_per_s": pv.get(str(m))})
        print(json.dumps(rows[-1]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
