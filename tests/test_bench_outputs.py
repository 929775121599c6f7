"""bench.py's plain run and --dump-outputs: a plain run carries the headline
figure and nothing of the --full legs, and the dumped digests are the timed
path's own output (float32, golden-checked, the same from run to run)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("parity", "strong", "weak_config4", "config4_shard8", "config4_shard2", "strong_projection",
             "config5", "config3_e2e", "config1", "verify_queue", "file", "master_verify",
             "latency_one_chunk", "cpu_baseline")


def test_dump_outputs_float32_capped_and_seeded(tmp_path, monkeypatch):
    import torch

    import bench
    rng = np.random.default_rng(1)
    digs = [torch.from_numpy(rng.integers(0, 256, (300, 20), dtype=np.uint8)) for _ in range(2)]
    want = np.concatenate([d.numpy() for d in digs])
    bench._dump_outputs(str(tmp_path / "a"), digs, None)
    got = np.load(tmp_path / "a" / "digests.npy")
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # above the cap: a sample of whole rows in index order, the same every time
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096 + 100 * 80)
    bench._dump_outputs(str(tmp_path / "b"), digs, 3)
    bench._dump_outputs(str(tmp_path / "c"), digs, 3)
    b = np.load(tmp_path / "b" / "digests_rank3.npy")
    assert b.shape == (100, 20) and os.path.getsize(tmp_path / "b" / "digests_rank3.npy") <= 4096 + 100 * 80
    assert np.array_equal(b, np.load(tmp_path / "c" / "digests_rank3.npy"))
    rows = {r.tobytes(): i for i, r in enumerate(want.astype(np.float32))}
    idx = [rows[r.tobytes()] for r in b]
    assert idx == sorted(idx) and len(set(idx)) == 100


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_digests(tmp_path, golden):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "GiB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u32" and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(4096 * 524288 / 2**30 / (d["ms_per_step"] / 1e3), rel=1e-3)
    assert d["roofline"]["frac"] > 0
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(out)) == ["digests.npy"]
    got = np.load(out / "digests.npy")
    assert got.dtype == np.float32 and got.shape == (4096, 20)
    assert hashlib.sha1(got.astype(np.uint8).tobytes()).hexdigest() == golden["weak4096"][0]
