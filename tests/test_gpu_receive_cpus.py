"""sha1chunk_receive_cpus (include/sha1chunk.h): the CPUs a verify queue's
receive thread should run on -- one L3 domain of the GPU's NUMA node per
receive thread ("Verify queue placement").  Checked
against the box's own sysfs: the domains partition the node's allowed CPUs,
each is exactly a shared_cpu_list (within the allowed node CPUs), slots wrap
round robin, and SHA1CHUNK_NUMA=off widens them to every allowed CPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpulist(text):
    out = set()
    for piece in text.strip().split(","):
        if not piece:
            continue
        a, _, b = piece.partition("-")
        out.update(range(int(a), int(b or a) + 1))
    return out


def _read(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError:
        return ""


def _node_cpus(bdf):
    node = _read(f"/sys/bus/pci/devices/{bdf.lower()}/numa_node").strip()
    if not node or int(node) < 0:
        return None
    return _cpulist(_read(f"/sys/devices/system/node/node{int(node)}/cpulist"))


@pytest.fixture(scope="module", autouse=True)
def dev(pkg):
    # torch's HIP runtime first, as every GPU test module does: the library's
    # backend then shares the process's already-loaded runtime
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    pkg.set_device(0)
    return torch


def _domains(pkg, dev):
    first, n = pkg.sha1chunk.receive_cpus(dev, 0)
    return [pkg.sha1chunk.receive_cpus(dev, s)[0] for s in range(n)], n, first


def test_receive_cpus_partition_the_node(pkg):
    dev = 0
    doms, n, first = _domains(pkg, dev)
    assert n >= 1 and all(doms)
    allowed = os.sched_getaffinity(0)
    node = _node_cpus(pkg.sha1chunk.device_pci_bus_id(dev))
    base = allowed & node if node and allowed & node else allowed
    union = set()
    for d in doms:
        assert not union & set(d), "domains overlap"
        union |= set(d)
        # exactly its first CPU's L3 list (where sysfs has one), within base
        l3 = _read(f"/sys/devices/system/cpu/cpu{d[0]}/cache/index3/shared_cpu_list")
        if l3:
            assert set(d) == _cpulist(l3) & (base - (union - set(d)))
    assert union == base
    # round robin: slot n is slot 0 again; the domain count comes back each time
    again, n2 = pkg.sha1chunk.receive_cpus(dev, n)
    assert again == first and n2 == n
    assert pkg.sha1chunk.receive_cpus(dev, 2 * n + 1)[0] == doms[1 % n]


def test_receive_cpus_rejects_a_bad_device(pkg):
    with pytest.raises(pkg.Sha1ChunkError) as ei:
        pkg.sha1chunk.receive_cpus(pkg.sha1chunk.device_count() + 3, 0)
    assert ei.value.code == pkg.sha1chunk.EINVAL


def test_receive_cpus_numa_off_uses_every_allowed_cpu():
    """SHA1CHUNK_NUMA=off (read once per process): the domains of the whole
    affinity mask."""
    code = (
        "import json, os, sys; sys.path.insert(0, %r)\n"
        "import torch; assert torch.cuda.is_available()\n"
        "import importlib; pkg = importlib.import_module('congestion-control-with-bittorren_amd')\n"
        "first, n = pkg.sha1chunk.receive_cpus(0, 0)\n"
        "u = set()\n"
        "for s in range(n): u |= set(pkg.sha1chunk.receive_cpus(0, s)[0])\n"
        "print(json.dumps({'n': n, 'union': sorted(u), 'allowed': sorted(os.sched_getaffinity(0))}))\n"
    ) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, SHA1CHUNK_NUMA="off"))
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["union"] == out["allowed"]


# ---- placement is the process's, whichever thread asks first ---
# near_cpus() and receive_domains() are cached once per process, so each case
# runs in a child process and is compared with a control child in which no
# thread is pinned: what the right answer is depends on the box.
_CHILD_HEAD = r"""
import hashlib, importlib, json, os, sys, threading
import numpy as np
sys.path.insert(0, sys.argv[1])
PIN = sys.argv[2] == "pinned"
import torch
assert torch.cuda.is_available()
pkg = importlib.import_module("congestion-control-with-bittorren_amd")
pkg.lib()
out = {"allowed": sorted(os.sched_getaffinity(0))}

def in_thread(fn):
    # fn on a thread of its own, pinned to one allowed CPU when asked
    res = {}
    def run():
        try:
            if PIN:
                os.sched_setaffinity(0, {max(os.sched_getaffinity(0))})
            res["mask"] = sorted(os.sched_getaffinity(0))
            res["value"] = fn()
        except BaseException as e:
            res["error"] = repr(e)
    t = threading.Thread(target=run)
    t.start()
    t.join(timeout=60)
    assert "error" not in res and "value" in res, res
    return res
"""

_FIRST_CALL_CHILD = _CHILD_HEAD + r"""
# the process's first library call: from the (pinned) thread
res = in_thread(lambda: pkg.sha1chunk.receive_cpus(0, 0))
out["thread_mask"] = res["mask"]
out["thread_first"], out["thread_n"] = res["value"]
first, n = pkg.sha1chunk.receive_cpus(0, 0)  # then the unpinned main thread, every slot
out["n"] = n
out["slots"] = [pkg.sha1chunk.receive_cpus(0, s)[0] for s in range(n)]
assert out["slots"][0] == first
out["main_mask"] = sorted(os.sched_getaffinity(0))
print(json.dumps(out))
"""

_POOL_CHILD = _CHILD_HEAD + r"""
# the device comes up on the unpinned main thread, by a path that makes no pool
pkg.set_device(0)
buf = torch.arange(4096, dtype=torch.uint8, device="cuda")
off = torch.tensor([0, 1024], dtype=torch.int64, device="cuda")
ln = torch.tensor([1000, 3072], dtype=torch.int32, device="cuda")
dig = torch.zeros((2, 20), dtype=torch.uint8, device="cuda")
pkg.hash_batch_device(buf, off, ln, dig)
host = buf.cpu().numpy().tobytes()
assert dig.cpu().numpy().tobytes() == hashlib.sha1(host[:1000]).digest() + hashlib.sha1(host[1024:]).digest()

def pools():
    found = []
    for tid in os.listdir("/proc/self/task"):
        try:
            if open(f"/proc/self/task/{tid}/comm").read().strip() != "s1pool":
                continue
            for line in open(f"/proc/self/task/{tid}/status"):
                if line.startswith("Cpus_allowed_list:"):
                    found.append(line.split(":", 1)[1].strip())
        except OSError:
            pass
    return sorted(found)

assert pools() == [], pools()
# a small ragged pageable batch: unaligned, so packed by the device's pack pool
rng = np.random.default_rng(9)
lens = [1, 63, 64, 65, 1000, 4097, 70001]
offs, at = [], 3
for n in lens:
    offs.append(at)
    at += n + 5
base = rng.integers(0, 256, at, dtype=np.uint8)
res = in_thread(lambda: pkg.hash_batch(base, offs, lens).tobytes())
want = b"".join(hashlib.sha1(base[o:o + n].tobytes()).digest() for o, n in zip(offs, lens))
out["digests_ok"] = res["value"] == want
out["thread_mask"] = res["mask"]
out["pools"] = pools()
print(json.dumps(out))
"""


def _children(code, **env):
    """The control child and the one with the pinned thread, side by side
    (a process's start is most of each): their JSON results."""
    hows = ("unpinned", "pinned")
    ps = [subprocess.Popen([sys.executable, "-c", code, ROOT, how], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, env=dict(os.environ, **env)) for how in hows]
    outs = []
    try:
        for how, p in zip(hows, ps):
            stdout, stderr = p.communicate(timeout=120)
            assert p.returncode == 0, (how, stdout[-1000:], stderr[-2000:])
            outs.append(json.loads(stdout.strip().splitlines()[-1]))
    finally:
        for p in ps:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return outs


def _needs_two_cpus():
    if len(os.sched_getaffinity(0)) < 2:
        pytest.skip("a pinned thread is no different from the process with fewer than 2 allowed CPUs")


def test_receive_cpus_first_call_from_a_pinned_thread():
    """A receive thread that has pinned itself to one CPU -- as
    sha1chunk_receive_cpus tells callers to -- and then makes the process's
    first library call must not shrink the cached placement to its own mask:
    its answer, and every slot the unpinned main thread asks for afterwards,
    equal those of a process in which nobody was pinned."""
    _needs_two_cpus()
    control, test = _children(_FIRST_CALL_CHILD)
    print(f"{control['n']} domains; pinned thread's mask {test['thread_mask']}, its slot 0 {test['thread_first']}")
    assert control["allowed"] == test["allowed"] == control["thread_mask"] == test["main_mask"]
    assert len(test["thread_mask"]) == 1 and len(test["allowed"]) >= 2
    assert control["n"] >= 1 and all(control["slots"])
    assert control["thread_first"] == control["slots"][0] and control["thread_n"] == control["n"]
    assert (test["n"], test["slots"]) == (control["n"], control["slots"])
    assert (test["thread_n"], test["thread_first"]) == (control["n"], control["slots"][0])


def test_pool_helpers_do_not_inherit_a_pinned_caller():
    """The pack pool's helper threads (named s1pool) are created by whichever
    thread first hashes a pageable batch.  Created by a thread pinned to one
    CPU they must run where they run when an unpinned thread creates them:
    on the GPU's node's CPUs, or on the process's, never on the creator's one
    CPU.  SHA1CHUNK_COPY_THREADS=4: the caller and three helpers."""
    _needs_two_cpus()
    control, test = _children(_POOL_CHILD, SHA1CHUNK_COPY_THREADS="4")
    print(f"pinned creator {test['thread_mask']}; helpers {test['pools']} (control {control['pools']})")
    assert control["digests_ok"] and test["digests_ok"]
    assert len(test["thread_mask"]) == 1 and control["thread_mask"] == control["allowed"] == test["allowed"]
    assert len(control["pools"]) == 3 and len(test["pools"]) == 3
    assert len(set(control["pools"])) == 1 and set(test["pools"]) == set(control["pools"])
    assert _cpulist(control["pools"][0]) <= set(control["allowed"]) and len(_cpulist(control["pools"][0])) >= 2
