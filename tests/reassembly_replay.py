"""Python replay of oracle/reassembly_driver.c's packet schedule, and the
checks its two test modules share (test_reassembly_cpu.py,
test_gpu_reassembly.py).

The driver hands the reference's reliable_udp.c the packets of each (chunk,
attempt) in an order that is a pure function of the chunk's seed and the
attempt.  replay_attempt() restates that order -- pick() below is the driver's
pick() -- and the reference's window bookkeeping (cumulative_ack,
copy_recv_packet_2_buf: a copy only for an in-window packet whose flag is
clear, the window sliding past every leading received packet), and so yields
the session buffer the driver must end up with, 0xA5 wherever no packet
landed.  Every expected value in the tests comes from here, from hashlib and
from the data file; none from the library."""
from __future__ import annotations

import hashlib
import os
import subprocess
from dataclasses import dataclass, field

CHUNK_LEN = 524288
BODY = 1484
NPACK = 354
LAST_BODY = CHUNK_LEN - (NPACK - 1) * BODY
WINDOW = 8
M64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "dropin", "reassembly_driver")
REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "reassembly_ref")
PV_MODES = ("pv", "pv-burst")

# absolute chunk positions every mode corrupts at least once (one-bit flips)
EDGE_OFFSETS = (0, 1483, 1484, 1535, 1536, 176 * BODY + 700, 523851, 523852, 524287)


@dataclass
class Chunk:
    seed: int
    early: bool = False
    corr: list = field(default_factory=list)  # (seqNo, offset in body, xor mask, "F" | "D")


@dataclass
class Scenario:
    sessions: int
    chunks: list
    gseed: int = 1
    subset: int = 70    # % of the open sessions served per round
    reorder: int = 100  # % of packets picked anywhere in the window, not in order
    dup: int = 100      # % of the picks of an already received packet that stay duplicates
    stray: int = 3      # % of packets outside the window
    sync: int = 15      # % of the advances after which the driver lets the device catch up

    def text(self) -> str:
        lines = [f"{self.sessions} {self.gseed} {self.subset} {self.reorder} {self.dup} {self.stray} {self.sync}"]
        for c in self.chunks:
            lines.append(" ".join([str(c.seed), str(int(c.early)), str(len(c.corr))] +
                                  [f"{s} {o} {m} {k}" for s, o, m, k in c.corr]))
        return "\n".join(lines) + "\n"


def at(pos: int, mask: int = 0x04, kind: str = "F"):
    """A corruption at absolute chunk position pos."""
    return (pos // BODY + 1, pos % BODY, mask, kind)


class _Lcg:
    def __init__(self, x):
        self.x = x & M64

    def next(self):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & M64
        return self.x >> 33


@dataclass
class Attempt:
    buf: bytes
    acked: int          # last_packet_acked when the short packet ended the session
    delivered: int
    dup_copies: dict    # seqNo -> deliveries after the first
    marks: list         # 1484 * last_packet_acked after every move, capped at CHUNK_LEN

    @property
    def whole(self) -> bool:
        return self.acked == NPACK


def replay_attempt(data: bytes, sc: Scenario, ch: Chunk, attempt: int) -> Attempt:
    assert len(data) == CHUNK_LEN
    buf = bytearray(b"\xa5" * CHUNK_LEN)
    lcg = _Lcg(ch.seed ^ ((0x9E3779B97F4A7C15 * (attempt + 1)) & M64))
    lpa, laf = 0, WINDOW
    flags = [0] * WINDOW
    count = [0] * (NPACK + 2)
    first = attempt == 0
    early = first and ch.early
    force = 0
    delivered = 0
    marks = []

    def received(seq):
        return flags[seq - lpa - 1] != 0

    def pick():
        nonlocal force
        lo = lpa + 1
        if force:
            seq, force = force, 0
            return seq
        if early:
            if laf >= NPACK:
                return NPACK
            hi = min(laf, NPACK - 2)
        else:
            if lo == NPACK:
                return NPACK
            hi = min(laf, NPACK - 1)
        if first:
            for s, _, _, kind in ch.corr:
                if kind == "D" and lo < s <= hi and not count[s]:
                    force = s
                    return s
        if lcg.next() % 100 < sc.stray:
            return lpa if (lcg.next() & 1) and lpa >= 1 else laf + 1
        if lcg.next() % 100 >= sc.reorder:
            return lo
        seq = lo + lcg.next() % (hi - lo + 1)
        if received(seq) and lcg.next() % 100 >= sc.dup:
            while received(seq):
                seq = lo if seq == hi else seq + 1
        return seq

    for _ in range(100000):
        seq = pick()
        if seq <= lpa or seq > laf:
            continue  # the stray-packet filter
        blen = LAST_BODY if seq == NPACK else BODY
        body = bytearray(data[BODY * (seq - 1):BODY * (seq - 1) + blen])
        if first:
            for s, off, mask, kind in ch.corr:
                if s == seq and (kind == "D") == (count[seq] > 0):
                    body[off] ^= mask
        count[seq] += 1
        delivered += 1
        if not received(seq):
            buf[BODY * (seq - 1):BODY * (seq - 1) + blen] = body
            flags[seq - lpa - 1] = 1
        if seq == lpa + 1:  # cumulative_ack
            k = 0
            while k < WINDOW and flags[k]:
                k += 1
            lpa += k
            laf += k
            flags = flags[k:] + [0] * k
            marks.append(min(CHUNK_LEN, BODY * lpa))
        if seq == NPACK:  # the short datagram: packet_handler.c:469
            return Attempt(bytes(buf), lpa, delivered, {s: c - 1 for s, c in enumerate(count) if c > 1}, marks)
    raise AssertionError("the schedule did not reach the last packet")


@dataclass
class Expected:
    results: dict   # (chunk, attempt) -> (verdict, digest, buffer)
    drops: dict     # (chunk, attempt) -> buffer         (pv modes only)
    attempts: dict  # (chunk, attempt) -> Attempt


def expected_run(data: bytes, sc: Scenario, mode: str) -> Expected:
    """What a correct run prints and dumps.  A session whose short last packet
    arrives above a hole is verified as it stands by the queue modes (and the
    reference), and dropped by the progressive verifier, which cannot complete
    it; a mismatch or a drop is followed by a clean re-GET."""
    exp = Expected({}, {}, {})
    for c, ch in enumerate(sc.chunks):
        chunk = data[c * CHUNK_LEN:(c + 1) * CHUNK_LEN]
        want = hashlib.sha1(chunk).digest()
        for attempt in range(4):
            a = replay_attempt(chunk, sc, ch, attempt)
            exp.attempts[c, attempt] = a
            if mode in PV_MODES and not a.whole:
                exp.drops[c, attempt] = a.buf
                continue
            digest = hashlib.sha1(a.buf).digest()
            exp.results[c, attempt] = (int(digest != want), digest, a.buf)
            if digest == want:
                break
        else:
            raise AssertionError(f"chunk {c} never verifies in the replay")
    return exp


def tag_of(chunk: int, attempt: int) -> int:
    return 0x1000 + chunk * 16 + attempt


def write_inputs(tmp, data: bytes, sc: Scenario):
    """The driver's three input files and its output directory."""
    k = len(sc.chunks)
    assert len(data) == k * CHUNK_LEN
    paths = {n: os.path.join(str(tmp), n) for n in ("data.bin", "chunks.txt", "scenario.txt", "out")}
    with open(paths["data.bin"], "wb") as f:
        f.write(data)
    with open(paths["chunks.txt"], "w") as f:  # the reference's chunk-file format: "<id> <hash>"
        for c in range(k):
            f.write(f"{c} {hashlib.sha1(data[c * CHUNK_LEN:(c + 1) * CHUNK_LEN]).hexdigest()}\n")
    with open(paths["scenario.txt"], "w") as f:
        f.write(sc.text())
    os.makedirs(paths["out"], exist_ok=True)
    return paths


def run_driver(exe: str, mode: str, paths: dict, env: dict, timeout: float):
    """Runs the driver in a child; its stdout (mostly the reference's own
    chatter) goes to a file.  Returns (exit status, the driver's own lines)."""
    log = os.path.join(paths["out"], "stdout.txt")
    with open(log, "wb") as out:
        r = subprocess.run([exe, mode, paths["data.bin"], paths["chunks.txt"], paths["scenario.txt"], paths["out"]],
                           stdout=out, stderr=subprocess.PIPE, env=env, timeout=timeout)
    with open(log, "r", errors="replace") as f:
        lines = [ln.split() for ln in f if ln.startswith("RSM ")]
    return r.returncode, lines, r.stderr.decode(errors="replace")


def check_run(mode: str, data: bytes, sc: Scenario, paths: dict, rc: int, lines: list, stderr: str = "") -> dict:
    """Every assertion the issue asks of a run; returns the parsed STATS and
    COUNTS lines as a dict of ints."""
    exp = expected_run(data, sc, mode)
    if rc != 0:
        # say what the driver saw, and the first results that differ from the replay
        tail = [" ".join(ln) for ln in lines if ln[1] == "ERROR"]
        wrong = []
        for ln in lines:
            if ln[1] == "RESULT":
                want = exp.results.get((int(ln[2]), int(ln[3])))
                got = (int(ln[5]), bytes.fromhex(ln[6]) if len(ln) > 6 else None)
                if want is None:
                    wrong.append(f"chunk {ln[2]} attempt {ln[3]}: no such session in the replay")
                elif got[0] != want[0] or (got[1] is not None and got[1] != want[1]):
                    wrong.append(f"chunk {ln[2]} attempt {ln[3]}: verdict {got[0]} digest {ln[6] if len(ln) > 6 else '-'}, "
                                 f"replay {want[0]} {want[1].hex()}")
        raise AssertionError(f"driver exit status {rc}: {tail}; results that differ from the replay: {wrong[:4]}; "
                             f"stderr: {stderr[-1000:]}")
    results, drops, jobs, info = {}, {}, [], {}
    seen_tags = []
    for ln in lines:
        if ln[1] == "RESULT":
            key = (int(ln[2]), int(ln[3]))
            assert key not in results, f"{key} reported twice"
            results[key] = (int(ln[5]), bytes.fromhex(ln[6]) if len(ln) > 6 else None)
            seen_tags.append(int(ln[4]))
            assert int(ln[4]) == tag_of(*key)
        elif ln[1] == "DROP":
            key = (int(ln[2]), int(ln[3]))
            assert key not in drops
            drops[key] = int(ln[4])
            assert int(ln[4]) == tag_of(*key)
        elif ln[1] == "JOB":
            jobs.append(int(ln[2]))
        elif ln[1] in ("STATS", "COUNTS"):
            info.update({k: int(v) for k, v in (x.split("=") for x in ln[2:])})
    # each tag exactly once, and exactly the replay's sessions
    assert sorted(seen_tags) == sorted(tag_of(*k) for k in exp.results), (sorted(results), sorted(exp.results))
    assert sorted(drops) == sorted(exp.drops)
    assert not set(drops.values()) & set(seen_tags)
    for key, (verdict, digest, buf) in exp.results.items():
        with open(os.path.join(paths["out"], f"buf_{key[0]}_{key[1]}.bin"), "rb") as f:
            dumped = f.read()
        if dumped != buf:
            bad = [i for i in range(CHUNK_LEN) if dumped[i] != buf[i]]
            raise AssertionError(f"session buffer of {key} differs from the replay at {len(bad)} bytes, "
                                 f"first {bad[0]} (packet {bad[0] // BODY + 1}), last {bad[-1]}")
        got_verdict, got_digest = results[key]
        assert got_verdict == verdict, (key, got_verdict, verdict)
        if mode in PV_MODES:
            assert got_digest == digest, (key, got_digest.hex(), digest.hex())
    for key, buf in exp.drops.items():
        with open(os.path.join(paths["out"], f"buf_{key[0]}_{key[1]}.bin"), "rb") as f:
            assert f.read() == buf, f"dropped session buffer of {key} differs from the replay"
    # every chunk finally verified (the re-GETs are clean): the job buffers are the data file
    assert jobs == list(range(len(sc.chunks)))
    with open(os.path.join(paths["out"], "job.bin"), "rb") as f:
        job = f.read()
    if job != data:
        bad = [c for c in range(len(sc.chunks)) if job[c * CHUNK_LEN:(c + 1) * CHUNK_LEN] != data[c * CHUNK_LEN:(c + 1) * CHUNK_LEN]]
        raise AssertionError(f"job buffers of chunks {bad[:16]} differ from the data file")
    info["_expected"] = exp
    return info


# ---- the scenarios both modules use ----------------------------------------
# Between them A and B flip one bit at every position of EDGE_OFFSETS in a
# chunk of its own (two corruptions in one chunk would hide each other), hold
# clean chunks, chunks whose only corruption sits in a duplicate copy (the
# reference's `copied` flag drops it: verdict 0), a chunk whose first copy is
# corrupted and followed by a clean duplicate (verdict 1), and two chunks each
# whose short last packet arrives above a hole.
def scenario_a(sessions: int, **kw) -> Scenario:
    return Scenario(sessions, [
        Chunk(101, corr=[at(0, 0x01)]),
        Chunk(102, corr=[at(1483, 0x80)]),
        Chunk(103, corr=[at(1484, 0x01)]),
        Chunk(104, corr=[at(1535, 0x10)]),
        Chunk(105, early=True),
        Chunk(106, corr=[at(1484, 0x01, "D"), at(176 * BODY + 700, 0x20, "D"), at(523851, 0x80, "D")]),
        Chunk(107, corr=[at(1536, 0x02), at(1536, 0x00, "D")]),
        Chunk(108, early=True, corr=[at(300 * BODY + 5, 0x40, "D")]),
    ], **kw)


def scenario_b(sessions: int, **kw) -> Scenario:
    return Scenario(sessions, [
        Chunk(201, corr=[at(176 * BODY + 700, 0x08)]),
        Chunk(202, early=True),
        Chunk(203, corr=[at(523851, 0x01)]),
        Chunk(204, corr=[at(523852, 0x80)]),
        Chunk(205, corr=[at(524287, 0x01)]),
        Chunk(206),
        Chunk(207, early=True, corr=[at(1536, 0x04)]),
        Chunk(208, corr=[at(1535, 0x10, "D"), at(1536, 0x10, "D")]),
    ], **kw)


def scenario_many(sessions: int, k: int, **kw) -> Scenario:
    """k chunks: A's, B's, then clean ones."""
    chunks = (scenario_a(1).chunks + scenario_b(1).chunks)[:k]
    chunks += [Chunk(1000 + i) for i in range(k - len(chunks))]
    return Scenario(sessions, chunks, **kw)


def corpus(k: int, seed: int = 20) -> bytes:
    import numpy as np
    return np.random.default_rng(seed).bytes(k * CHUNK_LEN)
