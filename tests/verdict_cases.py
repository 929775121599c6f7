"""Helper of tests/test_gpu_verdict_width.py: the chunks and the expected-
digest matrices every verdict-producing entry point is run against.  Plain
numpy and hashlib, no import of the library.  Not a test module.

The truth is hashlib: `want[i] = hashlib.sha1(chunk i).digest()`.  A case is a
pair (expected, mismatch): `expected` is `want` with some rows altered,
`mismatch[i]` is 1 where row i of `expected` is not row i of `want`, which is
what verify_hash (0 = match, 1 = mismatch) must answer for chunk i.

  flip_matrix  each of the 160 bits of a digest flipped in exactly one row (bit
               j = byte j // 8, bit j % 8), the other 40 rows untouched: a
               compare that skips a word, a byte or a bit answers 0 for one of
               them.  "ident" puts bit j at row j, "stride" at row
               (77 * j + 5) % 200, so that between the two every lane 0..63 of
               a group of 64 rows meets low and high digest words.
  swaps        rows exchanged pairwise inside a group of 64, across the group
               edges 63|64 and 127|128 and at both ends: a compare that reads
               the neighbour's row answers 0 for them.
  extremes     every bit of a row flipped, a row of zeros, a clean row: a diff
               built with the wrong operator, or a compare against a row that
               was never written.

N = 200 is three full groups of 64 and one of 8 (a persistent drain's
`lane < count` edge).  The digests of the 185 non-empty chunks are all
different; the 15 empty chunks (rows 0, 14, 28, ...) share SHA-1("").  No
swapped pair holds an empty chunk twice, so every swapped row is a mismatch."""
import hashlib

import numpy as np

N = 200
DIGEST_LEN = 20
BITS = 8 * DIGEST_LEN
LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 511, 700]  # the padding edges, and several blocks
MAX_LEN = max(LENGTHS)
GUARD = 0xA5
SWAPS = ((0, 1), (62, 63), (63, 64), (127, 128), (198, 199))
CASES = ("ident", "stride", "swaps", "extremes")


class Chunks:
    """N chunks packed into `data` at odd byte offsets, 1..15 guard bytes
    (0xA5) before each and 16 behind the last; `want` their hashlib digests,
    (N, 20) uint8."""

    def __init__(self, data, offsets, lengths, want):
        self.data, self.offsets, self.lengths, self.want = data, offsets, lengths, want

    def chunk(self, i: int) -> np.ndarray:
        o = int(self.offsets[i])
        return self.data[o:o + int(self.lengths[i])]


def chunks(seed: int) -> Chunks:
    rng = np.random.default_rng(seed)
    lengths = np.array([LENGTHS[i % len(LENGTHS)] for i in range(N)], np.uint32)
    offsets = np.zeros(N, np.uint64)
    single = rng.permutation(256).astype(np.uint8)  # the one-byte chunks: no byte twice
    parts, cur = [], 0
    for i in range(N):
        gap = 1 + (7 * i) % 15
        if (cur + gap) % 2 == 0:  # the chunk starts at an odd byte
            gap += 1 if gap < 15 else -1
        body = rng.integers(0, 256, int(lengths[i]), dtype=np.uint8)
        if lengths[i] == 1:
            body[0] = single[i // len(LENGTHS)]
        parts += [np.full(gap, GUARD, np.uint8), body]
        offsets[i] = cur + gap
        cur += gap + int(lengths[i])
    data = np.concatenate(parts + [np.full(16, GUARD, np.uint8)])
    raw = data.tobytes()
    want = np.frombuffer(b"".join(hashlib.sha1(raw[int(o):int(o) + int(n)]).digest()
                                  for o, n in zip(offsets, lengths)), np.uint8).reshape(N, DIGEST_LEN).copy()
    assert (offsets % 2 == 1).all()
    # every digest once -- but the empty chunk's, which the length cycle brings 15 times
    filled = np.flatnonzero(lengths)
    assert len({want[i].tobytes() for i in filled}) == filled.size == N - 15, "two chunks with one digest"
    assert len({w.tobytes() for w in want}) == filled.size + 1
    want.setflags(write=False)
    data.setflags(write=False)
    return Chunks(data, offsets, lengths, want)


def flip_row(placement: str, j: int) -> int:
    """The row that carries flipped bit j."""
    if placement == "ident":
        return j
    if placement == "stride":
        return (77 * j + 5) % N  # 77 is coprime to 200: 160 distinct rows
    raise ValueError(placement)


def flip_matrix(want: np.ndarray, placement: str):
    expected = np.array(want, np.uint8)
    mismatch = np.zeros(N, np.uint8)
    for j in range(BITS):
        row = flip_row(placement, j)
        assert not mismatch[row]
        expected[row, j // 8] ^= 1 << (j % 8)
        mismatch[row] = 1
    return expected, mismatch


def swaps(want: np.ndarray):
    expected = np.array(want, np.uint8)
    mismatch = np.zeros(N, np.uint8)
    for a, b in SWAPS:  # in turn: row 63 is in two pairs, so 62, 63, 64 rotate (nine rows in all)
        expected[[a, b]] = expected[[b, a]]
        mismatch[[a, b]] = 1
    return expected, mismatch


def extremes(want: np.ndarray):
    expected = np.array(want, np.uint8)
    expected[0::3] = ~expected[0::3]
    expected[1::3] = 0
    mismatch = (np.arange(N) % 3 != 2).astype(np.uint8)
    return expected, mismatch


def case(want: np.ndarray, name: str):
    """(expected, mismatch) of the case called `name` (one of CASES)."""
    if name in ("ident", "stride"):
        return flip_matrix(want, name)
    return {"swaps": swaps, "extremes": extremes}[name](want)


def describe(expected: np.ndarray, want: np.ndarray, row: int) -> str:
    """How row `row` of `expected` differs from `want`, for a failure message."""
    diff = np.unpackbits(expected[row] ^ want[row], bitorder="little")
    bits = np.flatnonzero(diff)
    if bits.size == 0:
        return f"row {row}: expected digest untouched"
    if bits.size == 1:
        j = int(bits[0])
        return f"row {row}: expected digest has byte {j // 8} bit {j % 8} flipped (word {j // 32})"
    return f"row {row}: expected digest differs in {bits.size} bits, the first at byte {int(bits[0]) // 8}"


def check(got, mismatch, expected=None, want=None, what: str = "") -> None:
    """`got` holds only 0 and 1 and equals `mismatch` everywhere; the failure
    names the rows -- with `expected` and `want`, the byte and bit -- that
    were missed (0 for an altered row) or falsely flagged (1 for a clean one)."""
    got = np.asarray(got)
    mismatch = np.asarray(mismatch)
    assert got.shape == mismatch.shape, f"{what}: {got.shape} verdicts for {mismatch.shape} rows"
    odd = np.flatnonzero((got != 0) & (got != 1))
    assert odd.size == 0, f"{what}: verdicts neither 0 nor 1 at rows {odd[:8].tolist()}: {got[odd[:8]].tolist()}"
    wrong = np.flatnonzero(got != mismatch)
    if wrong.size:
        def name(r):
            kind = "missed" if mismatch[r] else "false alarm"
            return f"{kind} at " + (describe(expected, want, int(r)) if expected is not None and want is not None
                                    else f"row {int(r)}")
        raise AssertionError(f"{what}: {wrong.size} wrong verdicts of {got.size}: " +
                             "; ".join(name(r) for r in wrong[:6]))
