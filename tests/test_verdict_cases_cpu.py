"""The case builder of the verdict tests (tests/verdict_cases.py) checked on
its own, without a device: the cases are what test_gpu_verdict_width.py says
they are, and `check` refuses every kind of wrong answer."""
import hashlib

import numpy as np
import pytest

import verdict_cases as vc


@pytest.fixture(scope="module")
def ch():
    return vc.chunks(7)


def _bits(a, b):
    """Differing bits per row."""
    return np.unpackbits(np.asarray(a) ^ np.asarray(b), axis=1).sum(axis=1)


def test_chunks(ch):
    assert ch.want.shape == (vc.N, 20) and vc.N == 200
    assert [int(n) for n in ch.lengths[:len(vc.LENGTHS)]] == vc.LENGTHS
    assert set(int(n) for n in ch.lengths) == set(vc.LENGTHS)
    raw = ch.data.tobytes()
    end = 0
    for i in range(vc.N):
        o, n = int(ch.offsets[i]), int(ch.lengths[i])
        assert o % 2 == 1 and 1 <= o - end <= 15
        assert raw[end:o] == bytes([vc.GUARD]) * (o - end)
        assert hashlib.sha1(raw[o:o + n]).digest() == ch.want[i].tobytes()
        assert ch.chunk(i).tobytes() == raw[o:o + n]
        end = o + n
    assert raw[end:] == bytes([vc.GUARD]) * 16
    # all digests distinct, but for the empty chunk's, which the length cycle repeats
    empty = hashlib.sha1(b"").digest()
    assert [i for i in range(vc.N) if ch.want[i].tobytes() == empty] == list(range(0, vc.N, len(vc.LENGTHS)))
    assert len({w.tobytes() for w in ch.want}) == vc.N - 14
    again = vc.chunks(7)
    assert np.array_equal(again.data, ch.data) and np.array_equal(again.want, ch.want)
    assert not np.array_equal(vc.chunks(8).want, ch.want)


@pytest.mark.parametrize("placement", ["ident", "stride"])
def test_flip_matrix(ch, placement):
    exp, mis = vc.flip_matrix(ch.want, placement)
    assert exp.shape == (vc.N, 20) and exp.dtype == np.uint8 and mis.shape == (vc.N,)
    assert int(mis.sum()) == 160
    dist = _bits(exp, ch.want)
    assert np.array_equal(dist, mis)  # Hamming distance 1 where flagged, identical rows elsewhere
    # each of the 160 bits exactly once, at the row the placement names
    seen = {}
    for row in np.flatnonzero(mis):
        j = int(np.flatnonzero(np.unpackbits(exp[row] ^ ch.want[row], bitorder="little"))[0])
        assert exp[row, j // 8] ^ ch.want[row, j // 8] == 1 << (j % 8)
        assert j not in seen
        seen[j] = int(row)
    assert sorted(seen) == list(range(160))
    assert all(seen[j] == vc.flip_row(placement, j) for j in range(160))
    assert len(set(seen.values())) == 160  # injective
    assert not np.shares_memory(exp, ch.want)


def test_every_group_of_64_meets_flipped_and_clean_rows(ch):
    """"ident" alone flips all of rows 0..127 and none of 192..199, "stride"
    all of 192..199: between the two placements each group of 64 rows (the
    last one of 8) holds flipped rows and clean rows, and "stride" mixes
    them in the three full groups."""
    ident = vc.flip_matrix(ch.want, "ident")[1]
    stride = vc.flip_matrix(ch.want, "stride")[1]
    for g in range(0, vc.N, 64):
        a, b = ident[g:g + 64], stride[g:g + 64]
        assert a.any() or b.any(), g
        assert not a.all() or not b.all(), g
        if g < 192:
            assert 0 < int(b.sum()) < 64, g
    assert not ident[192:].any() and stride[192:].all()


def test_placements_cover_every_lane_with_low_and_high_words(ch):
    """Between the two placements, every lane of a group of 64 rows decides
    on a flip in words 0-1 and on one in words 3-4."""
    low, high = set(), set()
    for placement in ("ident", "stride"):
        for j in range(160):
            lane = vc.flip_row(placement, j) % 64
            if j // 32 <= 1:
                low.add(lane)
            if j // 32 >= 3:
                high.add(lane)
    assert low == set(range(64)) and high == set(range(64))


def test_swaps(ch):
    exp, mis = vc.swaps(ch.want)
    assert vc.SWAPS == ((0, 1), (62, 63), (63, 64), (127, 128), (198, 199))
    # the pairs' ten ends are nine rows: 63 is in two pairs
    assert np.flatnonzero(mis).tolist() == [0, 1, 62, 63, 64, 127, 128, 198, 199]
    assert np.array_equal((exp != ch.want).any(axis=1), mis.astype(bool))
    # every altered row holds a neighbour's true digest; 63 | 64 and 127 | 128 cross a group of 64
    holds = {0: 1, 1: 0, 62: 63, 63: 64, 64: 62, 127: 128, 128: 127, 198: 199, 199: 198}
    assert all(np.array_equal(exp[r], ch.want[src]) for r, src in holds.items())
    assert sorted(e.tobytes() for e in exp) == sorted(w.tobytes() for w in ch.want)  # a permutation of the rows


def test_extremes(ch):
    exp, mis = vc.extremes(ch.want)
    assert mis.tolist() == [1, 1, 0] * 66 + [1, 1]
    assert np.array_equal((exp != ch.want).any(axis=1), mis.astype(bool))
    assert (_bits(exp[0::3], ch.want[0::3]) == 160).all()
    assert (exp[1::3] == 0).all()
    assert np.array_equal(exp[2::3], ch.want[2::3])


@pytest.mark.parametrize("name", vc.CASES)
def test_check(ch, name):
    exp, mis = vc.case(ch.want, name)
    vc.check(mis.copy(), mis, exp, ch.want, "right")
    vc.check(mis.astype(np.int64).tolist(), mis)
    hit = int(np.flatnonzero(mis)[3])
    clean = int(np.flatnonzero(mis == 0)[3])
    missed = mis.copy()
    missed[hit] = 0
    with pytest.raises(AssertionError, match=f"missed at row {hit}:") as e:
        vc.check(missed, mis, exp, ch.want, "a missed flip")
    if name in ("ident", "stride"):
        j = [j for j in range(160) if vc.flip_row(name, j) == hit][0]
        assert f"byte {j // 8} bit {j % 8} flipped" in str(e.value)
    alarm = mis.copy()
    alarm[clean] = 1
    with pytest.raises(AssertionError, match=f"false alarm at row {clean}: expected digest untouched"):
        vc.check(alarm, mis, exp, ch.want, "a false alarm")
    for row in (hit, clean):  # a value that is neither, where a 1 and where a 0 is due
        two = mis.copy()
        two[row] = 2
        with pytest.raises(AssertionError, match="neither 0 nor 1"):
            vc.check(two, mis, exp, ch.want, "a 2")
    with pytest.raises(AssertionError):
        vc.check(mis[:-1], mis)
    with pytest.raises(AssertionError, match="row"):
        vc.check(missed, mis)  # without the matrices the row alone is named
