"""tests/philox_ref.py against the Random123 known-answer vectors, and the
properties of the project's counter layouts that can be checked on the
reference alone.  The device streams are compared with this reference bit for
bit in tests/test_gpu_rng.py."""
import numpy as np
import pytest

import philox_ref as P

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, result)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answer_vectors(ctr, key, want):
    got = P.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [hex(int(v)) for v in got] == [hex(v) for v in want]


def test_vectorised_equals_one_by_one():
    """A batch of counters (and a batch of keys) gives what each gives alone."""
    ctr = np.array([k[0] for k in KAT], np.uint64)
    key = np.array([k[1] for k in KAT], np.uint64)
    want = np.array([k[2] for k in KAT], np.uint32)
    assert np.array_equal(P.philox4x32_10(ctr, key), want)
    same_key = P.philox4x32_10(ctr, KAT[2][1])  # one key broadcast over the counters
    assert np.array_equal(same_key[2], want[2]) and not np.array_equal(same_key[0], want[0])


def test_gate_counter_is_no_feature_counter():
    """(r, 16, off) is none of (r', 0..15, off): word 1 separates them, so the
    gate never shares a block with a feature quad, at any row or offset."""
    rows = np.array([0, 1, 15, 16, 17, 4112, 2 ** 32 - 1], np.uint64)
    for off in (0, 1, 2 ** 32 + 5, 2 ** 64 - 1):
        gate = {tuple(int(v) for v in c) for c in P.gate_counters(off, rows)}
        feat = {tuple(int(v) for v in c) for c in P.feat_counters(off, rows).reshape(-1, 4)}
        assert len(gate) == rows.size and len(feat) == rows.size * 16
        assert not gate & feat
        assert {c[1] for c in gate} == {16} and {c[1] for c in feat} == set(range(16))
        assert {c[2:] for c in gate | feat} == {(off & 0xFFFFFFFF, off >> 32)}
    # and the streams differ: gate word 0 is not feature quad 0's word 0
    assert P.noise_gate(7, 0, rows[:4])[0] != P.noise_feat(7, 0, rows[:4])[0, 0]


def test_offset_and_seed_halves_reach_the_block():
    """off_hi, seed_hi and bit 31 of either half change the draw."""
    rows = np.arange(4)
    base = P.noise_feat(5, 5, rows)
    for seed, off in ((5, 2 ** 32 + 5), (2 ** 32 + 5, 5), (5 | 1 << 31, 5), (5, 5 | 1 << 31)):
        assert not np.array_equal(P.noise_feat(seed, off, rows), base)
    assert np.array_equal(P.noise_feat(5, 5, rows)[2], P.noise_feat(5, 5, np.array([2]))[0])


def test_u01_range():
    u = P.u01(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], np.uint32))
    assert u.dtype == np.float32
    assert u[0] == 0.0 and u[1] == 0.0 and u[2] == np.float32(2.0 ** -24)
    assert u[3] == np.float32(1.0 - 2.0 ** -24) and u[3] < 1.0
    assert (u >= 0).all() and (u < 1).all()


def test_dropout_keep_packing():
    """Column c is bit c % 32 of word c / 32, words in block order; a row past
    2^32 folds its high half into the tag word."""
    rows = np.array([0, 3, 2 ** 32 + 3], np.uint64)
    keep = P.dropout_keep(11, 2, rows)
    assert keep.shape == (3, 128) and keep.dtype == bool
    words = P.philox4x32_10(P.dropout_counters(2, rows), (11, 0))
    for r in range(3):
        for c in (0, 1, 31, 32, 63, 64, 127):
            assert keep[r, c] == bool((int(words[r, c // 32]) >> (c % 32)) & 1)
    ctr = P.dropout_counters(2, rows)
    assert int(ctr[1, 1]) == P.DROP_TAG and int(ctr[2, 1]) == P.DROP_TAG ^ 1
    assert int(ctr[1, 0]) == int(ctr[2, 0]) == 3 and not np.array_equal(keep[1], keep[2])
