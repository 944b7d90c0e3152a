"""tests/acc_model.py itself: the inverse of splitmix64, the placement of keys by their hash, and the rounds the restated
host rules of an add take on the placed streams that tests/test_acc_placement.py runs on the device."""
import numpy as np
import pytest

import acc_model as A

U64 = np.uint64
ONES = U64(0xFFFFFFFFFFFFFFFF)


def test_unsplitmix64_inverts_splitmix64_both_ways():
    x = np.concatenate([np.random.default_rng(0xACC).integers(0, 1 << 64, 100_000, dtype=U64), [U64(0), ONES]])
    assert np.array_equal(A.unsplitmix64(A.splitmix64(x)), x)
    assert np.array_equal(A.splitmix64(A.unsplitmix64(x)), x)
    # the hash itself: splitmix64's published first output for the state 0, which is splitmix64(0) here
    assert int(A.splitmix64(np.array([0], U64))[0]) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("bits,prefix,home", [(4, 9, None), (4, 9, 4095), (11, A.PREFIX11, None), (12, 2 * A.PREFIX11 + 1, 0), (0, 0, 17)])
def test_place_gives_the_prefix_the_home_and_a_free_bit_under_the_prefix(bits, prefix, home):
    keys = A.place(np.random.default_rng(bits), 3000, prefix, bits, home=home)
    assert len(np.unique(keys)) == 3000
    h = A.splitmix64(keys)
    if bits:
        assert np.all(h >> U64(64 - bits) == U64(prefix))
    assert np.all(A.partition_of(keys, bits) == prefix)
    if home is not None:
        assert np.all(A.home_of(keys) == home)
    under = (h >> U64(63 - bits)) & U64(1)
    assert 1300 < int(under.sum()) < 1700, "the bit under the prefix does not vary"   # (3000 fair bits: 1500 +- 7 sigma)
    if home is None:
        assert len(np.unique(A.home_of(keys))) > 1500                 # (3000 uniform homes of 4096: about 2100 different)


def test_place_canonical_keys_and_palindromes():
    rng = np.random.default_rng(7)
    c = A.place(rng, 2000, 9, 4, home=4000, canonical=True)
    assert len(np.unique(c)) == 2000 and np.all(A.partition_of(c, 4) == 9) and np.all(A.home_of(c) == 4000)
    rc = A.rc_np(c, 32)
    assert np.array_equal(A.canonical_np(c, 32), c) and np.array_equal(A.canonical_np(rc, 32), c) and not np.any(rc == c)
    p = A.palindromes(rng, 64)
    assert len(np.unique(p)) == 64 and np.array_equal(A.rc_np(p, 32), p)
    # 32 A < 32 T and 32 C < 32 G: key 0 is canonical, the all-ones key is not
    assert A.canonical_np([0, ONES], 32).tolist() == [0, 0xAAAAAAAAAAAAAAAA]


def test_place_small_k_by_forward_search():
    keys = A.place_small_k(np.random.default_rng(21), 3585, 21, 0x26, 6)
    assert len(np.unique(keys)) == 3585 and int(keys.max()) < 4 ** 21
    assert np.all(A.partition_of(keys, 6) == 0x26) and len(np.unique(A.partition_of(keys, 7))) == 2


def test_the_models_constants():
    assert [A.acc_bits_for(g, b) for g, b in ((1, 0), (49_152, 0), (49_153, 0), (3585, 5), (19_784, 5), (98_305, 5), (7, 9))] == \
        [4, 4, 5, 5, 5, 6, 9]
    # the bins the issue's cases are written for: (histogram groups, bits) -> entries
    assert A.bin_cap(3584, 4) == 384 and A.bin_cap(20_000, 4) == 1568 and A.bin_cap(20_000, 4, 1569) == 1600
    assert A.bin_cap(32_000, 4) == 2400 and A.bin_cap(16_200, 4) == 1312 and A.bin_cap(3585, 12) == 64
    assert A.bin_cap(60_000, 4) == 4096 and A.bin_cap(100, 4, 4097) == 4096


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_the_model_takes_the_rounds_the_cases_are_written_for(name):
    """every step of every placed case: the rounds and partitions written in the case (groups B and C: those of the issue
    that asked for them), the groups np.unique's"""
    for step, parts, rounds, (gk, gc) in A.run_model(name):
        assert rounds[-1] == "commit" and parts >= 16
        assert len(gk) == len(np.unique(gk)) and int(np.bincount(A.partition_of(gk, parts.bit_length() - 1)).max()) <= A.ACC_BOUND


def test_the_exception_case_is_the_exception():
    """what the canonical dry run meets in "exception": bins that fit, occ + arrivals past the bound, occ + the new unflipped
    keys past the slots -- and a growth decision that does not depend on what the dry run then reports"""
    (s0, _, _, _), (s1, parts, rounds, (gk, _)) = A.run_model("exception")
    arr = A.canonical_np(s1.keys, 32)
    arrivals = np.bincount(A.partition_of(arr, 4), minlength=16)
    assert len(s1.keys) == 16_200 and A.bin_cap(16_200, 4) == 1312 >= arrivals.max() == arrivals[A.PART] == 1200
    assert 3584 + 1200 > A.ACC_BOUND and 3584 + 600 > A.ACC_SLOTS
    assert int((arr == s1.keys)[A.partition_of(arr, 4) == A.PART].sum()) == 600
    assert A.acc_bits_for(3584 + 15_600, 5) == A.acc_bits_for(3584 + 16_200, 5) == 5
    assert (parts, len(gk)) == (32, 19_184)


def test_total_skew_at_every_split():
    """"bound-later-585": the 3000 residents share 11 hash bits, so from 4 bits to 11 every split sends them to one child"""
    (s0, _, _, _), (s1, parts, rounds, _) = A.run_model("bound-later-585")
    assert rounds.count("grow") == 8 and parts == 4096
    assert all(len(np.unique(A.partition_of(s0.keys, b))) == 1 for b in range(4, 12))
    assert len(np.unique(A.partition_of(s0.keys, 12))) == 2
