"""The ordered count at every key width: dnagpu_count_keys, dnagpu_count_keys_in_range, the owner paths
(dnagpu_count_kmers_owned, dnagpu_partition_kmers) and dnagpu_count_kmers over a plain sequence, for every k and for the
key-bit counts (`rem` of plan_bits, csrc/count_kernels.hip) at which the level plan changes regime: rem <= 10 (one terminal
split), rem <= 20 (one digit left for a terminal next level), rem > 20 (split by size), the forced owner level and a root
whose rem is 2k - fixed for any fixed in 0 .. 2k.

The reference is exact everywhere: np.unique over the host's uint64 keys (orc.count_keys for the keys of a sequence).
Integer work: every comparison is bit-exact.  The key generators are checked on the CPU by a test that needs no device; the
device tests carry the gpu mark one by one, so that this one does not."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import load_package

gpu = pytest.mark.gpu

LEAF_CAP = 6144                       # csrc/kernels.hpp: the keys one leaf sorts
N_SMALL, N_LARGE = LEAF_CAP + 1, 200_003
ERR_INVALID_K, ERR_BAD_ARG = 1, 5     # include/dnagpu.h


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shard_math():
    # (shard_math, not sharded: importing torch here would put a second ROCm runtime into this process)
    return importlib.import_module(load_package().__name__ + ".shard_math")


def assert_same(got, want, what):
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape[0]} values, oracle has {want.shape[0]}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ; first at {i}: "
                             f"got {int(got[i]):#x}, oracle {int(want[i]):#x}")


def check_hist(hist, ok, oc, what):
    """test_gpu_parity.check_hist, plus what holds for every ordered count: total = rows, sorted unless empty;
    -> the download"""
    gk, gc = hist.download()
    assert hist.distinct == len(ok), f"{what}: {hist.distinct} groups, oracle {len(ok)}"
    assert_same(gk, ok, what + " keys")
    assert_same(gc, oc, what + " counts")
    assert hist.summary() == orc.hist_summary(ok, oc), what + " summary"
    assert hist.total == int(np.sum(oc, dtype=np.uint64)), what + " total"
    if len(ok):
        assert hist.is_sorted, what + " is_sorted"
    return gk, gc


def unique_u64(keys):
    ok, oc = np.unique(np.asarray(keys, dtype=np.uint64), return_counts=True)
    return ok, oc.astype(np.uint64)


# ------------------------------------------------------------------ key generators (plain functions, checked on the CPU)

def key_mask(k):
    return (1 << (2 * k)) - 1


def rand_bits(rng, n, b):
    """n values of b random low bits"""
    if b <= 0:
        return np.zeros(n, dtype=np.uint64)
    return rng.integers(0, 1 << b, n, dtype=np.uint64)


def rand_key(rng, b):
    return int(rand_bits(rng, 1, b)[0])


def gen_uniform(k, n, seed=1):
    return rand_bits(np.random.default_rng([seed, k, n]), n, 2 * k)


def gen_low_bits(k, n, b, seed=2):
    """a random constant prefix, b random low bits"""
    rng = np.random.default_rng([seed, k, n, b])
    prefix = (rand_key(rng, 2 * k) >> b) << b
    return np.uint64(prefix) | rand_bits(rng, n, b)


def gen_high_bits(k, n, b, seed=3):
    """b random top bits, the low part constant"""
    rng = np.random.default_rng([seed, k, n, b])
    low_bits = 2 * k - b
    low = rand_key(rng, low_bits)
    return (rand_bits(rng, n, b) << np.uint64(low_bits)) | np.uint64(low)


def gen_dominant(k, n, f, seed=4):
    """one key makes up the share f of the array, the rest uniform"""
    rng = np.random.default_rng([seed, k, n, int(f * 1000)])
    keys = rand_bits(rng, n, 2 * k)
    keys[rng.permutation(n)[:int(n * f)]] = np.uint64(rand_key(rng, 2 * k))
    return keys


def gen_two_keys(k, n, seed=5):
    """two keys that differ in the top and in the lowest key bit"""
    rng = np.random.default_rng([seed, k, n])
    a = rand_key(rng, 2 * k)
    b = a ^ ((1 << (2 * k - 1)) | 1)
    return np.where(rng.integers(0, 2, n) == 1, np.uint64(a), np.uint64(b)).astype(np.uint64)


def gen_one_key(k, n, seed=6):
    rng = np.random.default_rng([seed, k, n])
    return np.full(n, rand_key(rng, 2 * k), dtype=np.uint64)


def gen_sorted(k, n, descending=False, seed=7):
    keys = np.sort(gen_uniform(k, n, seed))
    return keys[::-1].copy() if descending else keys


def gen_all_ones(n, seed=8):
    """k = 32: the key 2^64 - 1 makes up half the array"""
    rng = np.random.default_rng([seed, n])
    keys = rand_bits(rng, n, 64)
    keys[rng.permutation(n)[:n // 2]] = np.uint64(2 ** 64 - 1)
    return keys


def gen_in_range(k, n, kmin, kmax, seed=9):
    """keys uniform in [kmin, kmax], both ends present (n >= 2, or a one-key range)"""
    rng = np.random.default_rng([seed, k, n, kmin & 0xFFFFFFFF, kmin >> 32, kmax & 0xFFFFFFFF, kmax >> 32])
    keys = rng.integers(kmin, kmax, n, dtype=np.uint64, endpoint=True)
    keys[rng.integers(0, n // 2)] = np.uint64(kmin)
    keys[n // 2 + rng.integers(0, n - n // 2)] = np.uint64(kmax)
    return keys


def shared_bits(k, kmin, kmax):
    """leading bits, of the 2k key bits, that the two bounds share"""
    return 2 * k - ((kmin ^ kmax) & key_mask(k)).bit_length()


def fixed_values(k):
    """the shared-bit counts of section 3: the ends of 0 .. 2k and both sides of rem = 10 and rem = 20"""
    b = 2 * k
    return sorted({f for f in (0, 1, 2, 3, b - 21, b - 20, b - 19, b - 11, b - 10, b - 9, b - 1, b) if 0 <= f <= b})


def range_unaligned(k, fixed, seed=10):
    """a random prefix of `fixed` bits; kmin = prefix 0 1 ..., kmax = prefix 1 0 ... (the rest random): the ends differ in
    exactly the first free bit and the range is not the prefix's whole block"""
    rng = np.random.default_rng([seed, k, fixed])
    free = 2 * k - fixed
    base = rand_key(rng, fixed) << free
    if free == 0:
        return base, base
    if free == 1:
        return base, base | 1
    return (base | (0b01 << (free - 2)) | rand_key(rng, free - 2),
            base | (0b10 << (free - 2)) | rand_key(rng, free - 2))


def range_aligned(k, fixed, seed=10):
    """the whole block of the same prefix: prefix 00...0 .. prefix 11...1"""
    rng = np.random.default_rng([seed, k, fixed])
    free = 2 * k - fixed
    base = rand_key(rng, fixed) << free
    return base, base | ((1 << free) - 1)


def range_widened(k, kmin, kmax):
    """the aligned block that shares one leading bit less than [kmin, kmax] (None when they share none)"""
    fixed = shared_bits(k, kmin, kmax)
    if fixed == 0:
        return None
    free = 2 * k - fixed + 1
    base = (kmin & key_mask(k)) >> free << free
    return base, base | ((1 << free) - 1)


def test_generators_keep_their_promises():
    for k in range(1, 33):
        mask = key_mask(k)
        # (the shapes run at N_LARGE for these k only; uniform runs at both sizes for every k)
        for n in (N_SMALL, N_LARGE) if k in (1, 6, 10, 11, 16, 21, 32) else (N_SMALL,):
            shapes = [gen_uniform(k, n), gen_dominant(k, n, 0.5), gen_dominant(k, n, 0.99), gen_two_keys(k, n),
                      gen_one_key(k, n), gen_sorted(k, n), gen_sorted(k, n, True)]
            for keys in shapes:
                assert keys.dtype == np.uint64 and len(keys) == n and int(keys.max()) <= mask
            assert np.all(shapes[5][1:] >= shapes[5][:-1]) and np.all(shapes[6][1:] <= shapes[6][:-1])
            assert np.array_equal(np.sort(shapes[5]), np.sort(shapes[6]))
            assert len(np.unique(shapes[3])) == 2 and len(np.unique(shapes[4])) == 1
            for f, keys in ((0.5, shapes[1]), (0.99, shapes[2])):
                assert int(np.unique(keys, return_counts=True)[1].max()) >= int(n * f)
            for b in (0, 1, 9, 10, 11, 19, 20, 21):
                if b > 2 * k:
                    continue
                keys = gen_low_bits(k, n, b)
                assert keys.dtype == np.uint64 and len(keys) == n and int(keys.max()) <= mask
                assert len(np.unique(keys >> np.uint64(b))) == 1                            # they differ in the low b bits only
                assert len(np.unique(keys)) >= min(1 << b, 64)
            for b in (1, 10, 11):
                if b > 2 * k:
                    continue
                keys = gen_high_bits(k, n, b)
                assert keys.dtype == np.uint64 and len(keys) == n and int(keys.max()) <= mask
                assert len(np.unique(keys & np.uint64((1 << (2 * k - b)) - 1))) == 1       # the low part is constant
                assert len(np.unique(keys)) >= min(1 << b, 64)
        assert int(gen_uniform(k, N_LARGE).max()) <= mask
    ones = gen_all_ones(N_LARGE)
    assert int((ones == np.uint64(2 ** 64 - 1)).sum()) >= N_LARGE // 2
    for k in (5, 10, 11, 16, 21, 31, 32):
        mask = key_mask(k)
        assert {0, 2 * k} <= set(fixed_values(k))
        for fixed in fixed_values(k):
            ua, al = range_unaligned(k, fixed), range_aligned(k, fixed)
            if fixed < 2 * k - 1:
                assert al[0] < ua[0] < ua[1] < al[1]            # inside the block, not aligned to it
            for kmin, kmax in (ua, al):
                assert 0 <= kmin <= kmax <= mask
                assert shared_bits(k, kmin, kmax) == fixed
                wide = range_widened(k, kmin, kmax)
                if fixed:
                    assert wide[0] <= kmin and kmax <= wide[1] <= mask and shared_bits(k, *wide) == fixed - 1
                else:
                    assert wide is None
                for n in (100, N_SMALL):
                    keys = gen_in_range(k, n, kmin, kmax)
                    assert keys.dtype == np.uint64 and len(keys) == n
                    assert int(keys.min()) == kmin and int(keys.max()) == kmax
    # the two k = 32 ranges around the top key bit
    assert shared_bits(32, 2 ** 63 - 1, 2 ** 63) == 0 and shared_bits(32, 2 ** 63, 2 ** 64 - 1) == 1
    keys = gen_in_range(32, 100, 2 ** 63 - 1, 2 ** 63)
    assert set(int(x) for x in np.unique(keys)) == {2 ** 63 - 1, 2 ** 63}


# ------------------------------------------------------------------ the device side

class KeyBuffer:
    """one device buffer for the key arrays of a test: a count uses its keys as scratch, so every call uploads again"""

    def __init__(self, ctx, n_max):
        self.ctx = ctx
        self.ptr = ctx.buffer_alloc(max(n_max, 1) * 8)

    def count(self, keys, k):
        self.ctx.upload_u64(self.ptr, keys)
        return self.ctx.count_keys_device(self.ptr, len(keys), k)

    def count_in_range(self, keys, k, kmin, kmax):
        self.ctx.upload_u64(self.ptr, keys)
        return self.ctx.count_keys_device_in_range(self.ptr, len(keys), k, kmin, kmax)

    def free(self):
        self.ctx.buffer_free(self.ptr)


@pytest.fixture
def keybuf(ctx):
    b = KeyBuffer(ctx, 300_000)
    yield b
    b.free()


def check_count_keys(keybuf, keys, k, what):
    h = keybuf.count(keys, k)
    ok, oc = unique_u64(keys)
    check_hist(h, ok, oc, what)
    assert h.total == len(keys), what
    h.free()


# ---- section 2: dnagpu_count_keys at every k

@gpu
@pytest.mark.parametrize("k", range(1, 33))
def test_count_keys_uniform_every_k(keybuf, k):
    for n in (N_SMALL, N_LARGE):
        check_count_keys(keybuf, gen_uniform(k, n), k, f"count_keys uniform k={k} n={n}")


@gpu
@pytest.mark.parametrize("k", [6, 10, 11, 16, 21, 32])
def test_count_keys_shapes(keybuf, k):
    n = N_LARGE
    for b in (0, 1, 9, 10, 11, 19, 20, 21):
        if b <= 2 * k:
            check_count_keys(keybuf, gen_low_bits(k, n, b), k, f"count_keys low_bits({b}) k={k}")
    for b in (1, 10, 11):
        check_count_keys(keybuf, gen_high_bits(k, n, b), k, f"count_keys high_bits({b}) k={k}")
    for f in (0.5, 0.99):
        check_count_keys(keybuf, gen_dominant(k, n, f), k, f"count_keys dominant({f}) k={k}")
    check_count_keys(keybuf, gen_two_keys(k, n), k, f"count_keys two_keys k={k}")
    check_count_keys(keybuf, gen_one_key(k, n), k, f"count_keys one_key k={k}")
    check_count_keys(keybuf, gen_sorted(k, n), k, f"count_keys sorted k={k}")
    check_count_keys(keybuf, gen_sorted(k, n, True), k, f"count_keys sorted descending k={k}")
    if k == 32:
        check_count_keys(keybuf, gen_all_ones(n), k, "count_keys all_ones")
    check_count_keys(keybuf, gen_uniform(k, 1), k, f"count_keys n=1 k={k}")
    for h in (keybuf.count(np.zeros(0, dtype=np.uint64), k), keybuf.ctx.count_keys_device(None, 0, k)):
        check_hist(h, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), f"count_keys n=0 k={k}")
        assert h.total == 0 and h.distinct == 0
        h.free()


# ---- section 3: dnagpu_count_keys_in_range at the edges of `fixed`

def check_in_range(keybuf, keys, k, kmin, kmax, what):
    """the in-range count = np.unique = dnagpu_count_keys, and unchanged under a wider promise"""
    ok, oc = unique_u64(keys)
    h = keybuf.count_in_range(keys, k, kmin, kmax)
    gk, gc = check_hist(h, ok, oc, what)
    assert h.total == len(keys), what
    h.free()
    wider = [("count_keys", None), ("full range", (0, key_mask(k)))]
    wide = range_widened(k, kmin, kmax)
    if wide is not None:
        wider.append(("one bit wider", wide))
    for name, r in wider:
        h = keybuf.count(keys, k) if r is None else keybuf.count_in_range(keys, k, r[0], r[1])
        wk, wc = h.download()
        assert_same(wk, gk, f"{what}: {name} keys")
        assert_same(wc, gc, f"{what}: {name} counts")
        assert h.total == len(keys) and h.distinct == len(gk) and (h.is_sorted or not len(gk)), f"{what}: {name}"
        h.free()


@gpu
@pytest.mark.parametrize("k", [5, 10, 11, 16, 21, 31, 32])
def test_count_keys_in_range_fixed_edges(keybuf, k):
    for fixed in fixed_values(k):
        ranges = {range_unaligned(k, fixed), range_aligned(k, fixed)}       # (the same range at fixed >= 2k - 1)
        for kmin, kmax in sorted(ranges):
            assert shared_bits(k, kmin, kmax) == fixed
            for n in (100, N_SMALL, 300_000):
                check_in_range(keybuf, gen_in_range(k, n, kmin, kmax), k, kmin, kmax,
                               f"in_range k={k} fixed={fixed} [{kmin:#x}, {kmax:#x}] n={n}")


@gpu
def test_count_keys_in_range_top_bit_of_k32(keybuf):
    k = 32
    cases = [(2 ** 63 - 1, 2 ** 63),                           # spans the top bit: free_bits == 64
             (2 ** 63, 2 ** 64 - 1),                           # both ends in the top half, the whole half
             (2 ** 63 + 12345, 2 ** 64 - 1 - 54321),           # ... and unaligned
             (0, 2 ** 64 - 1),
             (2 ** 64 - 1, 2 ** 64 - 1)]                       # the one-key range of the all-ones key
    for kmin, kmax in cases:
        for n in (100, N_SMALL, 300_000):
            check_in_range(keybuf, gen_in_range(k, n, kmin, kmax), k, kmin, kmax, f"in_range k=32 [{kmin:#x}, {kmax:#x}] n={n}")


@gpu
@pytest.mark.parametrize("k", [5, 10, 11, 16, 21, 31])
def test_count_keys_in_range_ignores_bound_bits_above_2k(keybuf, k):
    """include/dnagpu.h: bits of the two bounds above the 2k key bits are ignored"""
    junk = ((1 << 64) - 1) ^ key_mask(k)
    for fixed in (0, 2 * k - 10, 2 * k - 1, 2 * k):
        kmin, kmax = range_unaligned(k, fixed)
        for n in (100, 300_000):
            keys = gen_in_range(k, n, kmin, kmax)
            ok, oc = unique_u64(keys)
            for jmin, jmax in ((junk, junk), (junk & (junk << 1), junk)):        # (key_min <= key_max as 64-bit values)
                h = keybuf.count_in_range(keys, k, kmin | jmin, kmax | jmax)
                check_hist(h, ok, oc, f"in_range k={k} fixed={fixed} n={n} bounds with high bits")
                h.free()


@gpu
def test_count_keys_in_range_arguments(keybuf, pkg):
    ctx = keybuf.ctx
    keys = gen_uniform(16, 1000)
    ctx.upload_u64(keybuf.ptr, keys)
    with pytest.raises(pkg.DnaGpuError) as ei:
        ctx.count_keys_device_in_range(keybuf.ptr, len(keys), 16, 5, 4)         # key_min > key_max
    assert ei.value.code == ERR_BAD_ARG
    for k in (0, 33):
        with pytest.raises(pkg.DnaGpuError) as ei:
            ctx.count_keys_device_in_range(keybuf.ptr, len(keys), k, 0, 3)
        assert ei.value.code == ERR_INVALID_K
        with pytest.raises(pkg.DnaGpuError) as ei:
            ctx.count_keys_device(keybuf.ptr, len(keys), k)
        assert ei.value.code == ERR_INVALID_K
    empty = np.zeros(0, dtype=np.uint64)
    for k in (1, 16, 32):
        for ptr in (keybuf.ptr, None):
            h = ctx.count_keys_device_in_range(ptr, 0, k, 0, key_mask(k))
            check_hist(h, empty, empty, f"in_range n=0 k={k}")
            assert h.total == 0 and h.distinct == 0
            h.free()
    # both entry points record k: their histograms merge
    for k in (5, 16, 32):
        kmin, kmax = range_unaligned(k, 3)
        keys = gen_in_range(k, 50_000, kmin, kmax)
        ha = keybuf.count_in_range(keys, k, kmin, kmax)
        hb = keybuf.count(keys, k)
        hm = ha.merge(hb)
        ok, oc = unique_u64(keys)
        mk, mc = hm.download()
        order = np.argsort(mk, kind="stable")
        assert_same(mk[order], ok, f"merge k={k} keys")
        assert_same(mc[order], 2 * oc, f"merge k={k} counts")
        hk = keybuf.count(gen_uniform(k + 1 if k < 32 else 31, 1000), k + 1 if k < 32 else 31)
        with pytest.raises(pkg.DnaGpuError) as ei:
            ha.merge(hk)                                                            # (another k is still refused)
        assert ei.value.code == ERR_BAD_ARG
        for h in (ha, hb, hm, hk):
            h.free()


# ---- section 4: the owner paths at every k

def owner_of(keys, k, n_owners):
    """include/dnagpu.h: owner o owns the keys whose top `bits` bits d satisfy (d * n_owners) >> bits == o"""
    bits = min(2 * k, 10)
    return ((keys >> np.uint64(2 * k - bits)) * np.uint64(n_owners)) >> np.uint64(bits)


def check_owned(ctx, d, keys, k, n_owners, what):
    owner = owner_of(keys, k, n_owners)
    all_k, all_c = [], []
    for o in range(n_owners):
        h = ctx.count_kmers_owned(d, k, o, n_owners)          # (an owner of no digit: DNAGPU_OK and an empty histogram)
        mine = keys[owner == o]
        ok, oc = orc.count_keys(mine)
        gk, gc = check_hist(h, ok, oc, f"{what} owner {o}/{n_owners}")
        assert h.total == len(mine), f"{what} owner {o}/{n_owners}: total"
        all_k.append(gk)
        all_c.append(gc)
        h.free()
    fk, fc = orc.count_keys(keys)
    assert_same(np.concatenate(all_k), fk, f"{what} {n_owners} owners concatenated = global keys")
    assert_same(np.concatenate(all_c), fc, f"{what} {n_owners} owners concatenated = global counts")


OWNER_COUNTS = (2, 3, 5, 7, 8)


@gpu
@pytest.mark.parametrize("k", range(1, 33))
def test_count_kmers_owned_every_k(ctx, k):
    for n in (60_001, 100):
        d = ctx.synth(0x0E0 + k, n)
        keys = orc.generate_kmers(d.download(), n, k, faithful=False)
        for n_owners in OWNER_COUNTS:                          # (k = 1: 4 digits, k = 2: 16: owners that own none)
            check_owned(ctx, d, keys, k, n_owners, f"owned k={k} n={n}")
        d.free()


@gpu
@pytest.mark.parametrize("k", [4, 9, 10, 20])
def test_count_kmers_owned_repeat_rich(ctx, k):
    n = 60_001
    d = ctx.synth(0x0E7, n, motif_len=7)
    keys = orc.generate_kmers(d.download(), n, k, faithful=False)
    for n_owners in OWNER_COUNTS:
        check_owned(ctx, d, keys, k, n_owners, f"owned motif 7 k={k}")
    d.free()


@gpu
@pytest.mark.parametrize("k", range(6, 33))
def test_partition_kmers_every_k(ctx, shard_math, k):
    n = 60_001
    d = ctx.synth(0x9A0 + k, n)
    keys = orc.generate_kmers(d.download(), n, k, faithful=False)
    for first, count in ((0, len(keys)), (13, 40_000)):
        sub = np.sort(keys[first:first + count])
        for n_owners in (1, 2, 3, 5, 8, 1024):
            what = f"partition k={k} rows [{first}, +{count}) {n_owners} owners"
            ptr, offs = ctx.partition_kmers(d, k, first, count, n_owners)
            offs = offs.astype(np.int64)
            assert int(offs[0]) == 0 and int(offs[-1]) == count and np.all(np.diff(offs) >= 0), what
            # the oracle's slices: owners hold contiguous ascending key ranges, so they are slices of the sorted keys
            want_offs = np.concatenate(([0], np.cumsum(np.bincount(owner_of(sub, k, n_owners).astype(np.int64),
                                                                   minlength=n_owners))))
            assert_same(offs, want_offs, what + " offsets")
            got = ctx.download_u64(ptr, count)
            slot_owner = np.repeat(np.arange(n_owners, dtype=np.uint64), np.diff(offs))
            assert_same(owner_of(got, k, n_owners), slot_owner, what + " owner of every slot")
            assert_same(np.sort(got), sub, what + " keys as a multiset")
            # every slice counted on the device, with the owner's key range as the promise: 2k - 10 (or fewer) free bits
            for o in range(n_owners):
                lo, hi = int(offs[o]), int(offs[o + 1])
                kmin, kmax = shard_math.owner_key_range(k, o, n_owners)
                h = ctx.count_keys_device_in_range(C.c_void_p(ptr + lo * 8), hi - lo, k, kmin, kmax)
                ok, oc = unique_u64(sub[lo:hi])
                if hi > lo:
                    assert kmin <= int(ok[0]) and int(ok[-1]) <= kmax
                check_hist(h, ok, oc, f"{what} owner {o} slice")
                h.free()
            ctx.buffer_free(ptr)
    d.free()


@gpu
def test_partition_kmers_arguments(ctx, pkg):
    n = 60_001
    d = ctx.synth(0x9A0, n)
    ctx.set_profiling(True)
    try:
        h = ctx.count_kmers(d, 16)
        h.free()
        phases = ctx.last_phase_times()
        assert any(name == "leaves" for name, _ in phases)
        offs = np.full(1027, 77, dtype=np.uint64)
        po = offs.ctypes.data_as(C.POINTER(C.c_uint64))
        before = ctx.device_bytes()
        for k in range(1, 6):                                  # the whole key is the owner digit: refused, nothing done
            for count in (n - k + 1, 100, 0):
                ptr = C.c_void_p()
                rc = pkg.lib().dnagpu_partition_kmers(ctx.h, d.h, k, 0, count, 2, C.byref(ptr), po)
                assert rc == ERR_BAD_ARG and not ptr.value, f"k={k} count={count}: rc {rc}"
        assert ctx.device_bytes() == before
        assert ctx.last_phase_times() == phases                # no profiling interval was opened by the refused calls
        for n_owners in (0, 1025, -1):
            ptr = C.c_void_p()
            rc = pkg.lib().dnagpu_partition_kmers(ctx.h, d.h, 16, 0, 1000, n_owners, C.byref(ptr), po)
            assert rc == ERR_BAD_ARG and not ptr.value, f"n_owners={n_owners}: rc {rc}"
        for k in (0, 33):
            ptr = C.c_void_p()
            rc = pkg.lib().dnagpu_partition_kmers(ctx.h, d.h, k, 0, 1000, 2, C.byref(ptr), po)
            assert rc == ERR_INVALID_K and not ptr.value
        # and the next count is timed as usual
        h = ctx.count_kmers(d, 16)
        h.free()
        assert [name for name, _ in ctx.last_phase_times()] == [name for name, _ in phases]
    finally:
        ctx.set_profiling(False)
    d.free()


# ---- section 5: dnagpu_count_kmers over a plain sequence at every k

def expected_engine(n_bases, k, rows):
    """Which engine counts `rows` rows of k-mers (dense_pays, csrc/count_host.hip), written out case by case so that a moved
    threshold fails here instead of moving the sweep off the tree: the dense table takes k = 1 of the whole 6145-base
    sequence (every other case there has at most LEAF_CAP rows: one leaf), k <= 5 at 6211 bases and k <= 7 at 200 003."""
    dense_k = {N_SMALL: 1 if rows > LEAF_CAP else 0, 6211: 5, N_LARGE: 7}[n_bases]
    return "dense_count" if k <= dense_k else "leaves"


@gpu
@pytest.mark.parametrize("k", range(1, 33))
def test_count_kmers_sequence_every_k(ctx, k):
    ctx.set_profiling(True)
    try:
        # 6145 bases: at most LEAF_CAP rows from k = 2 on; 6211: just above it in every case; 200 003: many tiles
        for n in (N_SMALL, 6211, N_LARGE):
            d = ctx.synth(0x5E0 + k, n)
            words = d.download()
            rows = n - k + 1
            for first, count in ((0, rows), (13, rows - 29)):
                what = f"count_kmers k={k} n={n} rows [{first}, +{count})"
                h = ctx.count_kmers(d, k, first, count)
                names = [name for name, _ in ctx.last_phase_times()]
                ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, first, count, faithful=False))
                check_hist(h, ok, oc, what)
                assert h.total == count, what
                h.free()
                engine = expected_engine(n, k, count)
                other = "leaves" if engine == "dense_count" else "dense_count"
                assert engine in names and other not in names, f"{what}: phases {names}, expected the {engine} engine"
                if engine == "leaves" and count > LEAF_CAP:
                    assert "level0_hist" in names, f"{what}: phases {names}: no level ran over the sequence"
            d.free()
    finally:
        ctx.set_profiling(False)
