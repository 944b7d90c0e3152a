"""The k-mer accumulator on keys placed by their hash.  splitmix64 is a bijection, so at k = 32 acc_model.place() writes the
hash a key shall have -- partition prefix, the bits under it, home slot -- and inverts it; dnagpu_count_keys turns the keys
into a histogram.  Every case runs on a plain context and on one with DNAGPU_DEBUG_POISON_POOL | DNAGPU_DEBUG_GUARD_POOL,
synchronised after every add: a read of a partition nobody wrote shows as wrong groups, a write past a bin or a staging buffer
as a broken guard band.  After EVERY add: the download sorted == numpy's groups bit for bit, distinct / total / summary() ==
the oracle's digest of them, partitions == acc_model.Model's, and the layout contract of DESIGN.md 4.9 -- in download order
the partition of the keys never decreases, and every partition holds what np.bincount says.  Before the device sees a case,
acc_model.run_model asserts that the restated host rules take the rounds the case is named for.

Which comparison a case group meets from both sides (the file and function that holds it in brackets):
  A chains, the wrap    `s = (s + 1) & (ACC_SLOTS - 1)` [acc_kernels.hip: lds_claim, acc_merge_kernel phase A] and acc_home
                        [acc_device.hpp]: 2, 97, 3584 keys of one partition and ONE home slot 0, 2047, 4000, 4095 -- one chain,
                        from 4000 and 4095 across the partition's end --, then the same keys again (phase A walks the chain), and
                        into a chain of 2000 from slot 4095 resident keys beside new ones homed at its head, inside it, past its end
  B the bound, the bins `m[0] <= ACC_BOUND` and `m[1] <= cap`, the re-bin branch `m[1] > cap && m[1] <= ACC_SLOTS && m[0] <= ACC_BOUND`
                        [dnagpu_api.hip: acc_add], `at < bin_cap` [acc_kernels.hip: acc_bin]: 3584 | 3585 keys under one 11-bit
                        prefix on a first and on a later add (eight splits with every resident key going to ONE child:
                        acc_split_kernel, new_occ), a bin of exactly cap | cap + 1 arrivals, the LAST bin at twice its size, 4096 |
                        4097 arrivals, and the dry run of acc_merge_kernel<false> (commit == 0) at occ + new == 3584 | 3585
  C the canonical add   B1 / B2a / B2b of acc_merge_kernel<true>: pairs x, rc(x) in one chain (B2a probes through slots B1 just
                        claimed), the three classes with palindromes, key 0 and the all-ones key into an empty and into a resident
                        table, and the exception its comment describes (occ + new unflipped keys > ACC_SLOTS in a dry run: B1 fills
                        LDS, claims give up); the bound pair and the classes again at k = 21
  D windows             `r >= first && r - first < count` [acc_kernels.hip: acc_gather_kernel] and the p_lo / p_hi search
                        [dnagpu_api.hip: dnagpu_acc_download]: windows that begin and end one before, at and one after every
                        partition edge of a 16-partition table and of a 4096-partition table with two partitions in use
  E readers             `occ[p] == 0` never read [acc_summary_kernel; query_kernels.hip: live(); join_kernels.hip; hits_kernels.hip]
                        and the probes of join_partition_kernel, join_direct_kernel and hits_sweep_kernel: a miss that walks a
                        3584-slot chain across the wrap to the first empty slot, hits at its head and its last slot

Left as the code has it and written into the model: the second add of A at n = 3584 grows the table although no key is new --
its bins overflow (3584 > 384 entries) while occ + arrivals = 7168 is above the bound, and only bins that fit get a dry run.
"""
import ctypes as C

import numpy as np
import pytest

import acc_model as A
import oracle as orc
from __graft_entry__ import load_package
from test_count_queries import check_queries
from test_count_ranking import check_rank
from test_kmer_join import check_join
from test_table_hits import check_hits, ref_hits, ref_select, resident

pytestmark = pytest.mark.gpu

U64 = np.uint64
U64_MAX = (1 << 64) - 1
SLOTS, BOUND = A.ACC_SLOTS, A.ACC_BOUND
CHAIN = "chain-s4095-n3584"                         # group A's longest chain: 3584 slots from 4095 across the wrap
SPARSE = "bound-first-3585"                         # 4096 partitions, 3585 groups in two of them


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctxs(pkg):
    """a plain context and one whose pool buffers are poisoned and guarded"""
    plain, poison = pkg.Context(0), pkg.Context(0)
    poison._base_debug |= pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL
    poison.set_debug(0)
    yield {"plain": plain, "poison": poison}
    plain.close()
    poison.close()


@pytest.fixture(params=["plain", "poison"])
def c(request, ctxs):
    ctx = ctxs[request.param]
    yield ctx
    ctx.set_debug(0)
    ctx.synchronize()                               # (the poisoned context: every guard band is checked here)


# ------------------------------------------------------------------ histograms, the checks after an add, the run of a case

def hist_of(c, keys, counts, k):
    rows = np.repeat(keys, counts.astype(np.int64))
    p = c.buffer_alloc(8 * len(rows))
    c.upload_u64(p, rows)
    h = c.count_keys_device(p, len(rows), k)
    c.buffer_free(p)
    assert h.distinct == len(keys) and h.total == len(rows)
    return h


def check_table(acc, ek, ec, partitions, what):
    gk, gc = acc.download()
    assert acc.distinct == len(ek), f"{what}: {acc.distinct} groups, numpy {len(ek)}"
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], ek), what + ": keys"
    assert np.array_equal(gc[order], ec), what + ": counts"
    assert acc.total == int(ec.sum(dtype=U64)), what + ": total"
    assert acc.summary() == orc.hist_summary(ek, ec), what + ": summary"
    assert acc.partitions == partitions, f"{what}: {acc.partitions} partitions, the model {partitions}"
    pbits = partitions.bit_length() - 1
    part = A.partition_of(gk, pbits)
    assert np.all(np.diff(part) >= 0), what + ": the download is not in partition order"
    assert np.array_equal(np.bincount(part, minlength=partitions), np.bincount(A.partition_of(ek, pbits), minlength=partitions)), \
        what + ": keys per partition"
    return gk, gc


def add_step(c, acc, model, step, what):
    """one Step: the model first (it asserts the rounds the step is written for), then the device, then every check"""
    parts, rounds, (ek, ec) = A.check_step(model, step, what)
    h = hist_of(c, step.keys, step.counts, model.k)
    acc.add(h, canonical=step.canonical)
    c.synchronize()                                 # (guard bands: before a later call can take a returned block again)
    h.free()
    got = check_table(acc, ek, ec, parts, f"{what}, {step.what} {rounds}")
    return rounds, got


def run_case(c, name, upto=None):
    """-> (accumulator, model, the rounds of every step, the last download)"""
    steps, k = A.steps_of(name)
    acc, model, rounds, got = c.accumulator(k), A.Model(k), [], None
    for s in steps[:upto]:
        r, got = add_step(c, acc, model, s, name)
        rounds.append(r)
    return acc, model, rounds, got


# ------------------------------------------------------------------ A: chains and the wrap

@pytest.mark.parametrize("n", [2, 97, 3584])
@pytest.mark.parametrize("s0", [0, 2047, 4000, 4095])
def test_one_chain_from_one_home_slot(c, s0, n):
    """n keys whose hashes agree in the partition (4 bits) and the home slot s0: lds_claim walks up to n - 1 occupied slots
    for every key, from 4000 (n = 97 and 3584), 4095 and, at n = 3584, 2047 past slot 4095 to slot 0; n = 3584 is also the re-bin branch of
    acc_add (384 entries a bin, 3584 arrivals, occ + arrivals at the bound).  Then the same keys with other counts: phase A
    of acc_merge_kernel finds each by walking the chain (n = 3584: see the module's last paragraph)."""
    steps, _ = A.steps_of(f"chain-s{s0}-n{n}")
    keys = steps[0].keys
    assert np.all(A.partition_of(keys, 4) == A.PART) and np.all(A.home_of(keys) == s0) and len(keys) == n
    assert (s0 + n > SLOTS) == ((s0, n) in ((2047, 3584), (4000, 97), (4000, 3584), (4095, 2), (4095, 97), (4095, 3584)))
    acc, _, rounds, _ = run_case(c, f"chain-s{s0}-n{n}")
    assert "rebin" in rounds[0] or n == 2
    acc.free()


def test_resident_and_new_keys_meet_in_one_wrapped_chain(c):
    """a chain of 2000 slots from 4095 (slots 4095, 0 .. 1998); then 500 of its keys, found by phase A's walk, beside 500
    new ones that lds_claim homes at slot 4095 (the whole chain to walk), at slot 999 (inside it) and at slot 1999, the first
    empty one -- which the claims from 4095 and 999 reach too"""
    steps, _ = A.steps_of("chain-mixed")
    chain, mixed = steps[0].keys, steps[1].keys
    res = np.isin(mixed, chain)
    assert int(res.sum()) == 500 and np.all(A.partition_of(mixed, 4) == A.PART)
    assert np.bincount(A.home_of(mixed[~res]), minlength=SLOTS)[[4095, 999, 1999]].tolist() == [167, 167, 166]
    acc, _, _, _ = run_case(c, "chain-mixed")
    acc.free()


# ------------------------------------------------------------------ B: the bound and the bins

@pytest.mark.parametrize("name", ["bound-first-3584", "bound-first-3585", "bound-later-584", "bound-later-585"])
def test_the_bound_under_an_11_bit_prefix(c, name):
    """keys that share exactly 11 hash bits, so one partition of 16 receives them all: 3584 (first add, or 3000 + 584) end at
    ACC_BOUND and commit after a re-bin; one more and `m[0] <= ACC_BOUND` fails, the table grows a bit a round from 4 bits to
    12 -- at every split acc_split_kernel sends all keys of the parent to one child and writes new_occ = 0 for the other --
    until bit 12 parts them"""
    steps, _ = A.steps_of(name)
    allk = np.concatenate([s.keys for s in steps])
    assert all(len(np.unique(A.partition_of(allk, b))) == 1 for b in range(4, 12)) and len(np.unique(A.partition_of(allk, 12))) == 2
    acc, model, rounds, _ = run_case(c, name)
    assert rounds[-1].count("grow") == (8 if len(allk) > BOUND else 0)
    if len(allk) == BOUND:
        assert int(model.occ().max()) == BOUND
    acc.free()


@pytest.mark.parametrize("name", ["bin-edge-1568", "bin-edge-1569", "bin-drop-last", "slots-4096", "slots-4097"])
def test_a_bin_at_its_edge_and_past_it(c, name):
    """20 000 keys over 16 partitions give bins of 1568 entries: a partition that receives 1568 commits at once, 1569 takes the
    re-bin branch of acc_add (the one entry with `at == bin_cap` is dropped by acc_bin, the second binning has 1600); 3000 in
    the LAST partition drop 1432 entries at the very end of the bins.  4096 | 4097 arrivals in one partition (m[1] <= ACC_SLOTS
    holds | fails; both are past the bound): the table grows and every group is there"""
    steps, _ = A.steps_of(name)
    arrivals = np.bincount(A.partition_of(steps[0].keys, 4), minlength=16)
    want = {"bin-edge-1568": (A.EDGE, 1568), "bin-edge-1569": (A.EDGE, 1569), "bin-drop-last": (15, 3000), "slots-4096": (A.EDGE, 4096),
            "slots-4097": (A.EDGE, 4097)}[name]
    assert (int(arrivals.argmax()), int(arrivals.max())) == want
    if name.startswith("bin"):
        assert A.bin_cap(20_000, 4) == 1568 and len(steps[0].keys) == 20_000
    acc, _, _, _ = run_case(c, name)
    acc.free()


@pytest.mark.parametrize("r", [416, 415])
def test_the_dry_run_decides_at_the_bound(c, r):
    """2000 keys resident in partition 9 of 16; 2000 arrivals a partition fit the bins (2400), occ + arrivals = 4000 is past the
    bound, so acc_add asks acc_merge_kernel<false> (commit == 0) how many are new: with r = 416 resident occ + new is 3584 and
    the add commits into 16 partitions, with 415 it is 3585 and the table grows to 32 first"""
    steps, _ = A.steps_of(f"dry-edge-{r}")
    res, arr = steps[0].keys, steps[1].keys
    mine = A.partition_of(arr, 4) == A.PART
    assert np.bincount(A.partition_of(arr, 4)).tolist() == [2000] * 16 and A.bin_cap(32_000, 4) == 2400
    assert int(np.isin(arr[mine], res).sum()) == r and 2000 + 2000 - r == (BOUND if r == 416 else BOUND + 1)
    acc, _, rounds, _ = run_case(c, f"dry-edge-{r}")
    assert rounds[1][0] == "dry"
    acc.free()


# ------------------------------------------------------------------ C: the canonical add

def test_canonical_pairs_in_one_chain(c):
    """800 canonical keys of one partition and home slot 4000 (the chain wraps), each arriving as x and as rc(x): B1 claims the
    800 slots, B2a finds every flipped arrival's key by walking through slots B1 just claimed and adds to it: 800 new keys,
    not 1600, each count(x) + count(rc x)"""
    steps, _ = A.steps_of("pairs-chain")
    canon = A.canonical_np(steps[0].keys, 32)
    assert len(np.unique(canon)) == 800 == len(steps[0].keys) // 2 and np.all(A.home_of(canon) == 4000)
    acc, model, _, _ = run_case(c, "pairs-chain")
    assert len(model.keys) == 800
    acc.free()


@pytest.mark.parametrize("name", ["mixed-empty", "mixed-resident", "k21-mixed-empty", "k21-mixed-resident"])
def test_canonical_classes_in_one_chain(c, name):
    """900 canonical keys (k = 32: one partition, home slot 4090): 300 arrive as a pair, 300 unflipped only (B1), 300 as rc
    only (B2a misses, B2b claims); key 0 (canonical), the all-G key (flipped: C comes before G) and, at k = 32, 64 palindromes
    (unflipped, once).  Into an empty table, and into one that holds every other canonical key, where phase A adds twice for a
    resident pair.  k = 21: the keys of a 4-bit prefix found by forward search (no palindromes at an odd k)"""
    steps, k = A.steps_of(name)
    keys = steps[-1].keys
    canon = A.canonical_np(keys, k)
    flipped = canon != keys
    uniq, times = np.unique(canon, return_counts=True)
    assert int((times == 2).sum()) == 300 and len(uniq) == len(keys) - 300
    assert int(flipped.sum()) == 300 + 300 + 1 and 0 in keys and int(A.mask_of(k)) in keys
    if k == 32:
        assert int((A.rc_np(keys, 32) == keys).sum()) == 64
    acc, _, _, _ = run_case(c, name)
    acc.free()


def test_canonical_dry_run_past_the_slots(c):
    """the exception in the comment on acc_merge_kernel: 3584 canonical keys resident in partition 9 of 16, 600 new pairs for
    it and 1000 singles for every other partition.  The bins fit (1312 >= 1200), occ + arrivals = 4784 > 3584, so the dry run
    is taken -- and occ + the 600 new unflipped keys = 4184 > 4096: B1 fills LDS, the last 88 claims give up, B2a misses their
    partners.  Whatever it reports between 15 600 and 16 200 new keys, acc_bits_for(3584 + that, 5) = 5: exactly 32 partitions
    and 19 184 groups"""
    steps, _ = A.steps_of("exception")
    arr = A.canonical_np(steps[1].keys, 32)
    part = A.partition_of(arr, 4)
    assert len(arr) == 16_200 and np.bincount(part).tolist() == [1000] * 9 + [1200] + [1000] * 6 and A.bin_cap(16_200, 4) == 1312
    assert BOUND + 1200 > BOUND and BOUND + int(((arr == steps[1].keys) & (part == A.PART)).sum()) == 4184 > SLOTS
    assert A.acc_bits_for(BOUND + 15_600, 5) == A.acc_bits_for(BOUND + 16_200, 5) == 5
    acc, model, rounds, _ = run_case(c, "exception")
    assert rounds[1] == ["dry-over", "grow", "commit"] and (acc.partitions, acc.distinct) == (32, 19_184)
    acc.free()


@pytest.mark.parametrize("n", [3584, 3585])
def test_the_bound_at_k_21(c, n):
    """the bound pair of B with keys below 4^21 that share a 6-bit prefix: 3584 commit into 16 partitions after a re-bin, 3585
    grow to 128"""
    acc, _, rounds, _ = run_case(c, f"k21-bound-{n}")
    assert rounds[0].count("grow") == (0 if n == 3584 else 3)
    acc.free()


# ------------------------------------------------------------------ D: windows of the download

def raw_download(pkg, c, acc, first, count, want_keys=True, want_counts=True):
    """dnagpu_acc_download with either array NULL -> (keys | None, counts | None); a sentinel behind each array stays"""
    fill = U64(0x5A5A5A5A5A5A5A5A)
    k = np.full(count + 1, fill, dtype=U64) if want_keys else None
    n = np.full(count + 1, fill, dtype=U64) if want_counts else None
    ptr = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in (k, n)]
    assert pkg.lib().dnagpu_acc_download(c.h, acc.h, first, count, ptr[0], ptr[1]) == 0
    for a in (k, n):
        assert a is None or a[count] == fill
    return (None if k is None else k[:count]), (None if n is None else n[:count])


@pytest.mark.parametrize("name", [SPARSE, "bin-edge-1568"])
def test_windows_at_every_partition_edge(c, pkg, name):
    """pre = the cumulative groups per partition (numpy): windows that begin at pre[p] - 1, pre[p], pre[p] + 1 and end at
    pre[p + 1] - 1, pre[p + 1], pre[p + 1] + 1 for every partition in use -- the first and the last group a workgroup of
    acc_gather_kernel keeps, and the partitions dnagpu_acc_download's binary searches pick (4096 partitions: all but two hold
    nothing and were never written) --, windows of one at both ends, the whole; keys only and counts only give the same"""
    acc, model, _, (gk, gc) = run_case(c, name)
    P, D = acc.partitions, acc.distinct
    per = np.bincount(A.partition_of(model.keys, P.bit_length() - 1), minlength=P)
    pre = np.concatenate([[0], np.cumsum(per)])
    wins = {(0, 1), (D - 1, 1), (0, D)}
    for p in np.flatnonzero(per):
        for a in (pre[p] - 1, pre[p], pre[p] + 1):
            for b in (pre[p + 1] - 1, pre[p + 1], pre[p + 1] + 1):
                if 0 <= a < b <= D:
                    wins.add((int(a), int(b - a)))
    assert len(wins) >= (2 * 9 - 4 if name == SPARSE else 16 * 9 - 4)
    for first, count in sorted(wins):
        what = f"{name}: window ({first}, {count})"
        k1, n1 = acc.download(first, count)
        c.synchronize()
        k2, _ = raw_download(pkg, c, acc, first, count, want_counts=False)
        c.synchronize()
        _, n3 = raw_download(pkg, c, acc, first, count, want_keys=False)
        c.synchronize()
        assert np.array_equal(k1, gk[first:first + count]) and np.array_equal(n1, gc[first:first + count]), what
        assert np.array_equal(k2, k1) and np.array_equal(n3, n1), what + ", one array NULL"
    acc.free()


# ------------------------------------------------------------------ E: the readers

def test_queries_over_a_deep_sparse_table(c, pkg):
    """the 4096-partition table of B (two partitions in use, 4094 never written) takes 3583 more keys with counts 1 .. 300 that
    fill BOTH partitions to exactly ACC_BOUND (3585 more would pass the bound and grow the table to 2^13 partitions, 512 MB):
    summary (acc_summary_kernel), spectrum, select, top and rank (query_kernels.hip: live() skips a tile whose partition has
    occ == 0) against numpy on the same groups"""
    acc, model, _, _ = run_case(c, SPARSE)
    rng = np.random.default_rng(0xE1)
    occ = model.occ()
    p0, p1 = np.flatnonzero(occ)
    assert (p0, p1) == (2 * A.PREFIX11, 2 * A.PREFIX11 + 1) and int(occ.sum()) == 3585
    more = np.concatenate([A.place(rng, BOUND - int(occ[p0]), int(p0), 12), A.place(rng, BOUND - int(occ[p1]), int(p1), 12)])
    assert len(more) == 3583 and not np.isin(more, model.keys).any()
    counts = (U64(1) + (np.arange(len(more), dtype=U64) * U64(7919)) % U64(300))
    step = A.Step("3583 more, counts to 300", rng.permutation(more), counts, rounds=["rebin", "commit"], partitions=4096)
    add_step(c, acc, model, step, "deep sparse")
    assert model.occ()[[p0, p1]].tolist() == [BOUND, BOUND]
    ok, oc = model.groups
    check_queries(acc, ok, oc, "deep sparse", pkg, bins=(256,), tops=(50,), ranges=((2, 10),))
    check_rank(acc, ok, oc, "deep sparse", pkg)
    acc.free()


@pytest.mark.parametrize("other", [SPARSE, CHAIN])
def test_join_probes_placed_tables(c, pkg, other):
    """a 16-partition accumulator of 6000 keys against the 4096-partition table (|s - t| = 8, nearly every partition of the
    finer side empty and never written), and against group A's 3584-slot chain from slot 4095, each in both roles, all three
    kinds, on the partition path, the direct path and the default choice.  A third of the 6000 keys are shared, a third
    absent, a third absent WITH the partition (and, for the chain, the home slot 4095) of the other side's keys: such a miss
    walks join_partition_kernel's / join_direct_kernel's probe over the whole chain, across the wrap, to the first empty slot"""
    ra, rmodel, _, _ = run_case(c, other, upto=1)
    rk, rc = rmodel.groups
    rng = np.random.default_rng(0xE2)
    if other == SPARSE:
        aimed = A.place(rng, 1400, 2 * A.PREFIX11, 12)
    else:
        aimed = A.place(rng, 1400, A.PART, 4, home=4095)
        assert np.all(A.home_of(rk) == 4095) and len(rk) == 3584 and np.all(A.partition_of(rk, 4) == A.PART)
    shared = rng.permutation(rk)[:1800]
    absent = rng.integers(0, 1 << 64, 2800, dtype=U64)
    lkeys = rng.permutation(np.concatenate([shared, aimed, absent]))
    assert len(np.unique(lkeys)) == 6000 and int(np.isin(lkeys, rk).sum()) == 1800
    la, lmodel = c.accumulator(32), A.Model(32)
    add_step(c, la, lmodel, A.Step("the 6000", lkeys, A.counts_for(rng, 6000), rounds=["rebin", "commit"], partitions=16), "join left")
    left, right = lmodel.groups, (rk, rc)
    for flag in (pkg.DEBUG_JOIN_PARTITION, pkg.DEBUG_JOIN_DIRECT, 0):
        c.set_debug(flag)
        for kind in (pkg.JOIN_INNER, pkg.JOIN_ANTI, pkg.JOIN_LEFT):
            st = check_join(la, ra, left, right, kind, f"6000 x {other}, kind {kind}, flag {flag}")
            assert st[0] == (1800, 4200, 6000)[kind]
            st = check_join(ra, la, right, left, kind, f"{other} x 6000, kind {kind}, flag {flag}")
            assert st[0] == (1800, len(rk) - 1800, len(rk))[kind]
        c.synchronize()
    c.set_debug(0)
    la.free()
    ra.free()


def table_of_keys(keys):
    """one sequence of exactly 32 bases per key: the packed word of sequence i is key i -> texts"""
    words = np.ascontiguousarray(keys, dtype=U64)
    starts = np.arange(len(keys) + 1, dtype=U64) * U64(32)
    assert np.array_equal(orc.generate_kmers_table(words, starts, 32), words)
    text = orc.dna_decode(words, 32 * len(keys))
    return [text[32 * i:32 * i + 32] for i in range(len(keys))]


def check_selects(c, dna, acc, ref, what, **kw):
    rows, hits = ref
    with c.table_hits(dna, acc, **kw) as sh:
        for lo, hi, frac in ((1, U64_MAX, (0, 1)), (0, 0, (0, 1)), (0, U64_MAX, (1, 1))):
            seq, r, h, n = sh.select(lo, hi, frac)
            want = ref_select(0, rows, hits, lo, hi, *frac)
            assert n == len(want[0]) and all(np.array_equal(a, b) for a, b in zip((seq, r, h), want)), f"{what}: select {lo, hi, frac}"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_hits_probe_a_wrapped_chain(c, n):
    """n sequences of one row each against group A's chain of 3584 slots from slot 4095: the key at the chain's head (slot
    4095: the partition's last key in download order), at slot 0, in its middle and in its last slot (the one before the
    partition's last key) and random ones -- hits_sweep_kernel's probe finds each by walking from slot 4095 --; absent keys
    with the chain's partition and home (the walk ends at the first empty slot, 3584 probes on); absent keys of a partition
    with occ == 0, whose slots were never written and are never read.  All groups, then counts 2 .. 3 only, which cut the
    present keys in two; hits per sequence, totals and select against the numpy reference"""
    acc, model, _, (gk, gc) = run_case(c, CHAIN, upto=1)
    sk, sc = model.groups
    rng = np.random.default_rng(0xE3 + n)
    m = n // 3 + 1
    marks = gk[[-1, 0, len(gk) // 2, -2]]
    present = np.concatenate([marks, np.setdiff1d(rng.permutation(sk)[:m + 4], marks)])[:m]
    walkers = A.place(rng, m, A.PART, 4, home=4095)
    empty = A.place(rng, m, 3, 4)
    assert not np.isin(walkers, sk).any() and model.occ()[3] == 0 and np.isin(present, sk).all()
    keys = rng.permutation(np.concatenate([present, walkers, empty])[:n])
    n_present = int(np.isin(keys, sk).sum())
    texts = table_of_keys(keys)
    d = resident(c, texts)
    for lo, hi in ((1, U64_MAX), (2, 3)):
        ref = ref_hits(texts, 32, sk, sc, lo=lo, hi=hi)
        if n >= 63:
            assert int(ref[1].sum()) == n_present < n if lo == 1 else 0 < int(ref[1].sum()) < n_present
        check_hits(c, d, acc, texts, ref, f"{n} sequences, counts {lo} .. {hi}", min_count=lo, max_count=hi)
        check_selects(c, d, acc, ref, f"{n} sequences, counts {lo} .. {hi}", min_count=lo, max_count=hi)
    d.free()
    acc.free()


def test_hits_by_canonical_form_in_a_chain(c):
    """the table of "pairs in one chain" (800 canonical keys, home slot 4000): rows that are rc(x) of a present x hit only by
    canonical form, rows x both ways, rc(y) of an absent canonical y homed at the chain walks it to its end"""
    acc, model, _, _ = run_case(c, "pairs-chain")
    sk, sc = model.groups
    rng = np.random.default_rng(0xE4)
    y = A.place(rng, 20, A.PART, 4, home=4000, canonical=True)
    assert not np.isin(y, sk).any()
    keys = rng.permutation(np.concatenate([A.rc_np(sk[:25], 32), sk[25:45], A.rc_np(y, 32)]))
    texts = table_of_keys(keys)
    d = resident(c, texts)
    with_flag, without = ref_hits(texts, 32, sk, sc, canonical=True), ref_hits(texts, 32, sk, sc)
    assert (int(with_flag[1].sum()), int(without[1].sum())) == (45, 20)
    check_hits(c, d, acc, texts, with_flag, "canonical", canonical=True)
    check_hits(c, d, acc, texts, without, "as it is")
    check_selects(c, d, acc, with_flag, "canonical", canonical=True)
    d.free()
    acc.free()
