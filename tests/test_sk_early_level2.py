"""Level 2 of the record count behind a device-side gate, and the selection of the final buckets in one wait
(sk_host.hip: sk_l1_spec_end / sk_level2, sk_tail_select / sk_tail_select_over).

The one-tile regroup of level 2 is queued right behind the speculative level 1, before the host has read level 1's verdict:
a one-workgroup kernel writes a gate word, and the regroup does nothing unless it is 0.  The gate is 0 exactly when that
regroup is all of level 2 -- the sweep(s) before it stand, no mid bucket is heavy or longer than one regroup tile, the k-mers
are the expected ones.  The regroup writes into the buffer that the exact level 1 after an overflow reads, so a gate that
let it through wrongly shows as wrong groups: every case compares group for group with the CPU oracle, twice on one context.
The host recomputes the word from what it read back and fails the call on a difference, so a count that returns has a
device verdict equal to the host's.

Which way a count went is read from its phase names: "sk_spec1" = the speculative level 1, "sk_hist1" = the exact level
(alone, or after an overflow), "sk_sample1" = regions from a sampled histogram, "sk_regroup" = a regroup that did work
(marked once per such regroup), "sk_heavy_split" = heavy mid buckets left level 1's list, "sk_count_big" = there was a big
final bucket, "sk_expand_flat" = there was an over bucket.
"""
import numpy as np
import pytest

import oracle as orc
import sk_model as M
from __graft_entry__ import load_package
from test_sk_piped_levels import CHUNK_ROWS, count_twice, was_piped

gpu = pytest.mark.gpu

SK_COUNT_CAP = 4096                     # most k-mers of a final bucket that is counted from its records (sk_count_cap)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def codes_of(words, n, first=0, count=None):
    """bases [first, first + count) of a packed sequence as 2-bit codes"""
    count = n - first if count is None else count
    w0, w1 = first // 32, (first + count + 31) // 32
    c = ((np.asarray(words[w0:w1], dtype=np.uint64)[:, None] >> (np.arange(32, dtype=np.uint64) * np.uint64(2))) & np.uint64(3)).ravel()
    return c[first - 32 * w0:first - 32 * w0 + count].astype(np.uint8)


def model_buckets(codes, k, g):
    """tests/sk_model.py over a stretch of bases: every row's (mid bucket, final bucket) and the rows that start a run of one
    minimum (a record starts at least there: tile cuts and the length limit only add records)"""
    pos, v = M.sequence_minima(codes, k)
    m = M.mlen(k)
    mid = M.d0_of(v, m, g.c0n).astype(np.int64) * g.R + M.d1_of(v, g.b1).astype(np.int64)
    fin = mid * 16 + M.d2_of(v).astype(np.int64)
    starts = np.concatenate(([True], np.diff(pos) != 0))
    return mid, fin, starts


# ---------------------------------------------------------------- gate open

@gpu
@pytest.mark.parametrize("k", [31, 23])
def test_gate_open_unpiped(ctx, pkg, k):
    """random sequence of 4 level-0 chunks, the forced engine alone (exact level 0, speculative level 1): the gate is open
    -- the speculative level stands ("sk_spec1", no "sk_hist1") and ONE regroup did work"""
    rows = 4 * CHUNK_ROWS
    n = rows + k - 1
    words = orc.synth_words(0xEA7E + k, n)
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    for names in count_twice(ctx, pkg, d, k, 0, ok, oc, f"gate open, unpiped, k={k}"):
        assert "sk_spec1" in names and "sk_hist1" not in names, names
        assert names.count("sk_regroup") == 1 and not was_piped(names), names
        assert "sk_heavy_split" not in names, names
    d.free()


@gpu
@pytest.mark.parametrize("k", [31, 23])
@pytest.mark.parametrize("rows", [4 * CHUNK_ROWS, 4 * CHUNK_ROWS + 1000], ids=["4 chunks", "5 chunks"])
def test_gate_open_piped(ctx, pkg, rows, k):
    """the same under DNAGPU_DEBUG_SLAB0 (levels 0 and 1 side by side; the gate also reads level 0's slab status), and five
    chunks with their partial last tile: piped, no exact stage, one regroup"""
    n = rows + k - 1
    words = orc.synth_words(0xEA7E + k, n)
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    for names in count_twice(ctx, pkg, d, k, pkg.DEBUG_SLAB0, ok, oc, f"gate open, piped, {rows} rows, k={k}"):
        assert was_piped(names) and "sk_hist0" not in names and "sk_hist1" not in names, names
        assert names.count("sk_regroup") == 1 and names.count("sk_scatter0") == 1 and names.count("sk_scatter1") == 1, names
    d.free()


# ---------------------------------------------------------------- gate shut

@gpu
@pytest.mark.parametrize("k", [31, 23])
def test_gate_shut_by_region_overflow(ctx, pkg, k):
    """the planted input of test_level1_speculative_and_exact_agree (4000 copies of one 64-base segment over 3 000 001 random
    bases: even coarse buckets, so the speculative sweep runs; the segment's mid buckets overflow their regions): the exact
    level follows ("sk_hist1") and reads rec0, which an early regroup would have overwritten -- the oracle's groups are the
    evidence that it did not run"""
    n = 3_000_001
    words = orc.synth_words(0xC0FFEE + n, n)
    rng = np.random.default_rng(n)
    seg = words[1000:1002].copy()
    for p in rng.integers(0, len(words) - 3, size=4000):
        words[p:p + 2] = seg
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    for names in count_twice(ctx, pkg, d, k, 0, ok, oc, f"gate shut by an overflow, k={k}"):
        assert "sk_spec1" in names and "sk_hist1" in names, names
        assert names.index("sk_spec1") < names.index("sk_hist1") < names.index("sk_regroup"), names
    d.free()


MOTIF, MOTIF_N = 120, 21_000_000


def motif_longest_mid_bucket(words, n, k):
    """the model's count of records in the fullest mid bucket of the tiled half of synth_words_repeat(.., n, MOTIF): the runs
    of one minimum in 50 periods (read 2 periods in, clear of the random half), scaled to the periods of the half"""
    g = M.geometry(n - k + 1, k, forced=True)
    periods = 50
    first = n // 2 + 2 * MOTIF
    mid, _, starts = model_buckets(codes_of(words, n, first, periods * MOTIF + k - 1), k, g)
    starts[0] = False                                       # (the stretch begins inside a run)
    per_mid = np.bincount(mid[starts], minlength=g.c0n * g.R)
    return int(per_mid.max()) * ((n - n // 2) // MOTIF - 4) // periods


@gpu
@pytest.mark.parametrize("k", [31, 23])
def test_gate_shut_by_long_mid_bucket(ctx, pkg, k):
    """the 120-base tiled motif at 21 M bases of test_uneven_buckets_stay_unpipelined: uneven coarse buckets, so level 1's
    regions come from the sampled histogram ("sk_sample1") and hold what they get -- no overflow, no "sk_hist1" -- but the
    motif's few minimizers fill mid buckets far beyond one regroup tile of 8192 records.  tests/sk_model.py: the fullest
    mid bucket of the tiled half holds at least 87 496 records at k = 31 and 174 992 at k = 23 (87 496 periods, one and two
    runs of one minimum per period in it).  The gate is shut by them; the heavy ones leave through the chunked split
    ("sk_heavy_split"), the regroup runs once, late.  By itself the driver does not launch early behind sampled regions (a
    shut gate costs time, and repeats shut it: test_uneven_buckets_stay_unpipelined counts this input that way);
    DNAGPU_DEBUG_EARLY_L2 makes it"""
    n = MOTIF_N
    words = orc.synth_words_repeat(0xC0DE + n, n, MOTIF)
    longest = motif_longest_mid_bucket(words, n, k)
    print(f"k={k}: the model's fullest mid bucket of the tiled half: {longest} records")
    assert longest > M.SKR_TILE, longest
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    for names in count_twice(ctx, pkg, d, k, pkg.DEBUG_SLAB0 | pkg.DEBUG_EARLY_L2, ok, oc, f"gate shut by a long mid bucket, k={k}"):
        assert "sk_sample1" in names and "sk_spec1" in names and "sk_hist1" not in names, names
        assert names.count("sk_regroup") == 1 and "sk_heavy_split" in names, names
        assert names.index("sk_heavy_split") < names.index("sk_regroup"), names
    d.free()


# ---------------------------------------------------------------- the selection

OVER_ROWS = 4 * CHUNK_ROWS


def over_input(k):
    """A random sequence of 4 level-0 chunks with copies of one stretch of 2k - m bases planted at every 200th base: all
    k - m + 1 k-mers of a copy share the stretch's middle m-mer as their minimum (the stretch is chosen so: a full run in the
    plain sequence), so every copy adds k - m + 1 k-mers to ONE final bucket.  Copies are added, one at a time, until the
    model (tests/sk_model.py) sees a final bucket of more than SK_COUNT_CAP k-mers: the smallest number that does.
    -> words, n, the model's k-mers per final bucket"""
    n = OVER_ROWS + k - 1
    words = orc.synth_words(0x0BE5 + k, n)
    g = M.geometry(OVER_ROWS, k, forced=True)
    codes = codes_of(words, n)
    m, w = M.mlen(k), M.window(k)
    pos, _ = M.sequence_minima(codes, k)
    run_start = np.flatnonzero(np.concatenate(([True], np.diff(pos) != 0)))
    run_len = np.diff(np.concatenate((run_start, [len(pos)])))
    r = run_start[np.flatnonzero(run_len == w)[0]]          # rows r .. r + w - 1 share the minimum at base r + w - 1
    stretch = codes[r:r + 2 * k - m].copy()
    _, fin, _ = model_buckets(codes, k, g)
    target = fin[r]
    have = int(np.count_nonzero(fin == target))
    copies = max(0, (SK_COUNT_CAP - have) // w - 2)         # (the model decides below; this only saves iterations)
    at = 0
    for c in range(copies):
        at = 1000 + 200 * c
        codes[at:at + len(stretch)] = stretch
    while True:
        _, fin, _ = model_buckets(codes, k, g)
        per_fin = np.bincount(fin, minlength=g.c0n * g.R * 16)
        if per_fin.max() > SK_COUNT_CAP:
            break
        at = 1000 + 200 * copies
        assert at + len(stretch) < n
        codes[at:at + len(stretch)] = stretch
        copies += 1
    packed = np.zeros((n + 31) // 32 * 32, dtype=np.uint64)
    packed[:n] = codes
    out = (packed.reshape(-1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(axis=1, dtype=np.uint64)
    return out, n, per_fin


@gpu
@pytest.mark.parametrize("k", [31, 23])
def test_selection_over_bucket_without_big(ctx, pkg, k):
    """no big bucket and one over bucket: the selection of the over buckets comes out of the first sweep and its one wait.
    The model's final buckets: exactly one holds more than 4096 k-mers, and none more than 8192 (from where a bucket is
    "big").  The over bucket goes through the expansion ("sk_expand_flat"); "sk_count_big" does not appear"""
    words, n, per_fin = over_input(k)
    print(f"k={k}: the model's fullest final buckets: {np.sort(per_fin)[-3:]}")
    assert np.count_nonzero(per_fin > SK_COUNT_CAP) == 1 and per_fin.max() <= 2 * SK_COUNT_CAP, np.sort(per_fin)[-3:]
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    for names in count_twice(ctx, pkg, d, k, 0, ok, oc, f"one over bucket, no big one, k={k}"):
        assert "sk_expand_flat" in names and "sk_count_big" not in names, names
        assert names.count("sk_regroup") == 1, names
    d.free()


@gpu
@pytest.mark.parametrize("k", [31, 23])
def test_selection_with_big_bucket(ctx, pkg, k):
    """a tiled 64-base motif over the second half of 2 M bases: its minimizers' final buckets are big ("sk_count_big"), so
    the second selection runs as before (it reads what sk_count_big gave up on)"""
    n = 2_000_000
    words = orc.synth_words_repeat(0xB16 + n, n, 64)
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    for names in count_twice(ctx, pkg, d, k, 0, ok, oc, f"big buckets, k={k}"):
        assert "sk_count_big" in names and "sk_count" in names, names
    d.free()
