"""Levels 0 and 1 of the record count side by side (sk_host.hip: sk_l01_piped): the slab sweep of level 0 runs in pieces
over consecutive ranges of its chunks, and the speculative level 1 starts on a piece's records, on the context's second
stream, while the next piece is cut.  Every count here is compared group for group with the CPU oracle's, and runs twice
on one context: the second stream, its events and the pool memory must be reusable.  By itself the driver pipelines only
single sequences of 5 x 2^29 rows and more (bench.py --full checks that size against the oracle's digest); here
DNAGPU_DEBUG_SLAB0 / _SLAB0_OVERFLOW, which force the slab sweep, pipeline it at every length.

Sizes.  A level-0 chunk of a short sequence is four tiles of 8064 rows, so 3, 4 and 5 chunks are sequences of at most
96768, 129024 and 161280 rows.  The sweep has four pieces, the first ones of ceil(chunks / 4) chunks each: 3 chunks are
1 + 1 + 1 + 0 (an empty piece), 4 are one each, 5 are 2 + 2 + 1 + 0 (unequal pieces, a last piece of one chunk), 9 are
3 + 3 + 3 + 0.  Such sequences have ONE coarse bucket; the smallest sequence with two (more than 512 mid buckets of
16 x 2500 k-mers) has 20.5 million rows, which is the one larger case.

Which way a count went is read from the order of its phases: the pipelined driver plans level 1 and lays out its regions
("sk_spec1") BEFORE the first piece of level 0 ("sk_scatter0"), the unpipelined one after the sweep.
"""
import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import load_package
from test_gpu_parity import check_hist, check_hist_unordered

gpu = pytest.mark.gpu

CHUNK_ROWS = 4 * 8064                   # rows of a level-0 chunk of a short sequence (four tiles of SK_TILE_ROWS)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def phase_names(ctx):
    return [a for a, _ in ctx.last_phase_times()]


def was_piped(names):
    return "sk_spec1" in names and "sk_scatter0" in names and names.index("sk_spec1") < names.index("sk_scatter0")


def count_twice(ctx, pkg, d, k, flags, ok, oc, what, table=False):
    """the count under `flags` (on top of the forced engine), twice on the one context -> the phase names of both"""
    seen = []
    ctx.set_profiling(True)
    try:
        for rep in range(2):
            ctx.set_debug(pkg.DEBUG_FORCE_SUPERKMER | flags)
            try:
                h = ctx.count_kmers_table(d, k) if table else ctx.count_kmers_unordered(d, k)
            finally:
                ctx.set_debug(0)
            seen.append(phase_names(ctx))
            w = f"{what}, run {rep}"
            assert h.total == int(oc.sum()), w
            check_hist(h, ok, oc, w) if h.is_sorted else check_hist_unordered(h, ok, oc, w)
            h.free()
    finally:
        ctx.set_profiling(False)
    return seen


# rows -> level-0 chunks: 3 (the last a partial tile), 4 (whole tiles), 5 (the last chunk 1000 rows: a partial tile), 9
ROWS = {"3 chunks": 2 * CHUNK_ROWS + 3 * 8064 + 1266, "4 chunks": 4 * CHUNK_ROWS, "5 chunks": 4 * CHUNK_ROWS + 1000,
        "9 chunks": 8 * CHUNK_ROWS + 8064 + 77}


@gpu
@pytest.mark.parametrize("k", [31, 23])
@pytest.mark.parametrize("size", list(ROWS))
def test_piped_levels_match_oracle(ctx, pkg, size, k):
    """random sequence of 3, 4, 5 and 9 level-0 chunks: the plain pipelined path, its two fall-backs after level 1 has already
    consumed a piece -- level 0's (DNAGPU_DEBUG_SLAB0_OVERFLOW: the exact pair and a fresh level 1 over the whole sequence)
    and level 1's own (DNAGPU_DEBUG_SPEC1_OVERFLOW: the exact level over all of rec0) -- and the exact level 1, which is not
    pipelined"""
    rows = ROWS[size]
    n = rows + k - 1
    assert (rows + CHUNK_ROWS - 1) // CHUNK_ROWS == int(size[0])
    words = orc.synth_words(0x91BED + rows + k, n)
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    cases = (("piped", pkg.DEBUG_SLAB0), ("slab overflow", pkg.DEBUG_SLAB0_OVERFLOW),
             ("level 1 overflow", pkg.DEBUG_SLAB0 | pkg.DEBUG_SPEC1_OVERFLOW), ("exact level 1", pkg.DEBUG_SLAB0 | pkg.DEBUG_NO_SPEC1))
    for name, flags in cases:
        for names in count_twice(ctx, pkg, d, k, flags, ok, oc, f"{size} k={k} {name}"):
            assert "sk_sample0" in names, (name, names)
            if name == "exact level 1":
                assert not was_piped(names) and "sk_spec1" not in names and "sk_hist1" in names, (name, names)
                continue
            assert was_piped(names), (name, names)
            if name == "piped":                     # one entry per level, and no exact stage
                assert names.count("sk_scatter0") == 1 and names.count("sk_scatter1") == 1, names
                assert "sk_hist0" not in names and "sk_hist1" not in names, names
            if name == "slab overflow":
                assert "sk_hist0" in names and names.count("sk_scatter0") == 2, names
            if name == "level 1 overflow":
                assert "sk_hist0" not in names and "sk_hist1" in names, names
    d.free()


@gpu
def test_piped_levels_two_coarse_buckets(ctx, pkg):
    """the smallest sequence with two coarse buckets (two regions of rec0, each consumed piece by piece), with the slab
    sweep forced: pipelined, and the oracle's groups"""
    n, k = 21_000_000, 31
    words = orc.synth_words(0x2C0A5E, n)
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    for names in count_twice(ctx, pkg, d, k, pkg.DEBUG_SLAB0, ok, oc, "two coarse buckets"):
        assert was_piped(names) and "sk_hist0" not in names and "sk_hist1" not in names, names
    d.free()


@gpu
def test_uneven_buckets_stay_unpipelined(ctx, pkg):
    """a tiled 120-base motif (repeats), long enough for two coarse buckets: its few minimizers put 48 and 52 % of the
    records into them (tests/sk_model.py says so) -- even enough for the slab sweep (5 %), too uneven for level 1's plain
    regions (2 %), which then come from a sampled histogram of rec0 ("sk_sample1").  Level 1 therefore starts after the
    whole sweep, and the groups are the oracle's.  (A shorter sequence has one coarse bucket, which is even by
    definition.)"""
    n, k = 21_000_000, 31
    words = orc.synth_words_repeat(0xC0DE + n, n, 120)
    d = ctx.upload(words, n)
    ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, faithful=False))
    for names in count_twice(ctx, pkg, d, k, pkg.DEBUG_SLAB0, ok, oc, "motif"):
        assert "sk_sample0" in names and "sk_sample1" in names and not was_piped(names), names
    d.free()


@gpu
def test_piped_levels_table(ctx, pkg):
    """a resident table of random reads (dnagpu_count_kmers_table: level 0 skips the windows that cross a read's end), five
    level-0 chunks: pipelined under DNAGPU_DEBUG_SLAB0 (without the flag a table's sweep is not: it did not pay), and the
    oracle's groups"""
    k = 31
    n = 4 * CHUNK_ROWS + 1000 + k - 1
    rng = np.random.default_rng(0x7AB1E)
    cuts = np.unique(rng.integers(1, n, n // 180))
    starts = np.concatenate(([0], cuts, [n])).astype(np.uint64)
    words = orc.synth_words(0x7AB1E, n)
    d = ctx.upload(words, n)
    d.set_sequences(starts)
    ok, oc = orc.count_keys(orc.generate_kmers_table(words, starts, k))
    for names in count_twice(ctx, pkg, d, k, pkg.DEBUG_SLAB0, ok, oc, "table", table=True):
        assert was_piped(names), names
    d.free()
