"""Levels 1 and 2 of the record count on crafted record streams: sk_model.crafted_stream() puts a chosen number of records
into a chosen (coarse bucket, d1, d2), dnagpu_count_records counts them, and the histogram must equal np.unique of the
streams' k-mers bit for bit, the total their number, and the phase names what the restated host rules (sk_model.route,
spec_cap, heavy) predict.  global_rows only fixes the geometry (k = 31: 40 000 rows -> R = 2 mid buckets per coarse bucket,
160 000 -> 4, 10 300 000 -> 512, 21 000 000 -> 512 in two coarse buckets); the streams stay at tens of thousands of records.
Every case runs on a plain context and again on one with DNAGPU_DEBUG_POISON_POOL | DNAGPU_DEBUG_GUARD_POOL, synchronised
afterwards: a read of a region slot nobody wrote shows as a wrong histogram, a write past a region or buffer as a broken guard.

Which comparison a case group meets from both sides (the file and function that holds it in brackets):
  a region end          `p < glim[d]` and the dropped flag [sk_scatter1<SPEC>], `used > cap` [sk_spec_nodes]: a mid bucket of
                        cap - 1, cap, cap + 1 records, as digit 0, a middle digit and digit R - 1 (its region ends the buffer)
  b tiles and chunks    `n_tile == 8192` full tile / gather [sk_scatter1], chunks of four tiles [sk_chunk_len]: coarse buckets
                        of 1, 8191, 8192, 8193, 32767, 32768, 32769, 65535, 65537 records
  c skew in a tile      `cnt[tid] <= SK1_STAGE < cnt[tid + 1]` and `n_valid - cnt[tid] > SK1_STAGE` [sk_scatter1]: R = 2, tiles of
                        (4160, 4032), (4032, 4160) -- a half exactly the stage --, (4000, 4192), (4161, 4031) -- one record
                        over: the gather --, (8192, 0), (0, 8192); then four such tiles in a row (the cursors carry over)
  d NULL records        bin R of sk_scatter1 and the `m >> 63` of sk_hist1: scattered, a whole tile, a whole chunk, front, back,
                        a partial last tile, one real record among 8191
  e regroup             `nd.len > SKR_TILE`, `pos >> 12`, `nd.len == 0` [sk_regroup<false> / <true>], the wave-aggregated ranks
                        of LONG: mid buckets of 0, 1, 4095, 4096, 4097, 8191, 8192 | 8193, 16384, 16385, 24577, 65536 records
                        with one, two, all sixteen d2, every lane another d2, and runs of 64
  f heavy mid buckets   `rcn > SK_MID_RECORDS` (65536 | 65537 records), `kc > mid_limit` (forced, k = 23: 60 003 | 60 004
                        k-mers, counted by the sweep's packed 64-bit add and by sk_hist1) [sk_l1_census]; the by-d2 split behind
                        them [sk_heavy_take: sk_scatter1 without global cursors, its gpos path] at 32768 j + 1 records
  g route               sk_even's 1.02 [sk_l1_route_plain]: two coarse buckets of (20946, 20000) | (20947, 20000) records
  h key widths          b, d and the one-tile | LONG edge of e at k = 20 and k = 32 with records of lmax(k) k-mers
The input order of a stream is what a case controls; inside a mid bucket level 1 keeps it only roughly (tiles reserve their
slots in arrival order), so e's lane patterns reach sk_regroup as patterns of that kind, not record for record.
"""
import zlib

import numpy as np
import pytest

import sk_model as M
from __graft_entry__ import load_package
from test_sk_records import count_stream

pytestmark = pytest.mark.gpu

K = 31
ROWS = {2: 40_000, 4: 160_000, 512: 10_300_000}     # global_rows that give R mid buckets per coarse bucket, one coarse bucket
ROWS_TWO = 21_000_000                               # ... 512, and two coarse buckets
SHORT = (1, 3)                                      # k-mers per record where the case is about records, not k-mers
D2_ALL = tuple(range(16))


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctxs(pkg):
    """(a plain context, one whose pool buffers are poisoned and guarded)"""
    plain, poison = pkg.Context(0), pkg.Context(0)
    poison._base_debug |= pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL
    poison.set_debug(0)
    yield plain, poison
    plain.close()
    poison.close()


# ------------------------------------------------------------------ streams, predictions, the run

def seed_of(*what):
    return zlib.crc32(repr(what).encode())


def split_d2(bucket, d1, n, d2s, lengths):
    """n records of mid bucket (bucket, d1), dealt evenly over the listed d2"""
    return [(bucket, d1, d2, n // len(d2s) + (i < n % len(d2s)), lengths) for i, d2 in enumerate(d2s)]


def uniform(bucket, R, n, lengths):
    """n records of one coarse bucket, digits uniform: record i in d1 = i mod R, d2 = (i / R) mod 16"""
    i = np.arange(n)
    cnt = np.bincount((i % R) * 16 + (i // R) % 16, minlength=16 * R)
    return [(bucket, int(t) // 16, int(t) % 16, int(cnt[t]), lengths) for t in np.flatnonzero(cnt)]


class Stream:
    """a crafted stream with what the predictions need: the coarse buckets' record counts (NULL records included, as the host
    sees them) and the real records and k-mers of every mid bucket"""

    def __init__(self, k, rows, spec, *seed):
        self.k, self.rows = k, rows
        self.recs, self.bucket, self.truth = M.crafted_stream(k, spec, np.random.default_rng(seed_of(k, rows, *seed)))
        self.unique = np.unique(self.truth, return_counts=True)
        g = M.geometry(rows, k)
        d1, _, length, null = M.record_fields(self.recs)
        assert self.bucket.max() < g.c0n and (null.all() or d1[~null].max() < g.R), "the stream does not fit the geometry"
        self.n_null = int(null.sum())
        self.lens = np.bincount(self.bucket, minlength=g.n_coarse)
        mid = self.bucket[~null] * g.R + d1[~null]
        self.rc = np.bincount(mid, minlength=g.n_coarse * g.R)
        self.kc = np.bincount(mid, weights=length[~null], minlength=g.n_coarse * g.R).astype(np.int64)

    def pieces(self, p):
        start = np.concatenate([[0], np.cumsum(self.lens)])
        return [(p + 16 * int(start[b]), int(n), b) for b, n in enumerate(self.lens) if n]


def predicted(st, flags):
    """-> (phases that must occur, phases that must not), from the restated rules: the route, a region that overflows, the
    census"""
    forced = bool(flags & M.DEBUG_FORCE_SUPERKMER)
    g = M.geometry(st.rows, st.k, forced)
    must, never = {"sk_regroup"}, set()
    way = M.route(st.lens, flags, g.b1)
    if way == "Exact":
        must.add("sk_hist1")
        never |= {"sk_spec1", "sk_sample1"}
    elif way == "Speculative":
        over = any(st.rc[b * g.R:(b + 1) * g.R].max() > M.spec_cap(int(n), g.R) for b, n in enumerate(st.lens) if n)
        must.add("sk_spec1")
        never.add("sk_sample1")
        (must if over or (flags & M.DEBUG_SPEC1_OVERFLOW) else never).add("sk_hist1")
    else:
        must.add("sk_sample1")
    is_heavy = np.array([M.heavy(int(a), int(b), g.mid_limit, forced) for a, b in zip(st.kc, st.rc)])
    (must if is_heavy.any() and not (flags & M.DEBUG_HEAVY_EXPAND) else never).add("sk_heavy_split")
    if (flags & M.DEBUG_HEAVY_EXPAND) and 2 * int(st.kc[is_heavy].sum()) > int(st.kc.sum()):
        must.discard("sk_regroup")                   # (the set is skewed: levels 1-2 give up before anything moves)
        never.add("sk_regroup")
    return must, never


def run(ctxs, st, flags, what):
    """the stream through dnagpu_count_records on both contexts -> the phase names (of the plain run)"""
    must, never = predicted(st, flags)
    seen = None
    for c, name in zip(ctxs, ("plain", "poisoned")):
        c.set_debug(flags)
        try:
            phases = count_stream(c, st.recs, st.pieces, st.k, st.rows, st.truth, f"{what}, flags {flags}, {name}", profile=True,
                                  unique=st.unique)
        finally:
            c.set_debug(0)
        c.synchronize()                               # (the poisoned context: every guard band is checked here)
        assert must <= set(phases) and not (never & set(phases)), f"{what}, flags {flags}, {name}: {phases}; want {sorted(must)}, not {sorted(never)}"
        seen = seen or phases
    return seen


# ------------------------------------------------------------------ a: the region end of the speculative sweep

REGION_CASES = [(R, digit, delta) for R in (2, 4, 512) for digit in ("first", "middle", "last") for delta in (-1, 0, 1)
                if not (R == 2 and digit == "middle")]
REGION_LEN = {2: 8192, 4: 10_000, 512: 20_000}


@pytest.mark.parametrize("R,digit,delta", REGION_CASES)
def test_spec_region_end(ctxs, pkg, R, digit, delta):
    """one coarse bucket of len records, one mid bucket of spec_cap(len, R) + delta of them, the rest spread over the other
    digits: up to cap the sweep stands ("sk_spec1" without "sk_hist1"), one record more overflows the region (the exact level
    follows); with DNAGPU_DEBUG_NO_SPEC1 the exact level alone"""
    n = REGION_LEN[R]
    cap = M.spec_cap(n, R)
    d = {"first": 0, "middle": R // 2, "last": R - 1}[digit]
    others = [x for x in range(R) if x != d]
    rest = n - (cap + delta)
    assert M.geometry(ROWS[R], K).R == R and 0 < rest and rest // len(others) + 1 < cap
    groups = split_d2(0, d, cap + delta, D2_ALL, SHORT)
    for i, x in enumerate(others):
        groups += split_d2(0, x, rest // len(others) + (i < rest % len(others)), D2_ALL, SHORT)
    st = Stream(K, ROWS[R], {"groups": groups}, "a", R, digit, delta)
    assert int(st.rc[d]) == cap + delta and int(st.lens[0]) == n
    what = f"region end, R={R}, digit {d}, cap {cap} {delta:+d}"
    phases = run(ctxs, st, 0, what)
    assert "sk_spec1" in phases and ("sk_hist1" in phases) == (delta > 0), phases
    phases = run(ctxs, st, pkg.DEBUG_NO_SPEC1, what)
    assert "sk_hist1" in phases and "sk_spec1" not in phases, phases


# ------------------------------------------------------------------ b: tiles and chunks of sk_scatter1

BUCKET_LENS = [1, 8191, 8192, 8193, 32767, 32768, 32769, 65535, 65537]


@pytest.mark.parametrize("n", BUCKET_LENS)
def test_scatter1_tiles_and_chunks(ctxs, pkg, n):
    """a coarse bucket of n records, digits uniform over 512 mid buckets: a partial tile alone, full tiles, a full tile and one
    record, one chunk of four full tiles (32768), a second chunk of one record, two chunks and a record; speculative, exact"""
    assert M.chunk_len(n) == 4 * M.SK1_TILE
    st = Stream(K, ROWS[512], {"groups": uniform(0, 512, n, SHORT)}, "b", n)
    assert "sk_hist1" not in run(ctxs, st, 0, f"bucket of {n}")
    assert "sk_spec1" not in run(ctxs, st, pkg.DEBUG_NO_SPEC1, f"bucket of {n}")


# ------------------------------------------------------------------ c: skew inside a full tile (R = 2)

TILE_PAIRS = [(4160, 4032), (4032, 4160), (4000, 4192), (4161, 4031), (8192, 0), (0, 8192)]


def takes_gather(n0, n1):
    """does a full tile of n0 records of digit 0 and n1 of digit 1 take sk_scatter1's gather path?  The digit that holds
    sorted slot SK1_STAGE starts the second half; gather if the slots from its start on exceed the stage."""
    if n0 + n1 <= M.SK1_STAGE:
        return False
    start = 0 if n0 > M.SK1_STAGE else n0
    return n0 + n1 - start > M.SK1_STAGE


def test_tile_pairs_cover_both_sides():
    assert [takes_gather(*p) for p in TILE_PAIRS] == [False, False, True, True, True, True]


def pair_groups(n0, n1):
    return split_d2(0, 0, n0, D2_ALL, SHORT) + split_d2(0, 1, n1, D2_ALL, SHORT)


@pytest.mark.parametrize("order", ["shuffled", "digit"])
@pytest.mark.parametrize("n0,n1", TILE_PAIRS)
def test_scatter1_skew_one_tile(ctxs, pkg, n0, n1, order):
    """one full tile at R = 2 (cap 4680: only the one-digit tiles overflow their region), shuffled and all of digit 0 first"""
    assert M.geometry(ROWS[2], K).R == 2 and n0 + n1 == M.SK1_TILE and M.spec_cap(M.SK1_TILE, 2) == 4680
    st = Stream(K, ROWS[2], {"groups": pair_groups(n0, n1), "order": order}, "c", n0, n1)
    what = f"tile of ({n0}, {n1}), {order}"
    assert ("sk_hist1" in run(ctxs, st, 0, what)) == (max(n0, n1) > 4680)
    run(ctxs, st, pkg.DEBUG_NO_SPEC1, what)


def tile_by_tile(pairs):
    """the order that gives tile t exactly pairs[t] records of (digit 0, digit 1), shuffled inside the tile"""
    def order(bucket, d1, d2, rng):
        pool = [rng.permutation(np.flatnonzero(d1 == d)) for d in (0, 1)]
        at, out = [0, 0], []
        for pair in pairs:
            tile = np.concatenate([pool[d][at[d]:at[d] + pair[d]] for d in (0, 1)])
            out.append(rng.permutation(tile))
            at = [at[0] + pair[0], at[1] + pair[1]]
        return np.concatenate(out)
    return order


FOUR_TILES = {
    "each-edge": [(4160, 4032), (4032, 4160), (4000, 4192), (4161, 4031)],
    "gather-between": [(8192, 0), (4160, 4032), (0, 8192), (4032, 4160)],
    "stage-then-gather": [(4160, 4032), (4161, 4031), (4160, 4032), (4161, 4031)],
}


@pytest.mark.parametrize("name", sorted(FOUR_TILES))
def test_scatter1_skew_four_tiles(ctxs, pkg, name):
    """four full tiles = one chunk, every tile with its own exact pair of digit counts: the staged and the gather path take
    turns on one workgroup's cursors"""
    pairs = FOUR_TILES[name]
    n0, n1 = sum(p[0] for p in pairs), sum(p[1] for p in pairs)
    st = Stream(K, ROWS[2], {"groups": pair_groups(n0, n1), "order": tile_by_tile(pairs)}, "c4", name)
    d1 = M.record_fields(st.recs)[0]
    assert [(int((t == 0).sum()), int((t == 1).sum())) for t in d1.reshape(4, M.SK1_TILE)] == pairs
    run(ctxs, st, 0, f"four tiles, {name}")
    run(ctxs, st, pkg.DEBUG_NO_SPEC1, f"four tiles, {name}")


@pytest.mark.parametrize("n0,n1", [(4160, 4032), (4000, 4192), (8192, 0)])
def test_scatter1_skew_alternating_tiles(ctxs, pkg, n0, n1):
    """four times the pair, as tiles of ONE digit each (8192 of digit 0, 8192 of digit 1, ...): a bucket that is even overall
    with every tile maximally skewed; and the same multiset with all of digit 0 first"""
    for order in ("tiles", "digit"):
        st = Stream(K, ROWS[2], {"groups": pair_groups(4 * n0, 4 * n1), "order": order}, "c-alt", n0, n1)
        run(ctxs, st, 0, f"4 x ({n0}, {n1}), {order}")
        run(ctxs, st, pkg.DEBUG_NO_SPEC1, f"4 x ({n0}, {n1}), {order}")


# ------------------------------------------------------------------ d: NULL records

def null_cases(rng):
    """name -> (records of the coarse bucket, NULL positions)"""
    T = M.SK1_TILE
    return {
        "scattered-14%": (20_000, rng.choice(20_000, 2_800, replace=False)),
        "a-tile-of-nulls": (3 * T, np.arange(T, 2 * T)),
        "front": (12_000, np.arange(3_000)),
        "back": (12_000, np.arange(9_000, 12_000)),
        "a-chunk-of-nulls": (5 * T, np.arange(4 * T)),
        "partial-last-tile": (T + 1_000, T + rng.choice(1_000, 400, replace=False)),
        "one-real-record": (T, np.delete(np.arange(T), 5_000)),
    }


@pytest.mark.parametrize("name", sorted(null_cases(np.random.default_rng(0))))
def test_level1_drops_null_records(ctxs, pkg, name):
    """NULL records (unused slots of a slab sweep) in the coarse bucket: level 1 drops them -- they are in no mid bucket, no
    k-mer count and not in the total -- on the speculative and the exact route (never with DNAGPU_DEBUG_HEAVY_EXPAND: the
    expansion of whole coarse buckets must not meet them)"""
    n, pos = null_cases(np.random.default_rng(0xD0))[name]
    st = Stream(K, ROWS[512], {"groups": uniform(0, 512, n - len(pos), SHORT), "nulls": {0: pos}}, "d", name)
    assert st.n_null == len(pos) > 0 and int(st.lens[0]) == n and len(st.recs) == 2 * n
    assert "sk_hist1" not in run(ctxs, st, 0, f"NULL records, {name}")
    run(ctxs, st, pkg.DEBUG_NO_SPEC1, f"NULL records, {name}")


# ------------------------------------------------------------------ e: sk_regroup

ONE_TILE_MIDS = [0, 1, 4095, 4096, 4097, 8191, 8192]
LONG_MIDS = [8193, 16384, 16385, 24577]
D2_FORMS = {"d2=0": ((0,), "shuffled"), "d2=15": ((15,), "shuffled"), "two": ((3, 12), "shuffled"), "uniform": (D2_ALL, "shuffled"),
            "lanes": (D2_ALL, "lanes"), "runs64": (D2_ALL, "runs64")}


def mids_stream(sizes, form, *seed, k=K, lengths=SHORT):
    d2s, order = D2_FORMS[form]
    groups = []
    for i, n in enumerate(sizes):
        groups += split_d2(0, 5 * i + 1, n, d2s, lengths)         # (mid buckets 1, 6, 11, ...: the ones between stay empty)
    return Stream(k, ROWS[512], {"groups": groups, "order": order, "copies": 16}, "e", sizes, form, *seed)


@pytest.mark.parametrize("form", ["d2=0", "d2=15", "two", "uniform"])
def test_regroup_one_tile(ctxs, pkg, form):
    """mid buckets of 0, 1, 4095, 4096, 4097, 8191, 8192 records side by side (and 505 empty ones): the one-tile kernel alone,
    its two halves of 4096 sorted slots"""
    st = mids_stream(ONE_TILE_MIDS, form)
    assert sorted(st.rc[st.rc > 0].tolist()) == ONE_TILE_MIDS[1:] and st.rc.max() <= M.SKR_TILE
    run(ctxs, st, pkg.DEBUG_NO_SPEC1, f"one-tile mid buckets, {form}")


@pytest.mark.parametrize("form", sorted(D2_FORMS))
def test_regroup_long(ctxs, pkg, form):
    """mid buckets of 8193, 16384, 16385 and 24577 records (a tile and one record, whole tiles, three tiles and one): the LONG
    kernel, next to one-tile buckets of 8192 and 1 for the other launch"""
    st = mids_stream(LONG_MIDS + [8192, 1], form)
    assert st.rc.max() <= M.SK_MID_RECORDS and int((st.rc > M.SKR_TILE).sum()) == 4
    run(ctxs, st, pkg.DEBUG_NO_SPEC1, f"long mid buckets, {form}")


@pytest.mark.parametrize("form", ["d2=15", "uniform"])
def test_regroup_longest_not_heavy(ctxs, pkg, form):
    """a mid bucket of exactly SK_MID_RECORDS = 65536 records is still regrouped (eight tiles of the LONG kernel), beside
    one-tile buckets; without a flag the regions overflow and the exact level follows the sweep into the same buffer"""
    st = mids_stream([65536, 4096, 0, 8193, 1], form)
    for flags in (0, pkg.DEBUG_NO_SPEC1):
        assert "sk_heavy_split" not in run(ctxs, st, flags, f"mid bucket of 65536, {form}")


# ------------------------------------------------------------------ f: heavy mid buckets

@pytest.mark.parametrize("form", ["d2=9", "uniform"])
@pytest.mark.parametrize("n", [65536, 65537, 98305])
def test_heavy_by_records(ctxs, pkg, n, form):
    """unforced, R = 2: a mid bucket of 65536 records is regrouped, one of 65537 = 2 x 32768 + 1 or 98305 = 3 x 32768 + 1 is
    split by d2 with the chunked kernels (chunks of 32768: the last holds one record), all of one d2 -- one long final
    bucket -- or uniform; the other mid bucket stays at 60000"""
    d2s = (9,) if form == "d2=9" else D2_ALL
    groups = split_d2(0, 0, n, d2s, (1, 2)) + split_d2(0, 1, 60_000, D2_ALL, (1, 2))
    st = Stream(K, ROWS[2], {"groups": groups, "copies": 32}, "f", n, form)
    assert int(st.rc[0]) == n and M.chunk_len(n) == 32768
    phases = run(ctxs, st, 0, f"mid bucket of {n}, {form}")
    assert ("sk_heavy_split" in phases) == (n > 65536), phases


def forced_stream(extra, k=23):
    """k = 23, 40 000 rows forced: mid_limit = 60 003 k-mers.  Mid bucket 0: 1875 records of 32 k-mers and one of 3 + extra;
    mid bucket 1: 1800 records of 32"""
    g = M.geometry(ROWS[2], k, forced=True)
    assert (g.R, g.mid_limit, M.lmax(k)) == (2, 60_003, 32)
    groups = [(0, 0, d2, 117, 32) for d2 in range(1, 16)] + [(0, 0, 0, 121, np.array([32] * 120 + [3 + extra]))]
    groups += split_d2(0, 1, 1800, D2_ALL, 32)
    return Stream(k, ROWS[2], {"groups": groups}, "f-forced", extra), g


@pytest.mark.parametrize("extra", [0, 1])
def test_heavy_by_kmers_forced(ctxs, pkg, extra):
    """DNAGPU_DEBUG_FORCE_SUPERKMER: a mid bucket whose K-MERS equal mid_limit is not heavy, one more is -- with the k-mers
    counted by the speculative sweep (its packed 64-bit LDS add) and by sk_hist1.  No result shows these counts otherwise."""
    st, g = forced_stream(extra)
    assert int(st.kc[0]) == g.mid_limit + extra and int(st.kc[1]) < g.mid_limit
    for flags in (pkg.DEBUG_FORCE_SUPERKMER, pkg.DEBUG_FORCE_SUPERKMER | pkg.DEBUG_NO_SPEC1):
        phases = run(ctxs, st, flags, f"forced, {g.mid_limit} {extra:+d} k-mers")
        assert ("sk_heavy_split" in phases) == bool(extra), phases
        assert ("sk_spec1" in phases) == (flags == pkg.DEBUG_FORCE_SUPERKMER) and ("sk_hist1" in phases) != ("sk_spec1" in phases), phases


@pytest.mark.parametrize("other", [60_000, 1_000])
def test_heavy_expanded_whole(ctxs, pkg, other):
    """DNAGPU_DEBUG_HEAVY_EXPAND, no NULL records: the heavy mid bucket (65537 records of one k-mer each) goes to the tail's
    expansion as a whole; where it holds most of the k-mers (the other mid bucket at 1000 records) levels 1-2 report the set
    skewed and every coarse bucket is expanded"""
    groups = split_d2(0, 0, 65_537, D2_ALL, 1) + split_d2(0, 1, other, D2_ALL, 3)
    st = Stream(K, ROWS[2], {"groups": groups, "copies": 32}, "f-expand", other)
    assert st.n_null == 0
    phases = run(ctxs, st, pkg.DEBUG_HEAVY_EXPAND, f"heavy expanded, other mid bucket {other}")
    assert ("sk_regroup" in phases) == (other == 60_000) and "sk_heavy_split" not in phases, phases


# ------------------------------------------------------------------ g: the route over two coarse buckets

def test_route_over_two_coarse_buckets(ctxs, pkg):
    """lengths at the edge of sk_even's 1.02 (found with the restated rule; by hand: 20946 | 20947 against 20000): even buckets
    take the speculative sweep, uneven ones the sampled histogram, whose regions do not fit the landing buffer of
    dnagpu_count_records, so the exact level follows ("sk_sample1", "sk_hist1", no "sk_spec1"); an empty bucket beside a full
    one is even"""
    g = M.geometry(ROWS_TWO, K)
    assert (g.c0n, g.R) == (2, 512)
    edge = max(x for x in range(20_000, 23_000) if M.even([x, 20_000]))
    assert edge == 20_946 and not M.even([edge + 1, 20_000])
    for a, b in ((edge, 20_000), (edge + 1, 20_000), (20_000, edge + 1), (0, 20_000), (20_000, 0)):
        groups = (uniform(0, 512, a, SHORT) if a else []) + (uniform(1, 512, b, SHORT) if b else [])
        st = Stream(K, ROWS_TWO, {"groups": groups}, "g", a, b)
        assert st.lens.tolist() == [a, b]
        phases = run(ctxs, st, 0, f"coarse buckets of ({a}, {b})")
        if max(a, b) == edge + 1:
            assert "sk_sample1" in phases and "sk_hist1" in phases and "sk_spec1" not in phases, phases
        else:
            assert "sk_spec1" in phases and "sk_sample1" not in phases and "sk_hist1" not in phases, phases


# ------------------------------------------------------------------ h: other key widths

@pytest.mark.parametrize("k", [20, 32])
def test_other_key_widths(ctxs, pkg, k):
    """the bucket lengths of b, the NULL cases of d and the 8192 | 8193 edge of e at k = 20 and k = 32, every record of
    lmax(k) k-mers (51 and 54 bases: at k = 32 all 108 payload bits travel through both levels)"""
    lm = M.lmax(k)
    assert M.geometry(ROWS[512], k).R == 512 and lm + k - 1 >= 51
    for n in BUCKET_LENS:
        st = Stream(k, ROWS[512], {"groups": uniform(0, 512, n, lm), "copies": 64}, "h-b", n)
        assert "sk_hist1" not in run(ctxs, st, 0, f"k={k}, bucket of {n}")
    for name, (n, pos) in sorted(null_cases(np.random.default_rng(0xD0)).items()):
        st = Stream(k, ROWS[512], {"groups": uniform(0, 512, n - len(pos), lm), "nulls": {0: pos}, "copies": 64}, "h-d", name)
        run(ctxs, st, 0, f"k={k}, NULL records, {name}")
    st = mids_stream([8192, 8193], "uniform", "h", k=k, lengths=lm)
    run(ctxs, st, pkg.DEBUG_NO_SPEC1, f"k={k}, mid buckets of 8192 and 8193")
