"""The super-k-mer record contract, stage by stage: what level 0 emits (dnagpu_sk_records) held against an independent
numpy model of the contract (tests/sk_model.py), and hand-made and re-cut record streams pushed through
dnagpu_count_records at the edges of sk_count_clean's record test.  Every comparison is bit for bit, against numpy or the
CPU oracle.

dnagpu_sk_records always takes the exact pair of level 0 (sk_hist0 + sk_scatter0): the records of the slab sweep (level 0
without its histogram) are not reachable through the C-ABI and stay covered end to end only
(test_gpu_parity.py::test_level0_slabs_and_exact_agree).

Which stage an assertion group pins (check_level0, groups as numbered there):
  1 structure, 2 rows     sk_scatter0's walks and sk_build (payload cut, masks, length field), sk_hist0's prefix (offsets)
  3 offsets               the plain-tile walk and sk_build's position field (SK_POS_*) -- what sk_count_clean's record
                          test (sk_records_share_kmer) is exact on
  4 digits                sk_front's hash and window minima, sk_digits, the walk by value (sk_hash_of for its records)
  5 without the hash      the same, against the records themselves: equal k-mers meet in one final bucket
  6 shards                sk_geometry as a function of global_rows alone; tile cuts do not move a k-mer's bucket
The crafted, limit and metamorphic streams pin sk_count_clean (record table, flank filter, exact test, the in-place count
of sharing records), the selection's stage limits, sk_count and the expansion behind them.
"""
import numpy as np
import pytest

import oracle as orc
import sk_model as M
from __graft_entry__ import load_package
from test_gpu_parity import check_hist_unordered, pack_codes

gpu = pytest.mark.gpu

KS = list(range(20, 33))
SK_WAVE_ROWS = 2016                     # rows of a wave tile (SKW_ROWS)
SK_ROUND_ROWS = 4 * SK_WAVE_ROWS        # one round of a workgroup's four waves (SK_TILE_ROWS)
SKC_MAXREC = 512                        # records of a bucket sk_count_clean / sk_count take
SKQ_KMERS = 4096                        # k-mers of such a bucket (sk_count_cap)
SKQ_DIRTY_MAX = 640                     # k-mers of sharing records that sk_count_clean counts in place
GEOMETRY_ROWS = 50_000_000              # (only fixes the bucket geometry of the crafted streams: several coarse buckets)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ the model alone (CPU)

@pytest.mark.parametrize("k", KS)
def test_model_encode_decode_round_trip(k):
    """records of 1, w and lmax k-mers (the longest: 51 .. 54 bases, across the word boundary at base 32), with and without
    SK_REC_MULTI: decode gives the fields back, and k-mer j is bits [2j, 2j + 2k) of the payload -- cut here with Python
    integers, not with the model's shifts"""
    rng = np.random.default_rng(0x5C0DE + k)
    m, w, lm = M.mlen(k), M.window(k), M.lmax(k)
    assert (m, w) == ((15 if k >= 23 else 13 if k >= 21 else 12), k - m + 1) and lm == min(32, 55 - k)
    cases = []
    for length in sorted({1, 2, w - 1, w, lm - 1, lm}):
        codes = rng.integers(0, 4, length + k - 1, dtype=np.uint8)
        d1, d2 = int(rng.integers(0, 512)), int(rng.integers(0, 16))
        cases.append((codes, d1, d2, None))
        if length <= w:
            for a in sorted({length - 1, k - m}):
                cases.append((codes, d1, d2, a))
    cases.append((np.full(lm + k - 1, 3, dtype=np.uint8), 511, 15, None))            # every payload bit set
    cases.append((np.full(2 * k - m, 3, dtype=np.uint8), 511, 15, k - m))
    recs = M.encode_many([M.encode(c, k, d1=d1, d2=d2, a=a, multi=a is None) for c, d1, d2, a in cases])
    d = M.decode(recs, k)
    assert d.n == len(cases) and not d.null.any() and not M.payload_above(d).any()
    at = 0
    for i, (codes, d1, d2, a) in enumerate(cases):
        nb = len(codes)
        assert (int(d.length[i]), int(d.d1[i]), int(d.d2[i]), bool(d.multi[i])) == (nb - k + 1, d1, d2, a is None)
        if a is not None:
            assert int(d.a[i]) == a
        lo, hi = int(recs[2 * i]), int(recs[2 * i + 1])
        assert hi >> 63 == 0 and (hi >> 44) & 31 == nb - k and (hi >> 58) & 1 == (a is None)
        pay = lo | ((hi & ((1 << (39 if a is not None else 44)) - 1)) << 64)
        assert pay == sum(int(c) << (2 * j) for j, c in enumerate(codes))
        for j in range(nb - k + 1):
            assert int(d.kmers[at + j]) == (pay >> (2 * j)) & ((1 << (2 * k)) - 1)
            assert (int(d.kmer_rec[at + j]), int(d.kmer_j[at + j])) == (i, j)
        at += nb - k + 1
    assert at == len(d.kmers)
    assert any(len(c) > 32 for c, _, _, _ in cases)
    lo, hi = M.encode(cases[0][0], k, multi=True, null=True)
    assert M.decode(np.array([lo, hi], dtype=np.uint64), k).null.all()
    with pytest.raises(ValueError):
        M.encode(np.zeros(lm + k, dtype=np.uint8), k, multi=True)                   # one k-mer too many


@pytest.mark.parametrize("k", KS)
def test_model_minimum_is_a_function_of_the_kmer(k):
    """the leftmost minimum m-mer of a k-mer, found by sliding a window over a sequence, is what the k-mer's bits alone
    give: the same k-mers embedded in two different contexts have the same m-mer value and in-k-mer offset; ties (poly-A:
    every m-mer equal) go to the leftmost"""
    rng = np.random.default_rng(0xC0FFEE + k)
    m = M.mlen(k)
    piece = rng.integers(0, 4, 400, dtype=np.uint8)
    seen = []
    for ctx_seed, at in ((1, 57), (2, 1033)):
        r2 = np.random.default_rng(ctx_seed)
        seq = r2.integers(0, 4, 2000, dtype=np.uint8)
        seq[at:at + len(piece)] = piece
        pos, v = M.sequence_minima(seq, k)
        rows = np.arange(at, at + len(piece) - k + 1)
        seen.append((v[rows], pos[rows] - rows))
        v2, off2 = M.kmer_minimum(M.kmers_of_codes(seq, k), k)
        assert np.array_equal(v, v2) and np.array_equal(pos - np.arange(len(pos)), off2)
        assert np.array_equal(M.mmer_values(seq, m)[pos], v)
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])
    assert len(np.unique(seen[0][1])) > 3                                            # (the offsets do vary)
    v, off = M.kmer_minimum(np.zeros(3, dtype=np.uint64), k)
    assert not off.any() and not v.any()
    # the hash, spelled out once for one value per minimizer length
    val = (0x2ABCDEF5 & ((1 << (2 * m)) - 1))
    want = ((val & 0xFFFFFF) * 0x9E3779 + ((val >> 24) & ((1 << (2 * m - 24)) - 1)) * 0x85EBCB) & 0xFFFFFFFF
    assert int(M.mmer_hash(np.array([val]), m)[0]) == want
    f = (val * 0x9E3779B1) & 0xFFFFFFFF
    assert (int(M.d2_of(np.array([val]))[0]), int(M.d1_of(np.array([val]), 9)[0])) == ((f >> 19) & 15, (f >> 23) & 511)


def test_model_mean_run_length():
    """runs of one (hash, position) minimum on random sequence at k = 31: 9.01 k-mers on 2 Mbase with these constants
    (sk_device.hpp: 8.997 with tile cuts); the window only guards the model's constants against typos"""
    codes = np.random.default_rng(0x2E31).integers(0, 4, 400_000, dtype=np.uint8)
    assert 8.5 < M.mean_run_length(codes, 31) < 9.5


# ------------------------------------------------------------------ level 0 against the model

def level0_records(ctx, words, n_bases, k, first, count, global_rows):
    """dnagpu_sk_records -> (the records' 2n words, the bucket offsets)"""
    d = ctx.upload(words, n_bases)
    try:
        r = ctx.sk_records(d, k, first, count, global_rows)
        try:
            off = r.offsets.astype(np.int64)
            recs = ctx.download_u64(r.device_ptr, 2 * r.n_records).copy() if r.n_records else np.zeros(0, dtype=np.uint64)
        finally:
            r.free()
    finally:
        d.free()
    return recs, off


class Level0:
    """what check_level0 found out about one call's records"""


def check_level0(recs, off, k, c0, want_rows, what):
    """The record contract on the records of one dnagpu_sk_records call; all failures of the case in one message.
    -> Level0: dec (sk_model.decode), bucket per record, v / in-k-mer offset per k-mer under the model, b1, the number of
    pairs of records without SK_REC_MULTI that share a k-mer."""
    fails = []

    def bad(mask, text):
        mask = np.asarray(mask)
        if mask.any():
            fails.append(f"{text}: {int(mask.sum())} of {mask.size}, first at {int(np.flatnonzero(mask)[0])}")

    m, lm = M.mlen(k), M.lmax(k)
    dec = M.decode(recs, k)
    res = Level0()
    res.dec = dec
    # ---- 1 structure
    if len(off) != c0 + 1 or off[0] != 0 or np.any(np.diff(off) < 0):
        fails.append(f"1 offsets not ascending from 0 over {c0} buckets: {off.tolist()}")
    if off[-1] != dec.n:
        fails.append(f"1 last offset {int(off[-1])}, {dec.n} records")
    assert not fails, f"{what}: " + "; ".join(fails)                                 # (nothing below makes sense without buckets)
    bucket = np.repeat(np.arange(c0, dtype=np.int64), np.diff(off))
    res.bucket = bucket
    bad(dec.null, "1 NULL records")
    bad(dec.length > lm, f"1 records longer than lmax = {lm}")
    bad(M.payload_above(dec) != 0, "1 payload bits set at or above 2 (len + k - 1)")
    # ---- 2 rows
    got, want = np.sort(dec.kmers), np.sort(np.asarray(want_rows, dtype=np.uint64))
    if got.shape != want.shape:
        fails.append(f"2 {got.size} k-mers in the records, {want.size} rows")
    else:
        bad(got != want, "2 sorted k-mers differ from the sorted rows")
    # ---- the model, per k-mer
    v, o = M.kmer_minimum(dec.kmers, k)
    rec, j = dec.kmer_rec, dec.kmer_j
    plain = ~dec.multi
    pk = plain[rec]
    res.v, res.off, res.plain_kmer = v, o, pk
    # ---- 3 records without SK_REC_MULTI
    bad(plain & ((dec.a < dec.length - 1) | (dec.a > k - m)), "3 offset outside len - 1 .. k - m")
    bad(pk & (o != dec.a[rec] - j), "3 k-mers whose leftmost minimum m-mer is not at a - j")
    # ---- 4 every record
    v_first = v[dec.first[:-1]] if dec.n else v[:0]
    bad(v != v_first[rec], "4 k-mers whose minimum m-mer value differs from their record's first k-mer's")
    bad(M.d0_of(v_first, m, c0) != bucket, "4 records outside bucket d0(v)")
    bad(M.d2_of(v_first) != dec.d2, "4 records with d2 != d2(v)")
    b1 = M.infer_b1(dec.d1)
    res.b1 = b1
    if b1 > 9:
        fails.append(f"4 d1 takes {b1} bits")
    bad(M.d1_of(v_first, b1) != dec.d1, f"4 records with d1 != (f >> 23) masked to {b1} bits")
    # ---- 5 independent of the model's hash
    triple = (bucket << 13) | (dec.d1.astype(np.int64) << 4) | dec.d2.astype(np.int64)
    res.triple_kmer = triple[rec]
    order = np.argsort(dec.kmers, kind="stable")
    ks, ts = dec.kmers[order], res.triple_kmer[order]
    bad((ks[1:] == ks[:-1]) & (ts[1:] != ts[:-1]), "5 equal k-mers in different (bucket, d1, d2)")
    stated = M.mmer_at(dec, dec.a)                                                   # (meaningful for plain records only)
    po = order[pk[order]]                                                            # the plain records' k-mers, sorted
    same = dec.kmers[po][1:] == dec.kmers[po][:-1]
    ra, rb = rec[po][:-1], rec[po][1:]
    bad(same & (stated[ra] != stated[rb]), "5 equal k-mers of two plain records with different m-mers at the stated offsets")
    bad(same & ((dec.a[ra] - j[po][:-1]) != (dec.a[rb] - j[po][1:])), "5 equal k-mers of two plain records with different a - j")
    sh = same & (ra != rb)
    res.sharing_pairs = len(np.unique(np.stack([np.minimum(ra[sh], rb[sh]), np.maximum(ra[sh], rb[sh])]), axis=1).T) if sh.any() else 0
    assert not fails, f"{what}: " + "; ".join(fails)
    return res


def run_level0(ctx, words, n_bases, k, first, count, global_rows, what, rows=None):
    if rows is None:
        rows = orc.generate_kmers(words, n_bases, k, faithful=False)
    recs, off = level0_records(ctx, words, n_bases, k, first, count, global_rows)
    res = check_level0(recs, off, k, ctx.sk_buckets(global_rows, k), rows[first:first + count], what)
    res.recs, res.offsets = recs, off
    return res


def random_codes(n, seed):
    return np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)


def copies_codes(n, seed, pieces=60):
    """random sequence with 150-base pieces copied to random places"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 4, n, dtype=np.uint8)
    for _ in range(pieces):
        a, b = rng.integers(0, n - 150, 2)
        c[b:b + 150] = c[a:a + 150].copy()
    return c


def island_codes(n, seed):
    """a 3000-base low-complexity island (poly-A, (AC)n, a 5-base unit) inside random sequence: plain tiles, tiles of too
    many runs and the partial tile side by side"""
    c = random_codes(n, seed)
    at = 2 * SK_WAVE_ROWS + 700
    c[at:at + 1000] = 0
    c[at + 1000:at + 2000] = np.tile(np.array([0, 2], dtype=np.uint8), 500)
    c[at + 2000:at + 3000] = np.tile(np.array([3, 0, 1, 1, 2], dtype=np.uint8), 200)
    return c


_INPUTS = {}


def named_input(name):
    """-> (words, n_bases) of the low-complexity / repeat / random inputs, ~40 000 bases each; made once"""
    if name not in _INPUTS:
        n = 40_000
        if name == "polyA":
            w = pack_codes(np.zeros(n, dtype=np.uint8))
        elif name == "polyG":
            w = pack_codes(np.full(n, 3, dtype=np.uint8))
        elif name == "AC":
            w = pack_codes(np.tile(np.array([0, 2], dtype=np.uint8), n // 2))
        elif name == "motif7":
            w = orc.synth_words_repeat(0x5EED7, n, 7)
        elif name == "motif64":
            w = orc.synth_words_repeat(0x5EED64, n, 64)
        elif name == "copies":
            w = pack_codes(copies_codes(n, 0xC0B1E5))
        elif name == "island":
            w = pack_codes(island_codes(n, 0x151A))
        else:
            assert name == "random"
            w = pack_codes(random_codes(n, 0x4A2D))
        _INPUTS[name] = (w, n)
    return _INPUTS[name]


@gpu
@pytest.mark.parametrize("k", KS)
def test_level0_every_k(ctx, k):
    """every k from 20 to 32 (each its own SkFront<W> or minimizer length) on one random input of 30 000 bases, in its own
    geometry (one coarse bucket, a narrow d1) and in those of far larger global row counts: dozens of coarse buckets and
    d1 at its full width, so that the digits say something about the hash"""
    n = 30_000
    words = pack_codes(random_codes(n, 0x30000))
    all_rows = orc.generate_kmers(words, n, k, faithful=False)
    rows = n - k + 1
    seen = {}
    for global_rows in (rows, GEOMETRY_ROWS, 4_000_000_000):
        res = run_level0(ctx, words, n, k, 0, rows, global_rows, f"level 0, random, k={k}, geometry of {global_rows} rows", all_rows)
        assert not res.dec.multi.all() and res.dec.multi.any()                       # (full tiles plain, the partial tile by value)
        seen[global_rows] = (len(np.unique(res.bucket)), res.b1)
    assert seen[4_000_000_000][0] >= 64 and seen[4_000_000_000][1] == 9 and seen[GEOMETRY_ROWS][1] == 9, seen


ROW_COUNTS = [1, 63, 64, SK_WAVE_ROWS - 1, SK_WAVE_ROWS, SK_WAVE_ROWS + 1, SK_ROUND_ROWS - 1, SK_ROUND_ROWS, SK_ROUND_ROWS + 1,
              10 * SK_WAVE_ROWS + 1000]


@gpu
@pytest.mark.parametrize("k", [20, 21, 23, 31, 32])
def test_level0_row_counts(ctx, k):
    """row counts around the wave tile (2016 rows), the workgroup round (8064) and a partial tile, the sequence going on
    behind the window's last row.  On 10 * 2016 + 1000 rows at least 80 % of the k-mers lie in records without
    SK_REC_MULTI: full tiles of random sequence are plain, only the partial tile goes through the walk by value."""
    n = ROW_COUNTS[-1] + 100
    words = pack_codes(random_codes(n, 0x20C0 + k))
    rows = orc.generate_kmers(words, n, k, faithful=False)
    for count in ROW_COUNTS:
        res = run_level0(ctx, words, n, k, 0, count, count, f"level 0, k={k}, {count} rows", rows)
        if count == ROW_COUNTS[-1]:
            assert res.plain_kmer.mean() >= 0.8, f"{res.plain_kmer.mean():.3f} of the k-mers in plain records"
        if count % SK_WAVE_ROWS == 0:
            assert not res.dec.multi.any(), f"k={k}, {count} rows: full tiles of random sequence are plain"


@gpu
@pytest.mark.parametrize("k", [20, 21, 23, 31, 32])
def test_level0_windows(ctx, k):
    """windows that start off the word and tile boundaries, in the geometry of a larger global row count"""
    n = 30_000
    words = pack_codes(random_codes(n, 0x30000))
    rows = orc.generate_kmers(words, n, k, faithful=False)
    count = SK_ROUND_ROWS + 777
    widths = set()
    for first in (0, 1, 31, 33, SK_WAVE_ROWS - 7):
        res = run_level0(ctx, words, n, k, first, count, GEOMETRY_ROWS, f"level 0, k={k}, window at {first}", rows)
        widths.add(res.b1)
    assert ctx.sk_buckets(GEOMETRY_ROWS, k) >= 2 and max(widths) == 9                 # (several coarse buckets, d1 at its widest)


@gpu
@pytest.mark.parametrize("name", ["polyA", "polyG", "AC", "motif7", "motif64", "copies", "island"])
@pytest.mark.parametrize("k", [20, 22, 27, 32])
def test_level0_low_complexity_and_repeats(ctx, name, k):
    """low-complexity and repeat inputs: one m-mer value over whole tiles (sk_uniform_value), tiles of too many (hash,
    position) runs (the walk by value), copies of plain stretches (records that share k-mers)"""
    words, n = named_input(name)
    rows = n - k + 1
    res = run_level0(ctx, words, n, k, 0, rows, rows, f"level 0, {name}, k={k}")
    dec = res.dec
    if name in ("polyA", "motif7"):
        assert (dec.multi & (dec.length == M.lmax(k))).any(), "no SK_REC_MULTI record of lmax k-mers"
    if name == "copies":
        assert res.sharing_pairs >= 100, f"{res.sharing_pairs} pairs of plain records share a k-mer"
    if name == "island":
        assert dec.multi.any() and not dec.multi.all()


@gpu
@pytest.mark.parametrize("k", [21, 31])
def test_level0_shards(ctx, pkg, k):
    """the rows of one input cut as 3 shards with their halos (as test_records_exchange_one_process cuts them): every
    shard's records keep the contract, and every k-mer's (bucket, d1, d2) is the one the whole cut gives it"""
    import importlib
    sh = importlib.import_module(pkg.__name__ + ".shard_math")
    n = 300_000
    words = pack_codes(random_codes(n, 0x54A2D + k))
    all_rows = orc.generate_kmers(words, n, k, faithful=False)
    rows = n - k + 1
    whole = run_level0(ctx, words, n, k, 0, rows, rows, f"level 0, whole, k={k}", all_rows)
    order = np.argsort(whole.dec.kmers, kind="stable")
    wk, wt = whole.dec.kmers[order], whole.triple_kmer[order]
    seen = 0
    for first, cnt, lo, hi in sh.shard_ranges(n, k, 3):
        w = np.ascontiguousarray(words[lo // 32:(hi + 31) // 32])
        assert lo % 32 == 0 and cnt > 0
        recs, off = level0_records(ctx, w, hi - lo, k, 0, cnt, rows)
        part = check_level0(recs, off, k, ctx.sk_buckets(rows, k), all_rows[first:first + cnt], f"level 0, shard at {first}, k={k}")
        at = np.searchsorted(wk, part.dec.kmers)
        assert np.array_equal(wk[at], part.dec.kmers)
        moved = wt[at] != part.triple_kmer
        assert not moved.any(), f"shard at {first}: {int(moved.sum())} k-mers in another (bucket, d1, d2) than in the whole cut"
        assert part.b1 == whole.b1
        seen += cnt
    assert seen == rows


# ------------------------------------------------------------------ dnagpu_count_records on crafted streams

def count_stream(ctx, recs, pieces_of, k, rows, truth_kmers, what, profile=False, unique=None):
    """uploads the records (2n words), counts pieces_of(device pointer) -> [(pointer, n, bucket)], compares the histogram
    with np.unique of truth_kmers (unique: that result, np.unique(truth_kmers, return_counts=True), where the caller counts
    one stream several times and has it already).  -> the phase names if profile"""
    buf = ctx.buffer_alloc(max(recs.nbytes, 16))
    try:
        ctx.upload_u64(buf, recs)
        if profile:
            ctx.set_profiling(True)
        try:
            h = ctx.count_records(pieces_of(buf), k, rows)
            phases = [a for a, _ in ctx.last_phase_times()] if profile else None
        finally:
            if profile:
                ctx.set_profiling(False)
        try:
            ok, oc = unique if unique is not None else np.unique(np.asarray(truth_kmers, dtype=np.uint64), return_counts=True)
            assert h.total == len(truth_kmers), f"{what}: total {h.total}, {len(truth_kmers)} k-mers"
            check_hist_unordered(h, ok, oc.astype(np.uint64), what)
        finally:
            h.free()
    finally:
        ctx.buffer_free(buf)
    return phases


def window_record(S, k, start, length, d1, d2):
    """the record of `length` k-mers from base `start` of S, whose declared m-mer lies at base k - m of S"""
    return M.encode(S[start:start + length + k - 1], k, d1=d1, d2=d2, a=(k - M.mlen(k)) - start)


def family_windows(k, rng):
    """(start, length) of the sub-windows of a string of 2k - m bases whose k-mers all cover the m-mer at base k - m:
    the whole string, single k-mers at both ends (a = k - m and a = 0), lengths in between"""
    m, w = M.mlen(k), M.window(k)
    wins = [(0, w), (0, 1), (k - m, 1), (0, w // 2), (w - w // 2, w // 2), (1, w - 2), (k - m - 1, 2), (k - m - 2, 2)]
    for _ in range(4):
        length = int(rng.integers(1, w + 1))
        wins.append((int(rng.integers(0, w - length + 1)), length))
    assert all(s >= 0 and length >= 1 and s + length - 1 <= k - m for s, length in wins)
    return wins


def variants_of(S, k):
    """S itself and every S' that differs from it in exactly one base, L = 1 .. k - m bases left of the m-mer or R = 1 ..
    k - m right of it: around the m-mer S and S' agree over k - m - 1 up to k - m + 1 ... 2 (k - m) bases"""
    m = M.mlen(k)
    out = [("S", S)]
    for L in range(1, k - m + 1):
        V = S.copy()
        V[k - m - L] ^= 1
        out.append((f"L{L}", V))
    for R in range(1, k - m + 1):
        V = S.copy()
        V[k - 1 + R] ^= 2
        out.append((f"R{R}", V))
    return out


def cut_classes(k, start, length):
    """which of sk_count_clean's cuts a window takes (names as in the issue's list)"""
    m = M.mlen(k)
    a, nb = (k - m) - start, length + k - 1
    flank = min(8, (k - m) // 2)
    got = set()
    if 2 * (a + m) >= 64:
        got.add("sr>=64")
    elif 2 * (a + m) >= 32:
        got.add("sr 32..63")
    if a < flank:
        got.add("a<flank")
    if nb - a - m < flank:
        got.add("right<flank")
    if nb > 32:
        got.add("payload crosses base 32")
    if a < 16 < a + m:
        got.add("m-mer crosses a dword")
    return got


@gpu
@pytest.mark.parametrize("k", KS)
def test_count_records_crafted_families(ctx, k):
    """Hand-made records without SK_REC_MULTI around one declared m-mer: sub-windows of a random string S of 2k - m bases
    (the m-mer at base k - m, so a = k - m - start) and of every one-base variant of it, the truth whatever np.unique says
    about the cut k-mers.  Twice: all of it in ONE final bucket (nearly every record shares k-mers with others: up to
    k = 27 their k-mers stay within SKQ_DIRTY_MAX and sk_count_clean counts them in place, beyond that the bucket is
    sk_count's), and as PAIRS of records, every pair around a string of its own in a final bucket of its own -- there a
    pair that sk_records_share_kmer wrongly calls disjoint leaves the bucket as (key, 1) groups with a duplicate,
    whatever k.

    The cuts sk_count_clean takes differently must occur in the case list (asserted): 2 (a + m) >= 64 (k = 32, a = 17
    only), 2 (a + m) in 32 .. 63, a < flank, fewer than flank bases right of the m-mer, a payload across base 32.  An
    m-mer that itself crosses base 32 cannot occur in a record without SK_REC_MULTI (a + m <= k <= 32; at k = 32 and
    a = 17 it ends exactly there, the first case); what does occur, and is asserted, is an m-mer across the payload's
    first dword boundary (a < 16 < a + m), where the kernel switches the dwords it cuts from."""
    rng = np.random.default_rng(0xFA3117 + k)
    m = M.mlen(k)
    nb_geo = ctx.sk_buckets(GEOMETRY_ROWS, k)
    wins = family_windows(k, rng)
    classes = set().union(*(cut_classes(k, s, length) for s, length in wins))
    want = {"sr 32..63", "a<flank", "right<flank", "m-mer crosses a dword"}
    if 2 * k - m > 32:                               # (k >= 24: below that no record without SK_REC_MULTI has 33 bases)
        want.add("payload crosses base 32")
    if k == 32:
        want.add("sr>=64")
    assert want <= classes, f"k={k}: the case list lacks {sorted(want - classes)}"
    assert {(k - m) - s for s, _ in wins} >= {0, k - m}
    # ---- one final bucket
    S = rng.integers(0, 4, 2 * k - m, dtype=np.uint8)
    recs, kmers = [], []
    for vi, (_, V) in enumerate(variants_of(S, k)):
        for s, length in (wins if vi == 0 else wins[:3] + [wins[4 + vi % (len(wins) - 4)]]):
            recs.append(window_record(V, k, s, length, 7, 5))
            kmers.append(M.kmers_of_codes(V[s:s + length + k - 1], k))
    kmers = np.concatenate(kmers)
    assert len(recs) <= SKC_MAXREC and len(kmers) <= SKQ_KMERS and len(np.unique(kmers)) < len(kmers)
    words = M.encode_many(recs)
    dec = M.decode(words, k)
    assert np.array_equal(dec.kmers, kmers) and not M.payload_above(dec).any()        # (the stream keeps the contract)
    count_stream(ctx, words, lambda p: [(p, len(recs), nb_geo - 1)], k, GEOMETRY_ROWS, kmers, f"crafted family, one bucket, k={k}")
    # ---- pairs, a final bucket each
    recs, kmers, per_bucket = [], [], []
    bucket_id = 0
    for vi, (name, _) in enumerate(variants_of(S, k)):
        for wa in range(len(wins)):
            for wb in ((wa, 0, 2) if vi else (wa, 0)):
                Sb = rng.integers(0, 4, 2 * k - m, dtype=np.uint8)
                Vb = dict(variants_of(Sb, k))[name]
                d2, b, d1 = bucket_id % 16, (bucket_id // 16) % nb_geo, (bucket_id // (16 * nb_geo)) * 19 % 512
                bucket_id += 1
                (sa, la), (sb, lb) = wins[wa], wins[wb]
                recs += [window_record(Sb, k, sa, la, d1, d2), window_record(Vb, k, sb, lb, d1, d2)]
                kmers += [M.kmers_of_codes(Sb[sa:sa + la + k - 1], k), M.kmers_of_codes(Vb[sb:sb + lb + k - 1], k)]
                per_bucket.append(b)
    kmers = np.concatenate(kmers)
    uniq, cnt = np.unique(kmers, return_counts=True)
    assert (cnt > 1).any() and (cnt == 1).any()
    words = M.encode_many(recs).reshape(-1, 2)
    by_bucket = np.argsort(np.repeat(per_bucket, 2), kind="stable")                   # records grouped by coarse bucket
    words = np.ascontiguousarray(words[by_bucket]).reshape(-1)
    n_in = np.bincount(np.repeat(per_bucket, 2), minlength=nb_geo)
    starts = np.concatenate([[0], np.cumsum(n_in)])
    count_stream(ctx, words, lambda p: [(p + 16 * int(starts[b]), int(n_in[b]), b) for b in range(nb_geo) if n_in[b]],
                 k, GEOMETRY_ROWS, kmers, f"crafted pairs, {bucket_id} final buckets, k={k}")


def distinct_strings(rng, n, length):
    """n random base strings, told apart by their first 12 bases"""
    S = rng.integers(0, 4, (n, length), dtype=np.uint8)
    tag = np.arange(n)
    for i in range(12):
        S[:, i] = (tag >> (2 * i)) & 3
    return S


def limit_stream(k, rng, lengths, n_copied):
    """one record per entry of lengths, each a window (from base 0) of a string of its own; the last n_copied records are
    copies of the n_copied before them (so exactly those 2 n_copied records share k-mers) -> (words, k-mers)"""
    n = len(lengths)
    S = distinct_strings(rng, n - n_copied, 2 * k - M.mlen(k))
    recs, kmers = [], []
    for i, length in enumerate(lengths):
        src = i if i < n - n_copied else i - n_copied
        length = min(length, M.window(k))
        recs.append(window_record(S[src], k, 0, length, 3, 9))
        kmers.append(M.kmers_of_codes(S[src][:length + k - 1], k))
    return M.encode_many(recs), np.concatenate(kmers)


@gpu
@pytest.mark.parametrize("limit", ["records", "k-mers", "dirty"])
@pytest.mark.parametrize("k", [31, 21])
def test_count_records_stage_limits(ctx, k, limit):
    """one final bucket at the limits of sk_count_clean's stage: SKC_MAXREC records and one more, SKQ_KMERS k-mers and one
    more, SKQ_DIRTY_MAX k-mers of sharing records and one more.  One record or k-mer past the stage the selection sends the
    bucket through the expansion: "sk_expand_flat" is among the phases then and only then.  The dirty limit decides between
    sk_count_clean's in-place count and sk_count, which share the phase "sk_count": there the result alone is asserted."""
    rng = np.random.default_rng(0x11417 + k)
    last = ctx.sk_buckets(GEOMETRY_ROWS, k) - 1
    assert M.window(k) >= 9                                                          # (records of 9 k-mers below)
    if limit == "records":
        for n_rec in (SKC_MAXREC, SKC_MAXREC + 1):
            words, kmers = limit_stream(k, rng, [1 + i % 3 for i in range(n_rec)], 20)
            assert len(words) == 2 * n_rec and len(kmers) <= SKQ_KMERS
            phases = count_stream(ctx, words, lambda p: [(p, n_rec, last)], k, GEOMETRY_ROWS, kmers, f"{n_rec} records, k={k}", profile=True)
            assert ("sk_expand_flat" in phases) == (n_rec > SKC_MAXREC), (n_rec, phases)
            assert "sk_count_big" not in phases, phases
    elif limit == "k-mers":
        for n_km in (SKQ_KMERS, SKQ_KMERS + 1):
            lengths = [8] * SKC_MAXREC                                               # 512 x 8 = 4096 k-mers, two quads per record
            lengths[0] += n_km - SKQ_KMERS
            words, kmers = limit_stream(k, rng, lengths, 20)
            assert len(words) == 2 * SKC_MAXREC and len(kmers) == n_km
            phases = count_stream(ctx, words, lambda p: [(p, SKC_MAXREC, last)], k, GEOMETRY_ROWS, kmers, f"{n_km} k-mers, k={k}", profile=True)
            assert ("sk_expand_flat" in phases) == (n_km > SKQ_KMERS), (n_km, phases)
            assert "sk_count_big" not in phases, phases
    else:
        for n_dirty in (SKQ_DIRTY_MAX, SKQ_DIRTY_MAX + 1):
            lengths = [1 + i % 5 for i in range(200)] + [8] * 80                     # the 40 + 40 sharing records last: 640 k-mers
            lengths[-1] += n_dirty - SKQ_DIRTY_MAX
            words, kmers = limit_stream(k, rng, lengths, 40)
            uniq, cnt = np.unique(kmers, return_counts=True)
            assert sum(lengths[-80:]) == n_dirty and int((cnt == 2).sum()) == SKQ_DIRTY_MAX // 2 and cnt.max() == 2
            phases = count_stream(ctx, words, lambda p: [(p, len(lengths), last)], k, GEOMETRY_ROWS, kmers,
                                  f"{n_dirty} k-mers of sharing records, k={k}", profile=True)
            assert "sk_expand_flat" not in phases and "sk_count" in phases, phases


# ------------------------------------------------------------------ metamorphic: the real records, rearranged

def set_multi(words, which):
    """bit 58 set on the chosen records (their offset field, payload from then on, cleared)"""
    out = words.reshape(-1, 2).copy()
    hi = out[:, 1]
    plain = ((hi >> np.uint64(M.REC_MULTI_BIT)) & np.uint64(1)) == 0
    sel = which & plain
    hi[sel] = (hi[sel] & ~np.uint64(M.POS_MASK << M.POS_SHIFT)) | np.uint64(1 << M.REC_MULTI_BIT)
    return out.reshape(-1)


def recut(words, off, k, rng):
    """every record without bit 58, of len >= 2, cut in two at a random j: the first part keeps a and is truncated to
    j + k - 1 bases, the second starts j bases later with a - j; both keep the digits.  -> (words, offsets)"""
    dec = M.decode(words, k)
    cut = (~dec.multi) & (dec.length >= 2)
    j = np.where(cut, rng.integers(1, np.maximum(dec.length, 2)), 0).astype(np.int64)
    keep_bits = np.uint64(~((0x1F << M.LEN_SHIFT) | (M.POS_MASK << M.POS_SHIFT) | ((1 << M.POS_SHIFT) - 1)) & 0xFFFFFFFFFFFFFFFF)

    def part(lo, ph, nbases, length, a, hi):
        nb2 = 2 * nbases
        lo_m = np.where(nb2 >= 64, ~np.uint64(0), (np.uint64(1) << np.minimum(nb2, 63).astype(np.uint64)) - np.uint64(1))
        hi_m = (np.uint64(1) << np.clip(nb2 - 64, 0, 63).astype(np.uint64)) - np.uint64(1)
        return lo & lo_m, (hi & keep_bits) | (ph & hi_m) | ((length - 1).astype(np.uint64) << np.uint64(M.LEN_SHIFT)) | \
            (a.astype(np.uint64) << np.uint64(M.POS_SHIFT))

    s = (2 * j).astype(np.uint64)
    lo2 = np.where(s > 0, (dec.lo >> s) | (dec.pay_hi << ((np.uint64(64) - s) & np.uint64(63))), dec.lo)
    ph2 = dec.pay_hi >> s
    first = part(dec.lo, dec.pay_hi, j + k - 1, j, dec.a, dec.hi)
    second = part(lo2, ph2, dec.length - j + k - 1, dec.length - j, dec.a - j, dec.hi)
    n_out = 1 + cut.astype(np.int64)
    at = np.concatenate([[0], np.cumsum(n_out)])
    out = np.empty((int(at[-1]), 2), dtype=np.uint64)
    whole = ~cut
    out[at[:-1][whole], 0], out[at[:-1][whole], 1] = dec.lo[whole], dec.hi[whole]
    out[at[:-1][cut], 0], out[at[:-1][cut], 1] = first[0][cut], first[1][cut]
    out[at[:-1][cut] + 1, 0], out[at[:-1][cut] + 1, 1] = second[0][cut], second[1][cut]
    return out.reshape(-1), at[off]


@gpu
@pytest.mark.parametrize("name", ["random", "copies", "motif64"])
@pytest.mark.parametrize("k", [21, 27, 32])
def test_count_records_metamorphic(ctx, name, k):
    """the records level 0 cuts, rearranged in ways the contract allows, still count to the oracle's histogram: the records
    of every bucket shuffled; every bucket in many pieces (of one record, of none) in scrambled order; SK_REC_MULTI set on
    every record and on a random half; every plain record of two or more k-mers cut in two at a random place.
    The rows are whole wave tiles: a partial tile's records are SK_REC_MULTI, and spread over the few final buckets of so
    short an input they would send every bucket past sk_count_clean's record test (asserted: no such record as cut, on
    the inputs made of random sequence).  Twice: in the rows' own geometry (final buckets of ~1200 k-mers, sharing records
    by the dozen in each) and in that of a far larger global row count (thousands of final buckets of a few records)."""
    words, n = named_input(name)
    rows = (n - k + 1) // SK_WAVE_ROWS * SK_WAVE_ROWS
    kmers = orc.generate_kmers(words, n, k, faithful=False)[:rows]
    rng = np.random.default_rng(0x3E7A + k)
    for global_rows in (rows, GEOMETRY_ROWS):
        recs, off = level0_records(ctx, words, n, k, 0, rows, global_rows)
        nb = len(off) - 1
        n_rec = len(recs) // 2
        bucket = np.repeat(np.arange(nb), np.diff(off))
        whole = lambda o: (lambda p: [(p + 16 * int(o[b]), int(o[b + 1] - o[b]), b) for b in range(nb)])
        what = f"{name}, k={k}, geometry of {global_rows} rows"
        as_cut = M.decode(recs, k)
        if name != "motif64":
            assert not as_cut.multi.any(), what
        else:
            assert not as_cut.multi.all(), what
        count_stream(ctx, recs, whole(off), k, global_rows, kmers, what + ": as cut")
        # shuffled inside every bucket
        perm = np.lexsort((rng.random(n_rec), bucket))
        shuffled = np.ascontiguousarray(recs.reshape(-1, 2)[perm]).reshape(-1)
        count_stream(ctx, shuffled, whole(off), k, global_rows, kmers, what + ": shuffled")

        def pieces(p):
            out = []
            for b in range(nb):
                lo, hi = int(off[b]), int(off[b + 1])
                cuts = np.unique(np.concatenate([[lo, hi], rng.integers(lo, hi + 1, 12), [min(lo + 1, hi), max(hi - 1, lo)]]))
                for a, z in zip(cuts[:-1], cuts[1:]):
                    out.append((p + 16 * int(a), int(z - a), b))
                out += [(p + 16 * lo, 0, b), (0, 0, b)]                              # pieces of no record
            return [out[i] for i in rng.permutation(len(out))]

        count_stream(ctx, shuffled, pieces, k, global_rows, kmers, what + ": in pieces")
        count_stream(ctx, set_multi(recs, np.ones(n_rec, dtype=bool)), whole(off), k, global_rows, kmers, what + ": all SK_REC_MULTI")
        count_stream(ctx, set_multi(shuffled, rng.random(n_rec) < 0.5), whole(off), k, global_rows, kmers, what + ": half SK_REC_MULTI")
        cut_words, cut_off = recut(recs, off, k, rng)
        dec = M.decode(cut_words, k)
        assert len(cut_words) > len(recs) and np.array_equal(np.sort(dec.kmers), np.sort(kmers)) and not M.payload_above(dec).any()
        count_stream(ctx, cut_words, whole(cut_off), k, global_rows, kmers, what + ": re-cut")
