"""Count-ordered queries over counted groups (dnagpu_hist_* / dnagpu_acc_* spectrum, select, top): the reference's
ORDER BY count(*) DESC (test.sql:95) and its summary of the counts (test.sql:112-114) answered on the device, over histograms
of every shape and over the accumulator's 64-bit counts.  The expected answers are numpy over the oracle's groups:
np.bincount of the counts, a boolean mask, np.lexsort((keys, -counts)).  CPU test: the argument rules that need no device."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import ROOT, load_package

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
U64_MAX = 2 ** 64 - 1
BAD_ARG, TOO_LARGE = 5, 6
SENTINEL = np.uint64(0xC3C3C3C3C3C3C3C3)
GAP = 512                                         # sentinel words behind every device output


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


# ------------------------------------------------------------------ CPU: what needs no device

def test_query_argument_rules_without_a_device(pkg, g):
    L = pkg.lib()
    n = C.c_uint64(77)
    bins = (C.c_uint64 * 4)()
    for obj in ("hist", "acc"):
        spectrum, select, top = (getattr(L, f"dnagpu_{obj}_{q}") for q in ("spectrum", "select", "top"))
        assert spectrum(None, None, 4, bins) == BAD_ARG
        assert spectrum(None, None, 0, bins) == BAD_ARG
        assert spectrum(None, None, pkg.SPECTRUM_MAX_BINS + 1, bins) == BAD_ARG
        assert spectrum(None, None, 4, None) == BAD_ARG
        assert select(None, None, 1, U64_MAX, None, None, 0, C.byref(n), 0) == BAD_ARG
        assert select(None, None, 1, U64_MAX, None, None, 0, None, 0) == BAD_ARG
        assert top(None, None, 10, None, None, C.byref(n), 0) == BAD_ARG
        assert top(None, None, 10, None, None, None, 0) == BAD_ARG
        assert top(None, None, pkg.TOP_MAX + 1, None, None, C.byref(n), 0) == TOO_LARGE
        assert top(None, None, pkg.TOP_MAX, None, None, C.byref(n), 0) == BAD_ARG        # (in range: the missing object)
    assert pkg.SPECTRUM_MAX_BINS == 1 << 20 and pkg.TOP_MAX == 1 << 20
    assert pkg.abi_version() == 2
    # the glue's ORDER BY count(*) DESC LIMIT n refuses a bad limit before it touches a device
    for limit in (0, -3, pkg.TOP_MAX + 1):
        with pytest.raises(g.GlueError) as ei:
            g.count_kmers_top("ATCGATCGATCGATCGACG", 5, limit)
        assert str(ei.value) == "count_kmers_top: limit must be between 1 and 1048576"
        with pytest.raises(g.GlueError) as ei:
            g.count_kmers_agg_top(["ATCGATCG"], 5, limit)
        assert str(ei.value) == "count_kmers_agg_top: limit must be between 1 and 1048576"


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def add_up(parts):
    """[(keys, counts, multiplicity)] -> the groups summed, keys ascending (64-bit counts)"""
    keys = np.concatenate([k for k, _, _ in parts])
    counts = np.concatenate([c.astype(np.uint64) * np.uint64(m) for _, c, m in parts])
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    if not len(keys):
        return keys, counts
    head = np.concatenate([[True], keys[1:] != keys[:-1]])
    at = np.flatnonzero(head)
    return keys[at], np.add.reduceat(counts, at).astype(np.uint64)


def want_spectrum(oc, n_bins):
    """bins[c - 1] = groups with count c, the last bin = groups with count >= n_bins"""
    clamped = np.minimum(oc, np.uint64(n_bins)).astype(np.int64)
    return np.bincount(clamped, minlength=n_bins + 1)[1:].astype(np.uint64)


def are_groups(gk, gc, ok, oc):
    """every (gk[i], gc[i]) is a group of the oracle (ok ascending)"""
    if not len(gk):
        return True
    at = np.minimum(np.searchsorted(ok, gk), len(ok) - 1)
    return bool(np.all(ok[at] == gk) and np.all(oc[at] == gc))


def check_top(got_keys, got_counts, ok, oc, n, what=""):
    rows = min(n, len(ok))
    assert len(got_keys) == rows and len(got_counts) == rows, f"{what}: {len(got_keys)} rows, want {rows}"
    if rows == 0:
        return
    gc = got_counts.astype(np.uint64)
    assert np.all(gc[1:] <= gc[:-1]), f"{what}: counts not descending"
    same = gc[1:] == gc[:-1]
    assert np.all(got_keys[1:][same] > got_keys[:-1][same]), f"{what}: keys not strictly ascending inside equal counts"
    assert np.array_equal(gc, np.sort(oc)[::-1][:n]), f"{what}: not the {rows} largest counts"
    assert are_groups(got_keys, gc, ok, oc), f"{what}: a returned row is not a group"


def check_select(got, ok, oc, lo, hi, what=""):
    gk, gc, n = got
    m = (oc >= np.uint64(max(lo, 1))) & (oc <= np.uint64(hi)) if lo <= hi else np.zeros(len(oc), bool)
    assert n == int(m.sum()) == len(gk) == len(gc), f"{what}: {n} matches, oracle {int(m.sum())}"
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], ok[m]) and np.array_equal(gc[order], oc[m]), what


def check_queries(q, ok, oc, what, pkg, bins=(1, 2, 17, 8192, 8193, 1 << 20), tops=None, ranges=None):
    """all three queries of one Hist / Accumulator against the oracle's groups (ok ascending)"""
    assert q.distinct == len(ok), what
    for n_bins in bins:
        got = q.spectrum(n_bins)
        assert np.array_equal(got, want_spectrum(oc, n_bins)), f"{what}: spectrum({n_bins})"
        assert int(got.sum()) == len(ok)
    mx = int(oc.max()) if len(oc) else 1
    if ranges is None:
        ranges = ((1, U64_MAX), (0, U64_MAX), (2, U64_MAX), (1, 1), (0, 1), (2, max(mx - 1, 2)), (mx, mx), (mx + 1, U64_MAX), (5, 3))
    for lo, hi in ranges:
        check_select(q.select(lo, hi), ok, oc, lo, hi, f"{what}: select({lo}, {hi})")
    for n in tops if tops is not None else (1, 7, 1000, len(ok), len(ok) + 5):
        n = min(n, pkg.TOP_MAX)
        gk, gc = q.top(n)
        check_top(gk, gc, ok, oc, n, f"{what}: top({n})")
    gk, gc = q.top(0)
    assert len(gk) == 0 and len(gc) == 0


def tiled(motif_words, L, n):
    words = np.tile(motif_words, (n + L - 1) // L)[: (n + 31) // 32].copy()
    if n % 32:
        words[-1] &= np.uint64((1 << (2 * (n % 32))) - 1)
    return words


def shape_inputs(k):
    """(name, words, n_bases, oracle keys ascending, oracle counts) of the four shapes"""
    out = []
    n = 1_200_000                                 # (more groups than DNAGPU_TOP_MAX at large k)
    w = orc.synth_words(0xC0C0 + k, n)
    out.append(("uniform", w, n) + orc.count_keys(orc.generate_kmers(w, n, k, faithful=False)))
    n = 1_000_000
    w = orc.synth_words_repeat(0xC1C0 + k, n, 1000).copy()
    w[100:104] = ONES                             # 128 G's: the all-ones key at k = 32, copies (padding slots) everywhere
    out.append(("repeat", w, n) + orc.count_keys(orc.generate_kmers(w, n, k, faithful=False)))
    L, n = 4096, 10_000_000                       # ~4096 groups of ~2400 rows: counts past one 11-bit digit
    w = tiled(orc.synth_words(0xC2C0 + k, L), L, n)
    phase_keys = orc.generate_kmers(w, n, k, count=L, faithful=False)
    rows = n - k + 1
    per = np.array([(rows - 1 - r) // L + 1 for r in range(L)], dtype=np.uint64)
    out.append(("motif", w, n) + add_up([(phase_keys, per, 1)]))
    n = 1_000_000
    out.append(("poly-A", np.zeros((n + 31) // 32, np.uint64), n, np.zeros(1, np.uint64), np.array([n - k + 1], np.uint64)))
    return out


@pytest.mark.gpu
def test_the_references_statements(ctx, g, ref_vectors):
    """test.sql:95-104: ORDER BY count(*) DESC over ATCGATCGATCGATCGACG, k = 5; test.sql:107-119: the distribution of the
    counts of ACGTACGTACGTAG, k = 8 -- through the binding and through the glue"""
    v = ref_vectors["count"][0]
    assert v["dna"] == "ATCGATCGATCGATCGACG" and v["k"] == 5
    w, n = orc.dna_encode(v["dna"])
    d = ctx.upload(w, n)
    want = sorted(((orc.kmer_encode(t)[1], c) for t, c in v["groups"].items()), key=lambda r: (-r[1], r[0]))
    for count in (ctx.count_kmers, ctx.count_kmers_unordered):
        h = count(d, v["k"])
        for n_top in (6, 100, 1):
            gk, gc = h.top(n_top)
            assert [int(c) for c in gc] == [4, 3, 3, 3, 1, 1][:n_top]
            assert orc.kmer_decode(int(gk[0]), 5) == "ATCGA"
            assert {orc.kmer_decode(int(a), 5): int(b) for a, b in zip(gk, gc)}.items() <= v["groups"].items()
            if n_top >= 6:
                assert [int(a) for a in gk] == [int(a) for a, _ in want]
        h.free()
    d.free()
    s = ref_vectors["summary"][0]
    assert s["dna"] == "ACGTACGTACGTAG" and s["k"] == 8
    w, n = orc.dna_encode(s["dna"])
    d = ctx.upload(w, n)
    h = ctx.count_kmers(d, s["k"])
    assert list(h.spectrum(4)) == [3, 2, 0, 0] and list(h.spectrum(2)) == [3, 2] and list(h.spectrum(1)) == [5]
    assert int(h.spectrum(4)[0]) == s["unique"] and int(h.spectrum(4).sum()) == s["distinct"]
    h.free()
    d.free()
    # the same through the glue
    rows, totals = g.count_kmers_top(v["dna"], v["k"], 6)
    assert [c for _, c in rows] == [4, 3, 3, 3, 1, 1] and str(rows[0][0]) == "ATCGA"
    assert {str(km): c for km, c in rows} == v["groups"]
    assert totals == (15, 6, 2)
    rows, _ = g.count_kmers_top(v["dna"], v["k"], 100)
    assert [c for _, c in rows] == [4, 3, 3, 3, 1, 1]
    rows, _ = g.count_kmers_top(v["dna"], v["k"], 1)
    assert [(str(km), c) for km, c in rows] == [("ATCGA", 4)]
    assert g.count_kmers_spectrum(s["dna"], s["k"], 4) == [3, 2, 0, 0]
    assert g.count_kmers_spectrum(s["dna"], s["k"], 2) == [3, 2]
    assert g.count_kmers_spectrum(s["dna"], s["k"], 1) == [5]
    with pytest.raises(g.GlueError):
        g.count_kmers_spectrum(s["dna"], s["k"], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 10, 21, 31, 32])
def test_queries_match_the_oracle_over_shapes(ctx, pkg, k):
    """uniform, repeat-rich with 32 G's, motif-tiled and poly-A sequences through dnagpu_count_kmers and
    dnagpu_count_kmers_unordered (the super-k-mer engine forced for k >= 21: padding slots): spectrum, select and top"""
    for name, words, n, ok, oc in shape_inputs(k):
        d = ctx.upload(words, n)
        for unordered in (False, True):
            ctx.set_debug(pkg.DEBUG_FORCE_SUPERKMER if (unordered and k >= 21) else 0)
            try:
                h = ctx.count_kmers_unordered(d, k) if unordered else ctx.count_kmers(d, k)
            finally:
                ctx.set_debug(0)
            before = h.summary()
            check_queries(h, ok, oc, f"{name} k={k} {'unordered' if unordered else 'ordered'}", pkg)
            assert h.summary() == before == orc.hist_summary(ok, oc)
            h.free()
        if name == "repeat" and k == 32:
            assert ONES in ok
        d.free()


def device_out(ctx, words):
    p = ctx.buffer_alloc(8 * (words + GAP))
    ctx.upload_u64(p, np.full(words + GAP, SENTINEL, dtype=np.uint64))
    return p


@pytest.mark.gpu
def test_cap_smaller_than_the_matches_and_device_outputs(ctx, pkg):
    """n_out is the full total whatever cap is; the rows written are distinct groups inside the range; nothing is written
    past cap (sentinel-filled device buffers); device outputs equal host outputs"""
    k, n = 31, 1_000_000
    w = orc.synth_words_repeat(0xC3C0, n, 1000).copy()
    w[100:104] = ONES
    ok, oc = orc.count_keys(orc.generate_kmers(w, n, k, faithful=False))
    d = ctx.upload(w, n)
    h = ctx.count_kmers_unordered(d, k)
    acc = ctx.accumulator(k)
    acc.add(h)
    for q, what in ((h, "hist"), (acc, "acc")):
        for lo, hi in ((1, U64_MAX), (2, U64_MAX), (1, 1)):
            m = (oc >= np.uint64(lo)) & (oc <= np.uint64(hi))
            total = int(m.sum())
            assert total > 100
            for cap in (0, 1, 100, total - 1, total, total + 7):
                gk, gc, n_out = q.select(lo, hi, cap=cap)
                assert n_out == total and len(gk) == len(gc) == min(cap, total), f"{what} select({lo},{hi}) cap={cap}"
                assert len(np.unique(gk)) == len(gk) and are_groups(gk, gc, ok, oc)
                assert np.all((gc >= np.uint64(lo)) & (gc <= np.uint64(hi)))
                dk, dc = device_out(ctx, cap), device_out(ctx, cap)
                assert q.select(lo, hi, cap=cap, on_device=True, out=(dk, dc)) == total
                ak, ac = ctx.download_u64(dk, cap + GAP), ctx.download_u64(dc, cap + GAP)
                wrote = min(cap, total)
                assert np.all(ak[wrote:] == SENTINEL) and np.all(ac[wrote:] == SENTINEL), f"{what}: a store past cap={cap}"
                assert len(np.unique(ak[:wrote])) == wrote and are_groups(ak[:wrote], ac[:wrote], ok, oc)
                assert np.all((ac[:wrote] >= np.uint64(lo)) & (ac[:wrote] <= np.uint64(hi)))
                if cap >= total:                  # all matches: the same set as the host call's
                    assert np.array_equal(np.sort(ak[:wrote]), np.sort(gk))
                # either output may be NULL
                assert q.select(lo, hi, cap=cap, on_device=True, out=(None, dc)) == total
                assert q.select(lo, hi, cap=cap, on_device=True, out=(dk, None)) == total
                ctx.buffer_free(dk)
                ctx.buffer_free(dc)
        for n_top in (1, 10, 5000):
            gk, gc = q.top(n_top)
            check_top(gk, gc, ok, oc, n_top, f"{what} top({n_top})")
            dk, dc = device_out(ctx, n_top), device_out(ctx, n_top)
            assert q.top(n_top, on_device=True, out=(dk, dc)) == n_top
            ak, ac = ctx.download_u64(dk, n_top + GAP), ctx.download_u64(dc, n_top + GAP)
            assert np.all(ak[n_top:] == SENTINEL) and np.all(ac[n_top:] == SENTINEL)
            check_top(ak[:n_top], ac[:n_top], ok, oc, n_top, f"{what} top({n_top}) on the device")
            assert np.array_equal(ac[:n_top], gc)
            ctx.buffer_free(dk)
            ctx.buffer_free(dc)
        # allocated by the binding
        dk, dc, rows = q.top(100, on_device=True)
        check_top(ctx.download_u64(dk, rows), ctx.download_u64(dc, rows), ok, oc, 100, what)
        ctx.buffer_free(dk)
        ctx.buffer_free(dc)
    acc.free()
    h.free()
    d.free()


@pytest.mark.gpu
def test_host_select_with_a_cap_above_the_groups_and_an_output_missing(ctx, pkg):
    """select into host arrays of more entries than there are groups: each output NULL in turn, and both; nothing is written
    behind the matches"""
    k, n = 9, 20_000
    w = orc.synth_words(0xC4C0, n)
    ok, oc = orc.count_keys(orc.generate_kmers(w, n, k, faithful=False))
    d = ctx.upload(w, n)
    h = ctx.count_kmers(d, k)
    acc = ctx.accumulator(k)
    acc.add(h)
    cap = len(ok) + 1000
    for q, obj in ((h, "hist"), (acc, "acc")):
        fn = getattr(pkg.lib(), f"dnagpu_{obj}_select")
        for lo, hi in ((1, U64_MAX), (2, 3)):
            m = (oc >= np.uint64(lo)) & (oc <= np.uint64(hi))
            total = int(m.sum())
            assert 0 < total
            for want_keys, want_counts in ((True, True), (True, False), (False, True), (False, False)):
                keys, counts = np.full(cap, SENTINEL, dtype=np.uint64), np.full(cap, SENTINEL, dtype=np.uint64)
                n_out = C.c_uint64()
                assert fn(ctx.h, q.h, lo, hi, keys.ctypes.data if want_keys else None, counts.ctypes.data if want_counts else None,
                          cap, C.byref(n_out), 0) == 0
                what = f"{obj} select({lo}, {hi}) keys={want_keys} counts={want_counts}"
                assert n_out.value == total, what
                for arr, wanted in ((keys, want_keys), (counts, want_counts)):
                    assert np.all(arr[total if wanted else 0:] == SENTINEL), f"{what}: a store it was not asked for"
                if want_keys:
                    assert np.array_equal(np.sort(keys[:total]), ok[m]), what
                if want_counts:
                    assert np.array_equal(np.sort(counts[:total]), np.sort(oc[m])), what
                if want_keys and want_counts:
                    assert np.array_equal(counts[:total][np.argsort(keys[:total])], oc[m]), what
    acc.free()
    h.free()
    d.free()


@pytest.mark.gpu
def test_queries_over_histograms_of_several_parts(pkg):
    """the one-process multi-rank count on one device: histograms of several parts (and their borrowed part views); all
    three queries against the ranks' summed downloads"""
    seed, k, n = 0xC4C0, 31, 64_000_000
    with pkg.Multi([0, 0], pkg.MULTI_COPY) as m:
        m.set_parts(3)
        d = m.synth(seed, n)
        hs = m.count_unordered(d, k)
        m.dna_free(d)
        assert any(h.n_parts > 1 for h in hs), [h.n_parts for h in hs]
        for h in hs:
            ok, oc = add_up([h.download() + (1,)])
            check_queries(h, ok, oc, f"{h.n_parts} parts", pkg, bins=(1, 2, 17, 8193), tops=(1, 1000, pkg.TOP_MAX),
                          ranges=((0, U64_MAX), (2, U64_MAX), (5, 3)))
            # a borrowed part view is a histogram like any other: the parts' spectra add up to the whole's
            if h.n_parts > 1:
                total = np.zeros(17, np.uint64)
                for i in range(h.n_parts):
                    part = pkg.Hist(h.ctx, C.c_void_p(pkg.lib().dnagpu_hist_part(h.h, i)))
                    total += part.spectrum(17)
                assert np.array_equal(total, h.spectrum(17))
        for h in hs:
            h.free()


@pytest.mark.gpu
def test_acc_queries_past_2_to_the_32(ctx, pkg):
    """a random table x3, a motif-tiled sequence x100 and poly-A x100: the poly-A group and the total pass 2^32 -- the high
    digits of the 64-bit radix select; the accumulator is unchanged afterwards"""
    k = 31
    n_t = 300_000
    wt = orc.synth_words(0xC5C0, n_t)
    dt = ctx.upload(wt, n_t)
    ht = ctx.count_kmers_unordered(dt, k)
    dt.free()
    tk, tc = orc.count_keys(orc.generate_kmers(wt, n_t, k, faithful=False))
    L, n_m = 4096, 5_000_000
    wm = tiled(orc.synth_words(0xC5C1, L), L, n_m)
    dm = ctx.upload(wm, n_m)
    hm = ctx.count_kmers_unordered(dm, k)
    dm.free()
    rows = n_m - k + 1
    mk, mc = add_up([(orc.generate_kmers(wm, n_m, k, count=L, faithful=False),
                      np.array([(rows - 1 - r) // L + 1 for r in range(L)], dtype=np.uint64), 1)])
    n_a = 50_000_000
    da = ctx.upload(np.zeros((n_a + 31) // 32, np.uint64), n_a)
    ha = ctx.count_kmers_unordered(da, k)
    da.free()
    acc = ctx.accumulator(k)
    plan = [(ht, 3), (hm, 100), (ha, 100)]
    for i in range(100):
        for h, mult in plan:
            if i < mult:
                acc.add(h)
    ek, ec = add_up([(tk, tc, 3), (mk, mc, 100), (np.zeros(1, np.uint64), np.array([n_a - k + 1], np.uint64), 100)])
    big = 100 * (n_a - k + 1)
    assert acc.total > 2 ** 32 and big > 2 ** 32 and ek[0] == 0 and int(ec[0]) == big
    before = (acc.summary(), acc.distinct, acc.total)
    dk0, dc0 = acc.download()
    check_queries(acc, ek, ec, "past 2^32", pkg, bins=(1, 2, 17, 8193))
    sp = acc.spectrum(1000)
    assert int(sp[-1]) == len(mk) + 1             # the motif's groups (~122000 each) and poly-A land in the last bin
    gk, gc, n_out = acc.select(2 ** 32)
    assert n_out == 1 and int(gk[0]) == 0 and int(gc[0]) == big
    gk, gc = acc.top(10)
    assert int(gk[0]) == 0 and int(gc[0]) == big
    check_top(gk, gc, ek, ec, 10, "top(10) past 2^32")
    assert (acc.summary(), acc.distinct, acc.total) == before
    dk1, dc1 = acc.download()
    assert np.array_equal(dk0, dk1) and np.array_equal(dc0, dc1)       # (the download order too)
    acc.free()
    for h, _ in plan:
        h.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 31])
def test_glue_aggregate_top(g, k):
    """count_kmers_agg_top over the rows of a table with a flush size of 2000 bases (dozens of batches)"""
    rng = np.random.default_rng(0xC6C0 + k)
    lens = rng.integers(20, 300, 300)
    starts = np.concatenate([[0], np.cumsum(lens)])
    text = orc.dna_decode(orc.synth_words_repeat(0xC6C0 + k, int(starts[-1]), 700), int(starts[-1]))
    rows = [text[int(starts[i]):int(starts[i + 1])] for i in range(len(lens))]
    rows.append("ACGT" * 1500)
    keys = np.concatenate([orc.generate_kmers(*orc.dna_encode(r), k, faithful=False) for r in rows])
    ok, oc = orc.count_keys(keys)
    g.set_agg_flush_bases(2_000)
    try:
        for n in (1, 50, len(ok) + 3):
            got, (total, distinct, unique) = g.count_kmers_agg_top(rows, k, n)
            gk = np.array([km.c.bit_sequence for km, _ in got], dtype=np.uint64)
            gc = np.array([c for _, c in got], dtype=np.uint64)
            check_top(gk, gc, ok, oc, n, f"agg top({n}) k={k}")
            assert all(km.c.length == k for km, _ in got)
            assert (total, distinct, unique) == (int(oc.sum()), len(ok), int((oc == 1).sum()))
    finally:
        g.set_agg_flush_bases(1 << 30)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["3", "3m1000"])
def test_queries_full_size_against_the_digests(ctx, pkg, cfg):
    """config 3 (k = 31 over 248956422 bases; uniform, and with a 1000-base motif): consistency of the three queries with
    the CPU oracle's committed digests, over the histogram and (config 3) over an accumulator holding it"""
    with open(os.path.join(ROOT, "tests", "golden", "config_digests.json")) as f:
        want = json.load(f)[cfg]
    d = ctx.synth(want["seed"], want["n_bases"], want["motif"])
    h = ctx.count_kmers_unordered(d, want["k"])
    d.free()
    objs = [(h, "hist")]
    acc = None
    if cfg == "3":
        acc = ctx.accumulator(want["k"])
        acc.add(h)
        objs.append((acc, "acc"))
    for q, what in objs:
        assert q.summary() == (want["total"], want["distinct"], want["unique"], want["checksum"])
        n_bins = 1 << 20
        assert want["max_count"] < n_bins
        sp = q.spectrum(n_bins)
        assert int(sp.sum()) == want["distinct"], what
        assert int(sp[0]) == want["unique"], what
        assert int(sp[-1]) == 0 and int(sp[want["max_count"] - 1]) >= 1 and not sp[want["max_count"]:].any()
        assert int((sp * np.arange(1, n_bins + 1, dtype=np.uint64)).sum()) == want["total"], what
        small = q.spectrum(256)
        assert np.array_equal(small[:255], sp[:255]) and int(small.sum()) == want["distinct"]
        _, _, n_out = q.select(2, U64_MAX, cap=0)
        assert n_out == want["distinct"] - want["unique"], what
        gk, gc = q.top(1000)
        assert len(gk) == 1000 and len(np.unique(gk)) == 1000
        assert np.all(gc[1:] <= gc[:-1]) and int(gc[0]) == want["max_count"] and int(gc.sum()) <= want["total"]
        same = gc[1:] == gc[:-1]
        assert np.all(gk[1:][same] > gk[:-1][same])
        # the counts of the rows are exactly the spectrum read from the top
        top_counts = []
        for b in np.flatnonzero(sp)[::-1]:
            top_counts += [int(b) + 1] * min(int(sp[b]), 1000 - len(top_counts))
            if len(top_counts) == 1000:
                break
        assert [int(c) for c in gc] == top_counts, what
    if acc is not None:
        acc.free()
    h.free()
