"""The count-ordered read of ALL groups (dnagpu_hist_rank / dnagpu_acc_rank -> dnagpu_ranking): the reference's
GROUP BY k.kmer ORDER BY count(*) DESC (test.sql:95) with no LIMIT, answered on the device by a counting sort by count class.
The expected answers are numpy over the oracle's groups: np.sort of the counts (reversed for DESC) must equal the returned
count sequence exactly, and the returned rows sorted by key must equal the oracle's (keys, counts) exactly.  CPU test: the
argument rules that need no device."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import load_package

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
BAD_ARG = 5
SENTINEL = np.uint64(0xC3C3C3C3C3C3C3C3)
GAP = 512                                         # sentinel words behind every device output
RANK_CLASSES = 2048                               # the class limit C of csrc/query_host.hip (= Q_DIGITS): counts >= C are the tail
SMALL_CLASSES, SMALL_CHUNK = 4, 2048              # ... and what DEBUG_RANK_SMALL makes of it and of the 2^20-row sort chunk


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


# ------------------------------------------------------------------ CPU: what needs no device

def test_rank_argument_rules_without_a_device(pkg, g):
    L = pkg.lib()
    out = C.c_void_p(0x1234)
    for obj in ("hist", "acc"):
        rank = getattr(L, f"dnagpu_{obj}_rank")
        for order in (2, -1, 77):                 # a bad order comes before the missing object
            assert rank(None, None, order, C.byref(out)) == BAD_ARG
        for order in (pkg.ORDER_COUNT_DESC, pkg.ORDER_COUNT_ASC):
            out.value = 0x1234
            assert rank(None, None, order, C.byref(out)) == BAD_ARG
            assert not out.value                  # *out = NULL whenever there is an out
            assert rank(None, None, order, None) == BAD_ARG
    assert L.dnagpu_ranking_read(None, None, 0, 0, None, None, 0) == BAD_ARG
    assert L.dnagpu_ranking_read(None, None, 5, 1, None, None, 1) == BAD_ARG
    assert L.dnagpu_ranking_rows(None) == 0
    assert L.dnagpu_ranking_order(None) == 0
    assert not L.dnagpu_ranking_device_keys(None) and not L.dnagpu_ranking_device_counts(None)
    L.dnagpu_ranking_free(None, None)
    assert pkg.abi_version() == 2
    assert (pkg.ORDER_COUNT_DESC, pkg.ORDER_COUNT_ASC, pkg.DEBUG_RANK_SMALL) == (0, 1, 1024)
    assert pkg.TOP_MAX == 1 << 20                 # (top keeps its limit)
    assert hasattr(pkg, "Ranking") and hasattr(pkg.Hist, "rank") and hasattr(pkg.Accumulator, "rank")
    for name in ("count_kmers_ordered_begin", "count_kmers_agg_order"):
        assert hasattr(g.lib(), name), name
    assert callable(g.count_kmers_ordered) and callable(g.count_kmers_agg_ordered)


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
    at = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return keys[at], np.add.reduceat(counts, at).astype(np.uint64)


def want_counts(oc, order):
    s = np.sort(oc)
    return s[::-1] if order == 0 else s


def check_rows(gk, gc, ok, oc, order, what):
    """the count sequence is exactly the sorted counts; the rows are exactly the oracle's groups (ok ascending)"""
    assert len(gk) == len(gc) == len(ok), f"{what}: {len(gk)} rows, want {len(ok)}"
    assert np.array_equal(gc, want_counts(oc, order)), f"{what}: the count sequence differs"
    o = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[o], ok) and np.array_equal(gc[o], oc), f"{what}: not the oracle's groups"


def check_rank(q, ok, oc, what, pkg, orders=(0, 1)):
    """q.rank() of a Hist / Accumulator in both orders; -> the DESC rows"""
    desc = None
    for order in orders:
        r = q.rank(order)
        assert r.rows == len(ok) == q.distinct and r.order == order, what
        gk, gc = r.read()
        r.free()
        check_rows(gk, gc, ok, oc, order, f"{what} order={order}")
        if order == pkg.ORDER_COUNT_DESC:
            desc = (gk, gc)
    return desc


def bases_tiled(motif_words, L, n):
    """n bases that repeat the first L bases of motif_words (L need not be a multiple of 32), packed"""
    sh = np.arange(32, dtype=np.uint64) * np.uint64(2)
    bases = ((motif_words[:, None] >> sh) & np.uint64(3)).reshape(-1)[:L]
    seq = np.resize(bases, ((n + 31) // 32) * 32)
    seq[n:] = 0
    return np.bitwise_or.reduce(seq.reshape(-1, 32) << sh, axis=1)


def motif_input(seed, k, L=600, C_=RANK_CLASSES):
    """a motif of L bases tiled over rows = L * C + L / 2 rows: half the phases have count C + 1, half have count C"""
    rows = L * C_ + L // 2
    n = rows + k - 1
    w = bases_tiled(orc.synth_words(seed, L), L, n)
    phase_keys = orc.generate_kmers(w, n, k, count=L, faithful=False)
    per = np.array([(rows - 1 - r) // L + 1 for r in range(L)], dtype=np.uint64)
    assert int((per == C_ + 1).sum()) == L // 2 and int((per == C_).sum()) == L - L // 2
    return (w, n) + add_up([(phase_keys, per, 1)])


_SHAPES = {}


def shape_inputs(k):
    """(name, words, n_bases, oracle keys ascending, oracle counts) of the four shapes; built once per k"""
    if k in _SHAPES:
        return _SHAPES[k]
    out = []
    n = 200_000                                   # ~100 tiles of 2048 slots, the last one partial
    w = orc.synth_words(0xD0C0 + k, n)
    out.append(("uniform", w, n) + orc.count_keys(orc.generate_kmers(w, n, k, faithful=False)))
    w = orc.synth_words_repeat(0xD1C0 + k, n, 1000).copy()
    w[100:104] = ONES                             # 128 G's: the all-ones key at k = 32
    out.append(("repeat", w, n) + orc.count_keys(orc.generate_kmers(w, n, k, faithful=False)))
    out.append(("poly-A", np.zeros((n + 31) // 32, np.uint64), n, np.zeros(1, np.uint64), np.array([n - k + 1], np.uint64)))
    out.append(("motif",) + motif_input(0xD2C0 + k, k))
    _SHAPES[k] = out
    return out


@pytest.mark.gpu
def test_the_references_statement_in_full(ctx, pkg, g, ref_vectors):
    """test.sql:95: ORDER BY count(*) DESC over ATCGATCGATCGATCGACG, k = 5, without a LIMIT -- binding and glue, both orders"""
    v = ref_vectors["count"][0]
    assert v["dna"] == "ATCGATCGATCGATCGACG" and v["k"] == 5
    w, n = orc.dna_encode(v["dna"])
    d = ctx.upload(w, n)
    for count in (ctx.count_kmers, ctx.count_kmers_unordered):
        h = count(d, v["k"])
        with h.rank() as r:
            assert r.rows == 6 and r.order == pkg.ORDER_COUNT_DESC
            gk, gc = r.read()
        assert [int(c) for c in gc] == [4, 3, 3, 3, 1, 1]
        assert orc.kmer_decode(int(gk[0]), 5) == "ATCGA"
        assert {orc.kmer_decode(int(a), 5): int(b) for a, b in zip(gk, gc)} == v["groups"]
        with h.rank(pkg.ORDER_COUNT_ASC) as r:
            gk, gc = r.read()
        assert [int(c) for c in gc] == [1, 1, 3, 3, 3, 4]
        assert {orc.kmer_decode(int(a), 5): int(b) for a, b in zip(gk, gc)} == v["groups"]
        h.free()
    d.free()
    rows, totals = g.count_kmers_ordered(v["dna"], v["k"])
    assert [c for _, c in rows] == [4, 3, 3, 3, 1, 1] and str(rows[0][0]) == "ATCGA"
    assert {str(km): c for km, c in rows} == v["groups"] and totals == (15, 6, 2)
    rows, totals = g.count_kmers_ordered(v["dna"], v["k"], descending=False)
    assert [c for _, c in rows] == [1, 1, 3, 3, 3, 4] and str(rows[-1][0]) == "ATCGA"
    assert {str(km): c for km, c in rows} == v["groups"] and totals == (15, 6, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 21, 32])
def test_rank_matches_the_oracle_over_shapes(ctx, pkg, k):
    """uniform (every count 1 at k >= 21), repeat-rich with 32 G's, poly-A and a motif whose phase counts straddle the class
    limit, through dnagpu_count_kmers and dnagpu_count_kmers_unordered (the super-k-mer engine forced for k >= 21: padding
    slots): rows == distinct, exact count sequence, exact groups, both orders, the source untouched; top(n) agrees"""
    for name, words, n, ok, oc in shape_inputs(k):
        d = ctx.upload(words, n)
        for unordered in (False, True):
            ctx.set_debug(pkg.DEBUG_FORCE_SUPERKMER if (unordered and k >= 21) else 0)
            try:
                h = ctx.count_kmers_unordered(d, k) if unordered else ctx.count_kmers(d, k)
            finally:
                ctx.set_debug(0)
            what = f"{name} k={k} {'unordered' if unordered else 'ordered'}"
            before = h.summary()
            _, dc = check_rank(h, ok, oc, what, pkg)
            assert h.summary() == before == orc.hist_summary(ok, oc), what
            for n_top in (1, 7, 1000):
                _, tc = h.top(n_top)
                assert np.array_equal(tc, dc[:n_top]), f"{what}: top({n_top})"
            h.free()
        if name == "repeat" and k == 32:
            assert ONES in ok
        if name == "uniform" and k >= 21:
            assert int(oc.max()) == 1
        if name == "uniform" and k == 5:
            assert len(ok) == 1024
        d.free()


def crafted_counts(small):
    """(keys, counts): ~1500 keys of counts 1 + (i * 40503) % 4099, 200 keys that share one count, three keys at each of
    C - 2 .. C + 2, one key of count 1 and the all-ones key; small: also 5000 keys of distinct counts >= 4"""
    rng = np.random.default_rng(0xD3C0)
    i = np.arange(1500, dtype=np.uint64)
    counts = [np.uint64(1) + (i * np.uint64(40503)) % np.uint64(4099), np.full(200, 3000, np.uint64),
              np.repeat(np.arange(RANK_CLASSES - 2, RANK_CLASSES + 3, dtype=np.uint64), 3), np.array([1, 2500], np.uint64)]
    if small:
        counts.append(np.arange(4, 5004, dtype=np.uint64))
    counts = np.concatenate(counts)
    keys = np.unique(rng.integers(0, 2 ** 63, 2 * len(counts), dtype=np.uint64))[: len(counts) - 1]
    keys = np.concatenate([rng.permutation(keys), [ONES]])           # (the all-ones key takes the last count)
    order = np.argsort(keys)
    return keys[order], counts[order]


def hist_of(ctx, keys, counts):
    rows = np.repeat(keys, counts.astype(np.int64))
    p = ctx.buffer_alloc(8 * len(rows))
    ctx.upload_u64(p, rows)
    h = ctx.count_keys_device(p, len(rows), 32)
    ctx.buffer_free(p)
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_crafted_count_distributions(ctx, pkg, small):
    """ties on both sides of the class limit, a class of 200 rows, and under DEBUG_RANK_SMALL (class limit 4, chunks of 2048
    rows) a tail of ~6700 rows that takes at least three peels"""
    ok, oc = crafted_counts(small)
    assert len(np.unique(ok)) == len(ok) and ok[-1] == ONES
    if small:
        assert int((oc >= SMALL_CLASSES).sum()) > 3 * SMALL_CHUNK
    h = hist_of(ctx, ok, oc)
    acc = ctx.accumulator(32)
    acc.add(h)
    ctx.set_debug(pkg.DEBUG_RANK_SMALL if small else 0)
    try:
        before = h.summary()
        check_rank(h, ok, oc, f"crafted small={small} hist", pkg)
        check_rank(acc, ok, oc, f"crafted small={small} acc", pkg)
        assert h.summary() == before
    finally:
        ctx.set_debug(0)
    acc.free()
    h.free()


def device_out(ctx, words):
    p = ctx.buffer_alloc(8 * (words + GAP))
    ctx.upload_u64(p, np.full(words + GAP, SENTINEL, dtype=np.uint64))
    return p


@pytest.mark.gpu
def test_windows_and_device_outputs(ctx, pkg):
    """windows of 1, 777, 65537 rows and the rest tile the ranking; device outputs land in sentinel-filled buffers and leave
    the words behind them alone; keys-only and counts-only reads; the window rule's errors"""
    name, words, n, ok, oc = shape_inputs(21)[1]
    assert name == "repeat" and len(ok) >= 70_000 and len(np.unique(oc)) > 3
    d = ctx.upload(words, n)
    h = ctx.count_kmers_unordered(d, 21)
    d.free()
    r = h.rank()
    h.free()
    rows = r.rows
    wk, wc = r.read()
    check_rows(wk, wc, ok, oc, 0, "whole read")
    parts, at = [], 0
    for size in (1, 777, 65_537, None):
        size = rows - at if size is None else size
        parts.append(r.read(at, size))
        at += size
    assert at == rows
    assert np.array_equal(np.concatenate([p[0] for p in parts]), wk) and np.array_equal(np.concatenate([p[1] for p in parts]), wc)
    assert np.array_equal(ctx.download_u64(r.device_keys, rows), wk) and np.array_equal(ctx.download_u64(r.device_counts, rows), wc)
    for first, count in ((0, rows), (12_345, 4_097), (rows - 1, 1)):
        dk, dc = device_out(ctx, count), device_out(ctx, count)
        assert r.read(first, count, on_device=True, out=(dk, dc)) == count
        ak, ac = ctx.download_u64(dk, count + GAP), ctx.download_u64(dc, count + GAP)
        assert np.array_equal(ak[:count], wk[first:first + count]) and np.array_equal(ac[:count], wc[first:first + count])
        assert np.all(ak[count:] == SENTINEL) and np.all(ac[count:] == SENTINEL)
        # either output may be NULL: the other array is written, the buffer passed over stays as it is
        ctx.upload_u64(dk, np.full(count + GAP, SENTINEL, dtype=np.uint64))
        assert r.read(first, count, on_device=True, out=(None, dc)) == count
        assert np.all(ctx.download_u64(dk, count + GAP) == SENTINEL)
        ctx.upload_u64(dc, np.full(count + GAP, SENTINEL, dtype=np.uint64))
        assert r.read(first, count, on_device=True, out=(dk, None)) == count
        assert np.array_equal(ctx.download_u64(dk, count), wk[first:first + count])
        assert np.all(ctx.download_u64(dc, count + GAP) == SENTINEL)
        ctx.buffer_free(dk)
        ctx.buffer_free(dc)
    dk, dc, got = r.read(5, 100, on_device=True)                       # allocated by the binding
    assert got == 100 and np.array_equal(ctx.download_u64(dk, 100), wk[5:105]) and np.array_equal(ctx.download_u64(dc, 100), wc[5:105])
    ctx.buffer_free(dk)
    ctx.buffer_free(dc)
    L = pkg.lib()
    buf = np.full(8, SENTINEL, dtype=np.uint64)
    assert L.dnagpu_ranking_read(ctx.h, r.h, 3, 4, buf.ctypes.data, None, 0) == 0          # keys only, host
    assert np.array_equal(buf[:4], wk[3:7]) and np.all(buf[4:] == SENTINEL)
    assert L.dnagpu_ranking_read(ctx.h, r.h, 3, 4, None, buf.ctypes.data, 0) == 0          # counts only
    assert np.array_equal(buf[:4], wc[3:7]) and np.all(buf[4:] == SENTINEL)
    assert L.dnagpu_ranking_read(ctx.h, r.h, rows, 0, buf.ctypes.data, buf.ctypes.data, 0) == 0
    assert L.dnagpu_ranking_read(ctx.h, r.h, 0, rows, None, None, 0) == 0
    assert L.dnagpu_ranking_read(ctx.h, r.h, rows + 1, 0, buf.ctypes.data, None, 0) == BAD_ARG
    assert L.dnagpu_ranking_read(ctx.h, r.h, 10, rows - 10 + 1, buf.ctypes.data, None, 0) == BAD_ARG
    assert L.dnagpu_ranking_read(None, r.h, 0, 1, buf.ctypes.data, None, 0) == BAD_ARG
    assert L.dnagpu_ranking_read(ctx.h, None, 0, 1, buf.ctypes.data, None, 0) == BAD_ARG
    assert np.all(buf[4:] == SENTINEL)
    r.free()


@pytest.mark.gpu
def test_a_ranking_is_a_snapshot(ctx, pkg):
    """the histogram may be freed and the accumulator may take further adds: the ranking stays; the accumulator's download
    order is the same before and after a rank"""
    k = 21
    _, w1, n1, ok1, oc1 = shape_inputs(k)[1]
    _, w2, n2, ok2, oc2 = shape_inputs(k)[0]
    d1, d2 = ctx.upload(w1, n1), ctx.upload(w2, n2)
    h1, h2 = ctx.count_kmers_unordered(d1, k), ctx.count_kmers(d2, k)
    d1.free()
    d2.free()
    r = h1.rank(pkg.ORDER_COUNT_ASC)
    acc = ctx.accumulator(k)
    acc.add(h1)
    h1.free()
    junk = ctx.buffer_alloc(8 * 3 * len(ok1))                          # (the freed arrays are taken again and overwritten)
    ctx.upload_u64(junk, np.full(3 * len(ok1), SENTINEL, dtype=np.uint64))
    check_rows(*r.read(), ok1, oc1, 1, "after the histogram was freed")
    ctx.buffer_free(junk)
    r.free()
    dk0, dc0 = acc.download()
    before = acc.summary()
    ra = acc.rank()
    dk1, dc1 = acc.download()
    assert np.array_equal(dk0, dk1) and np.array_equal(dc0, dc1) and acc.summary() == before
    acc.add(h2)
    acc.add(h2)                                                        # (twice: the new groups' counts are 2)
    check_rows(*ra.read(), ok1, oc1, 0, "after further adds")
    ek, ec = add_up([(ok1, oc1, 1), (ok2, oc2, 2)])
    check_rank(acc, ek, ec, "the sums", pkg)
    check_rows(*ra.read(), ok1, oc1, 0, "after another rank")
    ra.free()
    acc.free()
    h2.free()


@pytest.mark.gpu
def test_rank_over_histograms_of_several_parts(pkg):
    """the one-process multi-rank count on one device (as test_queries_over_histograms_of_several_parts builds it): every
    rank's histogram and every borrowed part view.  Sorting 3 * 10^7 keys per rank on the host would take many seconds, so
    the whole histograms are checked by what needs no sort -- the count sequence against the spectrum, and the rows against
    the histogram's own order-independent digest of its (key, count) pairs (oracle.hist_summary over the rows read) -- and
    the first part view of every rank exactly, against the groups select(1, max) returns for it"""
    seed, k, n = 0xD4C0, 31, 64_000_000
    with pkg.Multi([0, 0], pkg.MULTI_COPY) as m:
        m.set_parts(3)
        d = m.synth(seed, n)
        hs = m.count_unordered(d, k)
        m.dna_free(d)
        assert any(h.n_parts > 1 for h in hs), [h.n_parts for h in hs]
        total_rows = 0
        for rank, h in enumerate(hs):
            order = rank % 2                                           # (one order per rank: the rows cross the bus once)
            with h.rank(order) as r:
                assert r.rows == h.distinct
                gk, gc = r.read()
            sp = h.spectrum(64)
            assert int(sp[-1]) == 0
            seq = np.repeat(np.arange(1, 65, dtype=np.uint64), sp.astype(np.int64))
            assert np.array_equal(gc, seq[::-1] if order == 0 else seq), f"{h.n_parts} parts order={order}"
            assert orc.hist_summary(gk, gc) == h.summary()
            total_rows += len(gk)
            if h.n_parts > 1:
                view_rows = 0
                for i in range(h.n_parts):
                    part = pkg.Hist(h.ctx, C.c_void_p(pkg.lib().dnagpu_hist_part(h.h, i)))
                    with part.rank(1 - order) as r:
                        view_rows += r.rows
                        if i == 0:
                            sk, sc, n_sel = part.select(1)
                            assert n_sel == r.rows > 0
                            o = np.argsort(sk, kind="stable")
                            check_rows(*r.read(), sk[o], sc[o], 1 - order, "part view 0")
                assert view_rows == h.distinct
        assert total_rows == sum(h.distinct for h in hs)
        for h in hs:
            h.free()


@pytest.mark.gpu
def test_acc_rank_past_2_to_the_32(ctx, pkg):
    """the motif's groups (counts around the class limit) x3, a two-phase repeat x150 and poly-A x100: three counts pass 2^32
    and two of them differ by one -- the count sequence is exact in 64 bits, in both orders, plainly and under
    DEBUG_RANK_SMALL; empty sources give 0 rows and NULL arrays"""
    k = 31
    wm, n_m, mk, mc = motif_input(0xD5C0, k)
    dm = ctx.upload(wm, n_m)
    hm = ctx.count_kmers_unordered(dm, k)
    dm.free()
    n_a = 50_000_000
    da = ctx.upload(np.zeros((n_a + 31) // 32, np.uint64), n_a)
    ha = ctx.count_kmers_unordered(da, k)
    da.free()
    n_b = 60_000_001
    wb = np.full((n_b + 31) // 32, 0x4444444444444444, np.uint64)     # ACAC...: two groups, rows / 2 each (one of them + 1)
    wb[-1] &= np.uint64((1 << (2 * (n_b % 32))) - 1)
    db = ctx.upload(wb, n_b)
    hb = ctx.count_kmers_unordered(db, k)
    db.free()
    rows_b = n_b - k + 1
    bk, bc = add_up([(orc.generate_kmers(wb, n_b, k, count=2, faithful=False),
                      np.array([(rows_b + 1) // 2, rows_b // 2], dtype=np.uint64), 1)])
    acc = ctx.accumulator(k)
    empty = acc.rank()
    assert empty.rows == 0 and not empty.device_keys and not empty.device_counts
    ek_, ec_ = empty.read(0, 0)
    assert len(ek_) == 0 and len(ec_) == 0
    assert pkg.lib().dnagpu_ranking_read(ctx.h, empty.h, 1, 0, None, None, 0) == BAD_ARG
    empty.free()
    plan = [(hm, 3), (hb, 150), (ha, 100)]
    for h, mult in plan:
        for _ in range(mult):
            acc.add(h)
    ek, ec = add_up([(mk, mc, 3), (bk, bc, 150), (np.zeros(1, np.uint64), np.array([n_a - k + 1], np.uint64), 100)])
    assert int((ec > np.uint64(2 ** 32)).sum()) == 3 and len(np.unique(ec[ec > np.uint64(2 ** 32)])) == 3
    assert int(bc[0]) != int(bc[1]) and abs(int(bc[0]) - int(bc[1])) == 1
    before = (acc.summary(), acc.distinct, acc.total)
    for flags in (0, pkg.DEBUG_RANK_SMALL):
        ctx.set_debug(flags)
        try:
            gk, gc = check_rank(acc, ek, ec, f"past 2^32 flags={flags}", pkg)
        finally:
            ctx.set_debug(0)
        assert int(gc[0]) == 100 * (n_a - k + 1) and int(gk[0]) == 0
    assert (acc.summary(), acc.distinct, acc.total) == before
    acc.free()
    for h, _ in plan:
        h.free()
    # an empty histogram (no k-mer fits): 0 rows, no arrays
    w, n = orc.dna_encode("ACGT")
    d = ctx.upload(w, n)
    h = ctx.count_kmers(d, 8)
    assert h.distinct == 0
    for order in (0, 1):
        r = h.rank(order)
        assert r.rows == 0 and r.order == order and not r.device_keys and not r.device_counts
        gk, gc = r.read(0, 0)
        assert len(gk) == 0 and len(gc) == 0
        r.free()
    h.free()
    d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 31])
def test_glue_aggregate_ordered(g, k):
    """count_kmers_agg_ordered over the rows of a table with a flush size of 500 bases (many batches), both orders; a late
    count_kmers_agg_order is refused as a late count_kmers_agg_top is"""
    rng = np.random.default_rng(0xD6C0 + k)
    lens = rng.integers(20, 200, 40)
    starts = np.concatenate([[0], np.cumsum(lens)])
    text = orc.dna_decode(orc.synth_words_repeat(0xD6C0 + k, int(starts[-1]), 300), int(starts[-1]))
    rows = [text[int(starts[i]):int(starts[i + 1])] for i in range(len(lens))]
    rows.append("ACGT" * 600)
    keys = np.concatenate([orc.generate_kmers(*orc.dna_encode(r), k, faithful=False) for r in rows])
    ok, oc = orc.count_keys(keys)
    g.set_agg_flush_bases(500)
    try:
        for descending in (True, False):
            got, (total, distinct, unique) = g.count_kmers_agg_ordered(rows, k, descending)
            gk = np.array([km.c.bit_sequence for km, _ in got], dtype=np.uint64)
            gc = np.array([c for _, c in got], dtype=np.uint64)
            check_rows(gk, gc, ok, oc, 0 if descending else 1, f"agg ordered k={k} descending={descending}")
            assert all(km.c.length == k for km, _ in got)
            assert (total, distinct, unique) == (int(oc.sum()), len(ok), int((oc == 1).sum()))
    finally:
        g.set_agg_flush_bases(1 << 30)
    L = g.lib()
    a = L.count_kmers_agg_begin(k)
    assert a
    try:
        row = g.dna(rows[0])
        assert L.count_kmers_agg_add(a, row.p)
        km, cnt = g._Kmer(), C.c_int64()
        assert L.count_kmers_agg_next(a, C.byref(km), C.byref(cnt))
        assert not L.count_kmers_agg_order(a, True)
        assert L.dna_glue_errmsg().decode() == "count_kmers_agg_order: called after the first row was served or the aggregate failed"
        assert not L.count_kmers_agg_top(a, 5)
        assert L.dna_glue_errmsg().decode() == "count_kmers_agg_top: called after the first row was served or the aggregate failed"
    finally:
        L.count_kmers_agg_end(a)
