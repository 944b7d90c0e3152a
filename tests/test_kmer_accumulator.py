"""The k-mer accumulator (dnagpu_acc_*): histograms added up on the device into 64-bit counts -- the HashAggregate of
test.sql:140-150 over a table of any size, batch by batch -- and the glue's table aggregate built on it.  CPU tests: the
argument rules that need no device; GPU tests: parity with the oracle, past 2^32, growth, errors, full size, the glue."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import ROOT, load_package

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
INVALID_K, BAD_ARG = 1, 5


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


# ------------------------------------------------------------------ CPU: what needs no device

def test_acc_argument_rules_without_a_device(pkg):
    L = pkg.lib()
    out = C.c_void_p()
    assert L.dnagpu_acc_create(None, 0, C.byref(out)) == INVALID_K
    assert L.dnagpu_acc_create(None, 33, C.byref(out)) == INVALID_K
    assert L.dnagpu_acc_create(None, 10, C.byref(out)) == BAD_ARG        # (no context)
    assert L.dnagpu_acc_add(None, None, None) == BAD_ARG
    assert L.dnagpu_acc_summary(None, None, None, None, None) == BAD_ARG
    assert L.dnagpu_acc_download(None, None, 0, 0, None, None) == BAD_ARG
    assert L.dnagpu_acc_distinct(None) == 0 and L.dnagpu_acc_total(None) == 0
    L.dnagpu_acc_free(None, None)


def test_glue_aggregate_bad_k_is_the_references_error(g):
    for k in (0, 33, -1):
        with pytest.raises(g.GlueError) as ei:
            g.count_kmers_agg([], k)
        assert str(ei.value) == "Invalid k value: must be between 1 and 32"          # dna.c:773


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def table_of_sequences(seed, n_seqs, lo, hi):
    """n_seqs sequences of lo .. hi bases back to back in one packed stream (+ a few empty ones and some shorter than any k):
    -> (words, starts)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n_seqs)
    lens[rng.integers(0, n_seqs, max(1, n_seqs // 50))] = 0
    lens[rng.integers(0, n_seqs, max(1, n_seqs // 50))] = rng.integers(1, 8)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return orc.synth_words(seed, int(starts[-1])), starts


def sub_table(words, starts, a, b):
    """sequences [a, b) of a table as a packed stream of their own -> (words, n_bases, starts)"""
    n = int(starts[-1])
    lo, hi = int(starts[a]), int(starts[b])
    w, nb = orc.dna_encode(orc.dna_decode(words, n)[lo:hi]) if hi > lo else (np.zeros(1, np.uint64), 0)
    return w, nb, starts[a:b + 1] - np.uint64(lo)


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


def check_acc(acc, ok, oc, what):
    gk, gc = acc.download()
    assert acc.distinct == len(ok), f"{what}: {acc.distinct} groups, oracle {len(ok)}"
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], ok), what + " keys"
    assert np.array_equal(gc[order], oc), what + " counts"
    assert acc.total == int(oc.sum(dtype=np.uint64)), what + " total"
    assert acc.summary() == orc.hist_summary(ok, oc), what + " summary"


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 21, 31, 32])
def test_acc_adds_the_batches_of_a_table(ctx, pkg, k):
    """a table counted in four batches (dnagpu_count_kmers_batch each, the super-k-mer engine forced on one at k >= 21), the
    batches added into one accumulator == the oracle's count over all rows; == the dnagpu_hist_merge chain below 2^32; plus a
    repeat-rich histogram with padding slots (and 32 G's at k = 32), an empty histogram, a histogram added twice, and an
    accumulator holding one histogram reporting exactly its summary"""
    words, starts = table_of_sequences(0xACC0 + k, 6_000, 40, 400)
    n_seqs = len(starts) - 1
    cuts = [0, 1_500, 2_900, 4_700, n_seqs]
    acc = ctx.accumulator(k)
    hists, devs = [], []
    for i in range(4):
        w, nb, st = sub_table(words, starts, cuts[i], cuts[i + 1])
        d = ctx.upload(w, nb)
        ctx.set_debug(pkg.DEBUG_FORCE_SUPERKMER if (k >= 21 and i == 1) else 0)
        try:
            h = ctx.count_kmers_batch(d, st, k)
        finally:
            ctx.set_debug(0)
        acc.add(h)
        hists.append(h)
        devs.append(d)
    ok, oc = orc.count_keys(orc.generate_kmers_table(words, starts, k))
    check_acc(acc, ok, oc, f"four batches, k={k}")
    # the dnagpu_hist_merge chain of the same batches (below 2^32): the same summary
    m = hists[0].merge(hists[1])
    for h in hists[2:]:
        m2 = m.merge(h)
        m.free()
        m = m2
    assert m.summary() == acc.summary(), f"merge chain, k={k}"
    m.free()
    # an empty histogram changes nothing
    d0 = ctx.upload(np.zeros(1, np.uint64), 3)
    h0 = ctx.count_kmers_batch(d0, np.array([0, 3], np.uint64), k) if k > 3 else None
    if h0 is not None:
        assert h0.distinct == 0
        acc.add(h0)
        h0.free()
        check_acc(acc, ok, oc, f"+ empty, k={k}")
    d0.free()
    # a repeat-rich sequence (copies: padding slots in the unordered arrays) with 32 G's, added twice
    wr = orc.synth_words_repeat(5 + k, 400_000, 1000).copy()
    wr[100:104] = ONES
    dr = ctx.upload(wr, 400_000)
    hr = ctx.count_kmers_unordered(dr, k)
    if not hr.is_sorted:
        assert hr.extent >= hr.distinct
    rk, rc = orc.count_keys(orc.generate_kmers(wr, 400_000, k, faithful=False))
    single = ctx.accumulator(k)
    single.add(hr)
    assert single.summary() == hr.summary(), f"one histogram, k={k}"
    check_acc(single, rk, rc, f"repeat-rich alone, k={k}")
    single.add(hr)
    check_acc(single, rk, rc * np.uint64(2), f"repeat-rich twice, k={k}")
    single.free()
    if k == 32:
        assert ONES in rk
    acc.add(hr)
    ak, ac = add_up([(ok, oc, 1), (rk, rc, 1)])
    check_acc(acc, ak, ac, f"batches + repeat-rich, k={k}")
    for h in hists + [hr]:
        h.free()
    for d in devs + [dr]:
        d.free()
    acc.free()


@pytest.mark.gpu
def test_acc_takes_histograms_of_several_parts(pkg):
    """the one-process multi-rank count on one device (ranks share it): histograms of several parts that record no k.  The
    ranks' groups (disjoint; their parity with the oracle is test_gpu_parity's) are what the accumulator must hold."""
    seed, k, n = 0xACC5, 31, 64_000_000           # (>= 4 coarse buckets: an owner cuts its range into groups)
    with pkg.Multi([0, 0], pkg.MULTI_COPY) as m:
        m.set_parts(3)
        d = m.synth(seed, n)
        hs = m.count_unordered(d, k)
        m.dna_free(d)
        assert any(h.n_parts > 1 for h in hs), [h.n_parts for h in hs]
        ok, oc = add_up([h.download() + (1,) for h in hs])
        assert sum(h.total for h in hs) == n - k + 1
        acc = m.ranks[0].accumulator(k)
        for h in hs:
            acc.add(h)
        check_acc(acc, ok, oc, "multi-rank parts")
        acc.free()
        for h in hs:
            h.free()


def motif_hist(ctx, L, n, k, seed):
    """a sequence that tiles an L-base motif over n bases (about L groups of n / L rows) -> (hist, oracle keys, counts)"""
    motif = orc.synth_words(seed, L)
    words = np.tile(motif, (n + L - 1) // L)[: (n + 31) // 32].copy()
    if n % 32:
        words[-1] &= np.uint64((1 << (2 * (n % 32))) - 1)
    d = ctx.upload(words, n)
    h = ctx.count_kmers_unordered(d, k)
    d.free()
    # row p holds the key of phase p mod L: the oracle's first L rows, each phase's row count
    phase_keys = orc.generate_kmers(words, n, k, count=L, faithful=False)
    rows = n - k + 1
    per = np.array([(rows - 1 - r) // L + 1 for r in range(L)], dtype=np.uint64)
    keys, counts = add_up([(phase_keys, per, 1)])
    return h, keys, counts


@pytest.mark.gpu
def test_acc_counts_past_2_to_the_32(ctx):
    """a random table, a motif-tiled sequence (~4096 groups of 5 * 10^7 rows) and poly-A (one group of 5 * 10^7) added 3, 100
    and 100 times: the total and the poly-A group pass 2^32, every group == the oracle's count x its multiplicity"""
    k = 31
    words, starts = table_of_sequences(0xACC1, 2_000, 50, 300)
    d = ctx.upload(words, int(starts[-1]))
    ht = ctx.count_kmers_batch(d, starts, k)
    d.free()
    tk, tc = orc.count_keys(orc.generate_kmers_table(words, starts, k))
    hm, mk, mc = motif_hist(ctx, 4096, 50_000_000, k, 0xACC2)
    n_a = 50_000_000
    da = ctx.upload(np.zeros((n_a + 31) // 32, np.uint64), n_a)
    ha = ctx.count_kmers_unordered(da, k)
    da.free()
    assert ha.distinct == 1 and ha.total == n_a - k + 1
    acc = ctx.accumulator(k)
    plan = [(ht, 3), (hm, 100), (ha, 100)]
    for i in range(100):                         # interleaved, as batches of a real table arrive
        for h, mult in plan:
            if i < mult:
                acc.add(h)
    ek, ec = add_up([(tk, tc, 3), (mk, mc, 100), (np.zeros(1, np.uint64), np.array([n_a - k + 1], np.uint64), 100)])
    assert acc.total > 2 ** 32
    assert int(ec[0]) == 100 * (n_a - k + 1) > 2 ** 32 and ek[0] == 0     # (poly-A: key 0)
    check_acc(acc, ek, ec, "past 2^32")
    acc.free()
    for h, _ in plan:
        h.free()


@pytest.mark.gpu
def test_acc_grows_and_windows_tile_the_groups(ctx):
    """from a small table to > 10^7 groups: several splits, some of them before the merge of a large add; download windows
    of odd sizes tile the groups exactly once"""
    k = 31
    acc = ctx.accumulator(k)
    keys = []
    # (seeds far apart: word w of a synthetic sequence is splitmix64(seed + w), so near seeds give shifted copies)
    for seed, n in ((0xACC10 << 32, 50_000), (0xACC11 << 32, 700_000), (0xACC12 << 32, 3_000_000), (0xACC13 << 32, 7_000_000)):
        d = ctx.synth(seed, n)
        h = ctx.count_kmers_unordered(d, k)
        acc.add(h)
        h.free()
        keys.append(orc.generate_kmers(orc.synth_words(seed, n), n, k, faithful=False))
        d.free()
    ok, oc = orc.count_keys(np.concatenate(keys))
    assert len(ok) > 10_000_000
    check_acc(acc, ok, oc, "grown")
    got_k, got_c, first = [], [], 0
    for w in (1, 999_983, 3, 4_000_037, 77, acc.distinct):
        w = min(w, acc.distinct - first)
        if w <= 0:
            break
        a, b = acc.download(first, w)
        got_k.append(a)
        got_c.append(b)
        first += w
    assert first == acc.distinct
    gk, gc = np.concatenate(got_k), np.concatenate(got_c)
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], ok) and np.array_equal(gc[order], oc)
    acc.free()


@pytest.mark.gpu
def test_acc_errors_leave_it_unchanged(ctx, pkg):
    L = pkg.lib()
    out = C.c_void_p()
    for k in (0, 33):
        assert L.dnagpu_acc_create(ctx.h, k, C.byref(out)) == INVALID_K
    assert L.dnagpu_acc_create(ctx.h, 10, None) == BAD_ARG
    n = 300_000
    d = ctx.synth(0xACC20, n)
    h31, h21 = ctx.count_kmers_unordered(d, 31), ctx.count_kmers_unordered(d, 21)
    acc = ctx.accumulator(31)
    acc.add(h31)
    before = (acc.distinct, acc.total, acc.summary())
    with pytest.raises(pkg.DnaGpuError) as ei:
        acc.add(h21)
    assert ei.value.code == BAD_ARG
    assert (acc.distinct, acc.total, acc.summary()) == before
    assert L.dnagpu_acc_add(ctx.h, acc.h, None) == BAD_ARG
    assert L.dnagpu_acc_add(ctx.h, None, h31.h) == BAD_ARG
    assert L.dnagpu_acc_add(None, acc.h, h31.h) == BAD_ARG
    assert L.dnagpu_acc_summary(None, acc.h, None, None, None) == BAD_ARG
    assert L.dnagpu_acc_download(ctx.h, acc.h, acc.distinct, 1, None, None) == BAD_ARG
    assert (acc.distinct, acc.total, acc.summary()) == before
    for o in (acc, h31, h21, d):
        o.free()


@pytest.mark.gpu
def test_acc_full_size_config3(ctx):
    """config 3's histogram (k = 31 over 248956422 bases) into an empty accumulator: the oracle's digest"""
    with open(os.path.join(ROOT, "tests", "golden", "config_digests.json")) as f:
        want = json.load(f)["3"]
    d = ctx.synth(want["seed"], want["n_bases"])
    h = ctx.count_kmers_unordered(d, want["k"])
    d.free()
    acc = ctx.accumulator(want["k"])
    acc.add(h)
    h.free()
    assert acc.summary() == (want["total"], want["distinct"], want["unique"], want["checksum"])
    acc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 31])
def test_glue_aggregate_over_a_table(g, k):
    """count_kmers_agg over the rows of a table with a flush size of 2000 bases (dozens of batches): the oracle's
    groups, and test.sql:140-150's sum(count), count(*), count(*) FILTER (WHERE count = 1)"""
    words, starts = table_of_sequences(0xACC30 + k, 400, 20, 300)
    n = int(starts[-1])
    text = orc.dna_decode(words, n)
    rows = [text[int(starts[i]):int(starts[i + 1])] for i in range(len(starts) - 1)]
    rows = [r for r in rows if r]                 # (a `dna` value is never empty)
    rows.append("ACGT" * 1500)                    # a row longer than the flush size: a batch of its own
    g.set_agg_flush_bases(2_000)
    try:
        got, (total, distinct, unique) = g.count_kmers_agg(rows, k)
    finally:
        g.set_agg_flush_bases(1 << 30)
    keys = np.concatenate([orc.generate_kmers(*orc.dna_encode(r), k, faithful=False) for r in rows])
    ok, oc = orc.count_keys(keys)
    gk = np.array([km.c.bit_sequence for km, _ in got], dtype=np.uint64)
    gc = np.array([c for _, c in got], dtype=np.uint64)
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], ok) and np.array_equal(gc[order], oc)
    assert all(km.c.length == k for km, _ in got)
    assert (total, distinct, unique) == (int(oc.sum()), len(ok), int((oc == 1).sum()))
