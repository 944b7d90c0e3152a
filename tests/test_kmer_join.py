"""The hash join of two accumulators (dnagpu_acc_join): JOIN / INTERSECT, EXCEPT and LEFT JOIN of two counted k-mer sets on
the device, with their statistics, and the glue's count_kmers_join over two table aggregates.  CPU tests: the argument rules
that need no device.  GPU tests: every case under both forced paths (partition, direct) against the CPU oracle's counts
joined with numpy -- rows compared as sets sorted by key, all six statistics and n_out."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import load_package

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
BAD_ARG = 5
SEED = 0x10A0 << 32
SENTINEL = np.uint64(0x5E5E5E5E5E5E5E5E)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


# ------------------------------------------------------------------ CPU: what needs no device

def test_join_argument_rules_without_a_device(pkg):
    L = pkg.lib()
    n = C.c_uint64(77)
    st = pkg.JoinStats()
    for kind in (-1, 3, 100):
        assert L.dnagpu_acc_join(None, None, None, kind, None, None, None, 0, C.byref(n), C.byref(st), 0) == BAD_ARG
    for kind in (0, 1, 2):                       # NULL objects (no context, no accumulators)
        assert L.dnagpu_acc_join(None, None, None, kind, None, None, None, 0, C.byref(n), C.byref(st), 0) == BAD_ARG
        assert L.dnagpu_acc_join(None, None, None, kind, None, None, None, 0, None, None, 0) == BAD_ARG
    assert n.value == 77
    assert L.dnagpu_acc_partitions(None) == 0
    assert (pkg.JOIN_INNER, pkg.JOIN_ANTI, pkg.JOIN_LEFT) == (0, 1, 2)
    assert (pkg.DEBUG_JOIN_PARTITION, pkg.DEBUG_JOIN_DIRECT) == (2048, 4096)


def test_glue_join_refuses_a_bad_kind_character(g):
    with g.count_kmers_table_agg(5) as a, g.count_kmers_table_agg(5) as b:
        for kind in ("x", "I", "", "j"):
            with pytest.raises(g.GlueError) as ei:
                g.count_kmers_join(a, b, kind)
            assert "unknown kind" in str(ei.value)


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["partition", "direct"])
def path(request, ctx, pkg):
    """every join of the test runs on the forced path"""
    flag = pkg.DEBUG_JOIN_PARTITION if request.param == "partition" else pkg.DEBUG_JOIN_DIRECT
    ctx.set_debug(flag)
    yield flag
    ctx.set_debug(0)


_ORACLE = {}


def oracle_counts(seed, n, k, times=1):
    """the oracle's groups of the synthetic sequence (seed, n), counts x times; computed once, never modified"""
    key = (seed, n, k)
    if key not in _ORACLE:
        ks, cs = orc.count_kmers(orc.synth_words(seed, n), n, k)
        ks.setflags(write=False)
        cs = cs.astype(np.uint64)
        cs.setflags(write=False)
        _ORACLE[key] = (ks, cs)
    ks, cs = _ORACLE[key]
    return ks, cs * np.uint64(times)


@pytest.fixture(scope="module")
def accs(ctx):
    """accumulators over synthetic sequences, built once per (seed, n, k, times) and only ever read"""
    made = {}

    def get(seed, n, k, times=1):
        key = (seed, n, k, times)
        if key not in made:
            d = ctx.synth(seed, n)
            h = ctx.count_kmers_unordered(d, k)
            a = ctx.accumulator(k)
            for _ in range(times):
                a.add(h)
            h.free()
            d.free()
            made[key] = a
        return made[key]

    yield get
    for a in made.values():
        a.free()


def oracle_join(left, right, kind):
    """(keys ascending, count_left, count_right, the six statistics) of the join of two (keys ascending, counts)"""
    lk, lc = left
    rk, rc = right
    _, il, ir = np.intersect1d(lk, rk, assume_unique=True, return_indices=True)
    cr_all = np.zeros(len(lk), dtype=np.uint64)
    cr_all[il] = rc[ir]
    hit = np.isin(lk, rk)
    assert int(hit.sum()) == len(il)
    sel = hit if kind == 0 else ~hit if kind == 1 else np.ones(len(lk), dtype=bool)
    keys, cl, cr = lk[sel], lc[sel], cr_all[sel]
    pos = cr > 0
    stats = (len(keys), int(cl.sum(dtype=np.uint64)), int(cr.sum(dtype=np.uint64)), int(np.minimum(cl, cr).sum(dtype=np.uint64)),
             orc.hist_summary(keys, cl)[3] if len(keys) else 0, orc.hist_summary(keys[pos], cr[pos])[3] if pos.any() else 0)
    return keys, cl, cr, stats


def check_join(la, ra, left, right, kind, what):
    """Accumulator.join against the oracle join: its first call's n_out sizes the arrays, so the number of rows it returns is
    n_out; the rows as sets sorted by key; the six statistics of the call with rows and of the statistics-only call"""
    ok, ocl, ocr, ostats = oracle_join(left, right, kind)
    keys, cl, cr, st = la.join(ra, kind)
    assert st.as_tuple() == ostats, f"{what}: statistics"
    assert len(keys) == len(cl) == len(cr) == ostats[0], f"{what}: rows"
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(keys[order], ok), f"{what}: keys"
    assert np.array_equal(cl[order], ocl), f"{what}: count_left"
    assert np.array_equal(cr[order], ocr), f"{what}: count_right"
    _, _, _, only = la.join(ra, kind, want_rows=False)
    assert only.as_tuple() == ostats, f"{what}: statistics-only call"
    return ostats


def raw_join(pkg, ctx, la, ra, kind, cap, arrays, with_stats=True, on_device=0):
    """the C call itself: arrays = three numpy arrays / device pointers / None -> (status, n_out, stats)"""
    ptr = [None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a) for a in arrays]
    n, st = C.c_uint64(12345), pkg.JoinStats()
    rc = pkg.lib().dnagpu_acc_join(ctx.h if ctx else None, la.h if la else None, ra.h if ra else None, kind, ptr[0], ptr[1],
                                   ptr[2], cap, C.byref(n), C.byref(st) if with_stats else None, on_device)
    return rc, n.value, st.as_tuple()


@pytest.mark.gpu
def test_join_equal_geometry(ctx, accs, path):
    """two tables of 16 partitions each, 29,970 groups each, 20,370 shared: all three kinds in both role orders"""
    k = 31
    a, b = accs(SEED, 30_000, k), accs(SEED + 300, 30_000, k)
    oa, ob = oracle_counts(SEED, 30_000, k), oracle_counts(SEED + 300, 30_000, k)
    assert a.partitions == 16 and b.partitions == 16
    assert len(np.intersect1d(oa[0], ob[0])) == 20_370
    for kind in (0, 1, 2):
        check_join(a, b, oa, ob, kind, f"a x b kind {kind}")
        check_join(b, a, ob, oa, kind, f"b x a kind {kind}")


@pytest.mark.gpu
def test_join_right_finer_by_two_bits_and_the_reverse(ctx, accs, path):
    """16 partitions at mean load 0.75 (long probe chains, chains that wrap) against 64: s < t and s > t, every kind"""
    k = 31
    a, b = accs(SEED, 49_000, k), accs(SEED + 600, 150_000, k)
    oa, ob = oracle_counts(SEED, 49_000, k), oracle_counts(SEED + 600, 150_000, k)
    assert (len(oa[0]), len(ob[0])) == (48_970, 149_970)
    assert a.partitions == 16 and b.partitions == 64
    for kind in (0, 1, 2):
        sa = check_join(a, b, oa, ob, kind, f"16 x 64 kind {kind}")
        sb = check_join(b, a, ob, oa, kind, f"64 x 16 kind {kind}")
        if kind == 0:
            assert sa[0] == sb[0] == 29_770


@pytest.mark.gpu
def test_join_counts_above_one_and_unequal(ctx, accs, path):
    """k = 10: counts up to 7 and 8, left added twice so that min(count_left, count_right) depends on the comparison"""
    k = 10
    a, b = accs(SEED, 300_000, k, 2), accs(SEED + 3000, 1_000_000, k)
    oa1, ob = oracle_counts(SEED, 300_000, k), oracle_counts(SEED + 3000, 1_000_000, k)
    oa = oracle_counts(SEED, 300_000, k, 2)
    assert (len(oa[0]), len(ob[0])) == (260_984, 644_509)
    assert oracle_join(oa1, ob, 0)[3][0] == 225_454 and oracle_join(oa1, ob, 0)[3][3] == 253_414
    assert int(oa1[1].max()) >= 7 and int(ob[1].max()) >= 8
    for kind in (0, 1, 2):
        st = check_join(a, b, oa, ob, kind, f"k=10 kind {kind}")
        check_join(b, a, ob, oa, kind, f"k=10 reversed kind {kind}")
        if kind == 0:                            # sum_min is neither side's sum: some minima come from each side
            assert st[3] < st[1] and st[3] < st[2] and st[3] > 253_414


def text_acc(ctx, text, k):
    w, n = orc.dna_encode(text)
    d = ctx.upload(w, n)
    h = ctx.count_kmers(d, k)
    a = ctx.accumulator(k)
    a.add(h)
    h.free()
    d.free()
    ks, cs = orc.count_kmers(w, n, k)
    return a, (ks, cs.astype(np.uint64))


@pytest.mark.gpu
def test_join_tiny_and_empty(ctx, pkg, path):
    """poisoned, guarded pool; k = 32 with key 0 and the all-ones key on both sides, most partitions unoccupied; an empty left,
    an empty right (ANTI == left), left is right"""
    k = 32
    ctx.set_debug(path | pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL)
    a, oa = text_acc(ctx, "G" * 32 + "A" * 32 + "G", k)
    b, ob = text_acc(ctx, "A" * 32 + "C" + "G" * 32, k)
    empty = ctx.accumulator(k)
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    try:
        assert oa[0][0] == 0 and oa[0][-1] == ONES and ob[0][0] == 0 and ob[0][-1] == ONES
        assert empty.partitions == 0 and a.partitions == 16
        for kind in (0, 1, 2):
            st = check_join(a, b, oa, ob, kind, f"tiny kind {kind}")
            check_join(b, a, ob, oa, kind, f"tiny reversed kind {kind}")
            if kind == 0:
                assert st[0] >= 2
            assert check_join(empty, a, none, oa, kind, f"empty left kind {kind}")[0] == 0
            st = check_join(a, empty, oa, none, kind, f"empty right kind {kind}")
            assert st[0] == (0 if kind == 0 else len(oa[0])) and st[2] == 0
            st = check_join(a, a, oa, oa, kind, f"left is right kind {kind}")
            assert st[0] == (0 if kind == 1 else len(oa[0]))
            assert check_join(empty, empty, none, none, kind, f"both empty kind {kind}")[0] == 0
        ctx.synchronize()                        # (raises if a kernel wrote past the end of a work buffer)
    finally:
        for o in (a, b, empty):
            o.free()


@pytest.mark.gpu
def test_join_caps_null_arrays_and_device_outputs(ctx, pkg, accs, path):
    k = 31
    a, b = accs(SEED, 30_000, k), accs(SEED + 300, 30_000, k)
    oa, ob = oracle_counts(SEED, 30_000, k), oracle_counts(SEED + 300, 30_000, k)
    for kind in (0, 1):
        ok, ocl, ocr, ostats = oracle_join(oa, ob, kind)
        rows = ostats[0]
        want = {int(x): (int(y), int(z)) for x, y, z in zip(ok, ocl, ocr)}
        # cap = 0 with arrays: nothing stored, everything counted
        arrs = [np.full(8, SENTINEL) for _ in range(3)]
        assert raw_join(pkg, ctx, a, b, kind, 0, arrs) == (0, rows, ostats)
        assert all((x == SENTINEL).all() for x in arrs)
        # cap = rows - 1: all rows counted; the written rows are distinct, valid result rows
        arrs = [np.full(rows + 4, SENTINEL) for _ in range(3)]
        assert raw_join(pkg, ctx, a, b, kind, rows - 1, arrs) == (0, rows, ostats)
        gk = arrs[0][:rows - 1]
        assert len(np.unique(gk)) == rows - 1
        assert all(want[int(x)] == (int(y), int(z)) for x, y, z in zip(gk, arrs[1], arrs[2]))
        assert all((x[rows - 1:] == SENTINEL).all() for x in arrs)
        # cap > rows
        arrs = [np.full(rows + 4, SENTINEL) for _ in range(3)]
        assert raw_join(pkg, ctx, a, b, kind, rows + 1000, arrs) == (0, rows, ostats)
        order = np.argsort(arrs[0][:rows], kind="stable")
        assert np.array_equal(arrs[0][:rows][order], ok) and np.array_equal(arrs[1][:rows][order], ocl)
        assert np.array_equal(arrs[2][:rows][order], ocr)
        assert all((x[rows:] == SENTINEL).all() for x in arrs)
        # NULL subsets of the three arrays; stats NULL
        for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 0)):
            arrs = [np.full(rows, SENTINEL) if w else None for w in keep]
            assert raw_join(pkg, ctx, a, b, kind, rows, arrs, with_stats=any(keep)) == (0, rows, ostats if any(keep) else (0,) * 6)
            if keep[0]:
                assert np.array_equal(np.sort(arrs[0]), ok)
            if keep[1]:
                assert np.array_equal(np.sort(arrs[1]), np.sort(ocl))
            if keep[2]:
                assert np.array_equal(np.sort(arrs[2]), np.sort(ocr))
            if keep[0] and keep[2]:
                order = np.argsort(arrs[0], kind="stable")
                assert np.array_equal(arrs[2][order], ocr)
        # device outputs into caller buffers
        bufs = [ctx.buffer_alloc(8 * rows) for _ in range(3)]
        try:
            assert raw_join(pkg, ctx, a, b, kind, rows, bufs, on_device=1) == (0, rows, ostats)
            got = [ctx.download_u64(p, rows) for p in bufs]
            order = np.argsort(got[0], kind="stable")
            assert np.array_equal(got[0][order], ok) and np.array_equal(got[1][order], ocl) and np.array_equal(got[2][order], ocr)
            dk, dl, dr, st = a.join(b, kind, cap=rows, on_device=True, out=tuple(bufs))
            assert st.as_tuple() == ostats and (dk, dl, dr) == tuple(bufs)
        finally:
            for p in bufs:
                ctx.buffer_free(p)


@pytest.mark.gpu
def test_join_64_bit_counts(ctx, path):
    """poly-A (one group of 5 * 10^7 rows) added 100 times into left and 90 times into right beside a small random table on
    both sides: key 0's row carries both counts above 2^32, sum_min takes the 90-fold count, all sums exact"""
    k, n_a = 31, 50_000_000
    da = ctx.upload(np.zeros((n_a + 31) // 32, np.uint64), n_a)
    ha = ctx.count_kmers_unordered(da, k)
    da.free()
    assert ha.distinct == 1 and ha.total == n_a - k + 1
    sides = []
    for seed, times in ((SEED + 0x7000, 100), (SEED + 0x7000 + 50, 90)):
        d = ctx.synth(seed, 5_000)
        h = ctx.count_kmers_unordered(d, k)
        acc = ctx.accumulator(k)
        acc.add(h)
        for _ in range(times):
            acc.add(ha)
        h.free()
        d.free()
        ks, cs = oracle_counts(seed, 5_000, k)
        assert ks[0] != 0
        sides.append((acc, (np.concatenate([[np.uint64(0)], ks]),
                            np.concatenate([[np.uint64(times * (n_a - k + 1))], cs]))))
    ha.free()
    (a, oa), (b, ob) = sides
    try:
        for kind in (0, 1, 2):
            check_join(a, b, oa, ob, kind, f"64-bit kind {kind}")
            check_join(b, a, ob, oa, kind, f"64-bit reversed kind {kind}")
        keys, cl, cr, st = a.join(b, 0)
        at = int(np.flatnonzero(keys == 0)[0])
        assert int(cl[at]) == 100 * (n_a - k + 1) > 2 ** 32 and int(cr[at]) == 90 * (n_a - k + 1) > 2 ** 32
        shared = st.rows - 1
        assert shared == 5_000 - 32 * 50 - 30
        assert st.sum_min == 90 * (n_a - k + 1) + shared and st.sum_left == 100 * (n_a - k + 1) + shared
        assert st.sum_left <= a.total
    finally:
        a.free()
        b.free()


@pytest.mark.gpu
def test_join_leaves_its_sources_untouched_and_errors(ctx, pkg, accs, path):
    k = 31
    a, b = accs(SEED, 49_000, k), accs(SEED + 600, 150_000, k)
    before = [(x.summary(), x.distinct, x.total, x.partitions) + tuple(arr.tobytes() for arr in x.download()) for x in (a, b)]
    for kind in (0, 1, 2):
        a.join(b, kind)
        b.join(a, kind, cap=10)
        a.join(a, kind, want_rows=False)
    after = [(x.summary(), x.distinct, x.total, x.partitions) + tuple(arr.tobytes() for arr in x.download()) for x in (a, b)]
    assert before == after
    # k = 31 against k = 21: BAD_ARG, nothing written
    d = ctx.synth(SEED, 5_000)
    h21 = ctx.count_kmers_unordered(d, 21)
    c21 = ctx.accumulator(21)
    c21.add(h21)
    try:
        arrs = [np.full(64, SENTINEL) for _ in range(3)]
        for la, ra in ((a, c21), (c21, a)):
            rc, n, st = raw_join(pkg, ctx, la, ra, 0, 64, arrs)
            assert rc == BAD_ARG and n == 12345 and st == (0,) * 6
        assert all((x == SENTINEL).all() for x in arrs)
        # kind = 3: BAD_ARG before anything else is looked at, NULL objects included
        assert raw_join(pkg, ctx, a, b, 3, 64, arrs)[0] == BAD_ARG
        assert raw_join(pkg, None, None, None, 3, 0, [None] * 3)[0] == BAD_ARG
        assert raw_join(pkg, ctx, None, b, 0, 0, [None] * 3)[0] == BAD_ARG
        assert raw_join(pkg, ctx, a, None, 0, 0, [None] * 3)[0] == BAD_ARG
        assert raw_join(pkg, None, a, b, 0, 0, [None] * 3)[0] == BAD_ARG
        assert pkg.lib().dnagpu_acc_join(ctx.h, a.h, b.h, 0, None, None, None, 0, None, None, 0) == BAD_ARG
        assert all((x == SENTINEL).all() for x in arrs)
    finally:
        for o in (c21, h21, d):
            o.free()


@pytest.mark.gpu
def test_join_default_choice_small_against_large(ctx, accs):
    """no debug flag: 16 partitions against 512 and the reverse (the rule picks a path per order; the large left side is read
    out in two staged chunks) == the oracle"""
    k = 31
    a, b = accs(SEED, 30_000, k), accs(SEED + 300, 1_000_000, k)
    oa, ob = oracle_counts(SEED, 30_000, k), oracle_counts(SEED + 300, 1_000_000, k)
    assert a.partitions == 16 and b.partitions >= 256
    for kind in (0, 1, 2):
        st = check_join(a, b, oa, ob, kind, f"small x large kind {kind}")
        check_join(b, a, ob, oa, kind, f"large x small kind {kind}")
        if kind == 0:
            assert st[0] == 20_370


def _rows(seed, n_rows, lo, hi):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n_rows)
    text = orc.dna_decode(orc.synth_words(seed, int(lens.sum())), int(lens.sum()))
    cuts = np.concatenate([[0], np.cumsum(lens)])
    return [text[int(cuts[i]):int(cuts[i + 1])] for i in range(n_rows)]


def _oracle_table(rows, k):
    ks, cs = orc.count_keys(np.concatenate([orc.generate_kmers(*orc.dna_encode(r), k, faithful=False) for r in rows]))
    return ks, cs.astype(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 31])
def test_glue_join_of_two_aggregates(g, k):
    """two table aggregates counted in many batches, paired by the three kinds and served row by row == the oracle join; the
    stats call; the different-k error; both aggregates still serve their groups afterwards"""
    shared = _rows(0x10A1, 60, 40, 200)
    lrows = _rows(0x10A2, 80, 40, 200) + shared
    rrows = shared[:40] + _rows(0x10A3, 120, 40, 200)
    ol, orr = _oracle_table(lrows, k), _oracle_table(rrows, k)
    g.set_agg_flush_bases(2_000)
    try:
        with g.count_kmers_table_agg(k, lrows) as la, g.count_kmers_table_agg(k, rrows) as ra, \
                g.count_kmers_table_agg(k + 1, lrows[:3]) as other:
            for kind, code in (("i", 0), ("a", 1), ("l", 2)):
                for (x, ox), (y, oy) in (((la, ol), (ra, orr)), ((ra, orr), (la, ol))):
                    ok, ocl, ocr, ostats = oracle_join(ox, oy, code)
                    got, stats = g.count_kmers_join(x, y, kind)
                    assert stats == ostats[:4]
                    assert all(km.c.length == k for km, _, _ in got)
                    gk = np.array([km.c.bit_sequence for km, _, _ in got], dtype=np.uint64)
                    order = np.argsort(gk, kind="stable")
                    assert np.array_equal(gk[order], ok)
                    assert np.array_equal(np.array([c for _, c, _ in got], dtype=np.uint64)[order], ocl)
                    assert np.array_equal(np.array([c for _, _, c in got], dtype=np.uint64)[order], ocr)
            with pytest.raises(g.GlueError) as ei:
                g.count_kmers_join(la, other, "i")
            assert "different lengths" in str(ei.value)
            for x, ox in ((la, ol), (ra, orr)):
                got = x.groups()
                gk = np.array([km.c.bit_sequence for km, _ in got], dtype=np.uint64)
                order = np.argsort(gk, kind="stable")
                assert np.array_equal(gk[order], ox[0])
                assert np.array_equal(np.array([c for _, c in got], dtype=np.uint64)[order], ox[1])
    finally:
        g.set_agg_flush_bases(1 << 30)
