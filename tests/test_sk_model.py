"""The second half of tests/sk_model.py on its own: the host's rules of levels 1 and 2 give the values worked out by hand in
their docstrings, and crafted_stream() delivers what its spec asks for and keeps the engine's contract.  CPU only, but for
the last test, which ties the restated geometry to the engine (dnagpu_sk_buckets, and the d1 width of real records)."""
import numpy as np
import pytest

import sk_model as M

gpu = pytest.mark.gpu


def test_rules_spec_cap_and_span():
    assert M.spec_cap(8192, 2) == 4680 and M.spec_cap(40000, 4) == 11328 and M.spec_cap(60000, 512) == 208
    assert M.spec_cap(0, 512) == 72 and M.spec_cap(1, 2) == 72 and M.spec_cap(16, 2) == 88      # (0 + 79, 0 + 79, 9 + 79) & ~7
    assert M.spec_span(0, 9) == 0 and M.spec_span(60000, 9) == 208 * 512 and M.spec_span(8192, 1) == 9360
    for length in (1, 7, 4097, 65537, 1 << 31, 0xFFFFFFFF):
        for R in (2, 4, 512):
            cap = M.spec_cap(length, R)
            assert cap % 8 == 0 and cap >= 72 and cap * R >= length + length // 8 - R     # whole lines; the regions hold len + 12.5 %


def test_rules_chunk_len():
    assert M.chunk_len(0) == 32768 and M.chunk_len(1) == 32768 and M.chunk_len(32769) == 32768
    assert M.chunk_len(4096 * 32768) == 32768 and M.chunk_len(4096 * 32768 + 1) == 40960
    assert all(M.chunk_len(x) == 32768 for x in range(0, 134_217_729, 1_048_573))
    assert M.chunk_len(1 << 32) == (1 << 20) and M.chunk_len(10_000, 4096, 2016 * 4) == 4 * 8064


def test_rules_even():
    assert M.even([20946, 20000]) and not M.even([20947, 20000])
    assert M.even([]) and M.even([0, 0]) and M.even([70000, 0]) and M.even([0, 1])       # none, or one used bucket, are even
    assert M.even([1000, 1100, 1000]) and not M.even([1000, 1200, 1000])                  # 3300 <= 3354; 3600 > 3456
    assert M.even([20947, 20000], 1.03)                                                    # (the tolerance is what decides)


def test_rules_even_small_buckets_by_hand():
    """64 records of slack per used bucket: [100, 170] is 340 <= 1.02 * 270 + 128 = 403.4, even; [100, 400]: 800 > 638"""
    assert M.even([100, 170]) and not M.even([100, 400])


def test_rules_geometry_by_hand():
    want = {40_000: (1, 1), 160_000: (2, 1), 10_300_000: (9, 1), 21_000_000: (9, 2)}
    for rows, (b1, c0n) in want.items():
        g = M.geometry(rows, 31)
        assert (g.b1, g.c0n, g.r0bits, g.mid_limit, g.n_coarse, g.R) == (b1, c0n, 1, 1 << 27, 2, 1 << b1), (rows, g)
    g = M.geometry(40_000, 23, forced=True)
    assert (g.b1, g.c0n, g.mid_limit) == (1, 1, 60_003)
    g = M.geometry(4_000_000_000, 31)                 # 1.6 M final, 100 000 mid buckets, 196 coarse buckets of 512
    assert (g.b1, g.c0n, g.r0bits) == (9, 196, 8)
    assert M.geometry(1, 20).c0n == 1 and M.geometry(0xFFFFFFFF, 20).c0n <= M.SK_MAX_C0


def test_rules_received_cap_and_route():
    assert M.received_cap([8192, 0], 1) == 9360 and M.received_cap([0, 0], 9) == 0
    assert M.received_cap([20946, 20000], 9) == 512 * (M.spec_cap(20946, 512) + M.spec_cap(20000, 512)) == 512 * (120 + 120)
    assert M.received_cap([0xFFFFFFFF, 5], 9) == 0xFFFFFFFF + 5                           # (regions past 2^32: the records alone)
    assert M.route([20946, 20000], 0) == "Speculative" and M.route([20947, 20000], 0) == "Sampled"
    assert M.route([20946, 20000], M.DEBUG_NO_SPEC1) == "Exact" and M.route([20946, 20000], M.DEBUG_SAMPLE1) == "Sampled"
    assert M.route([0, 0], 0) == "Exact" and M.route([0, 30000], 0) == "Speculative"
    assert M.route([0xFFFFFFFF, 0], 0) == "Exact"
    assert M.heavy(60_004, 10, 60_003, True) and not M.heavy(60_003, 1 << 20, 60_003, True)
    assert M.heavy(5, 65_537, 1 << 27, False) and not M.heavy(1 << 27, 65_536, 1 << 27, False)


@pytest.mark.parametrize("k", [20, 23, 31, 32])
def test_encode_windows_is_encode(k):
    """the generator's vectorised encoder against encode(), every length, with and without NULL"""
    rng = np.random.default_rng(0xE2C + k)
    lm = M.lmax(k)
    codes = rng.integers(0, 4, (2 * lm, lm + k - 1), dtype=np.uint8)
    codes[-1] = 3
    length = np.concatenate([np.arange(1, lm + 1), np.arange(lm, 0, -1)])
    d1, d2 = rng.integers(0, 512, 2 * lm), rng.integers(0, 16, 2 * lm)
    lo, hi = M._pack_payload(codes)
    for null in (False, True):
        got = M.encode_windows(lo, hi, length, k, d1, d2, null=null).reshape(-1, 2)
        for i in range(2 * lm):
            want = M.encode(codes[i][:length[i] + k - 1], k, d1=int(d1[i]), d2=int(d2[i]), multi=True, null=null)
            assert (int(got[i, 0]), int(got[i, 1])) == want, (k, i)
    with pytest.raises(ValueError):
        M.encode_windows(lo[:1], hi[:1], [lm + 1], k, [0], [0])


def per_triple(records, bucket, k):
    """-> {(bucket, d1, d2): (records, k-mers)} of the non-NULL records"""
    d1, d2, length, null = M.record_fields(records)
    out = {}
    for b, a, c, n in zip(bucket[~null].tolist(), d1[~null].tolist(), d2[~null].tolist(), length[~null].tolist()):
        r, m = out.get((b, a, c), (0, 0))
        out[(b, a, c)] = (r + 1, m + n)
    return out


@pytest.mark.parametrize("order", ["shuffled", "digit", "tiles", "lanes", "runs64"])
@pytest.mark.parametrize("k", [20, 31, 32])
def test_crafted_stream_delivers_its_spec(k, order):
    rng = np.random.default_rng(0x57EA + k)
    lm = M.lmax(k)
    fixed = rng.integers(1, lm + 1, 700)
    groups = [(0, 0, 0, 9000, 2), (0, 0, 15, 1, lm), (0, 1, 3, 8192, (1, 3)), (0, 511, 7, 700, fixed), (1, 5, 5, 300, None),
              (1, 5, 6, 0, 1), (3, 0, 0, 5, 1)]
    nulls = {0: np.arange(0, 400, 3), 2: np.arange(10), 3: [5, 6]}
    recs, bucket, truth = M.crafted_stream(k, {"groups": groups, "copies": 4, "order": order, "nulls": nulls}, rng)
    n = len(recs) // 2
    d1, d2, length, null = M.record_fields(recs)
    assert len(bucket) == n and np.all(np.diff(bucket) >= 0)
    assert int(null.sum()) == 134 + 10 + 2 and n == sum(g[3] for g in groups) + 146
    got = per_triple(recs, bucket, k)
    want = {(0, 0, 0): (9000, 18000), (0, 0, 15): (1, lm), (0, 511, 7): (700, int(fixed.sum())), (3, 0, 0): (5, 5)}
    for key, val in want.items():
        assert got[key] == val, (key, got[key], val)
    assert got[(0, 1, 3)][0] == 8192 and 8192 <= got[(0, 1, 3)][1] <= 3 * 8192 and got[(1, 5, 5)][0] == 300
    assert set(got) == {(g[0], g[1], g[2]) for g in groups if g[3]}
    # NULL records where asked: bucket 0's first 400 slots, all of bucket 2, the last two of bucket 3
    at0 = np.flatnonzero(bucket == 0)
    assert np.array_equal(np.flatnonzero(null[at0]), np.arange(0, 400, 3))
    assert null[bucket == 2].all() and null[bucket == 3].tolist() == [False] * 5 + [True] * 2
    dec = M.decode(recs.reshape(-1, 2)[~null], k)
    assert np.array_equal(dec.kmers, truth) and dec.multi.all() and not M.payload_above(dec).any()
    assert len(truth) == sum(v[1] for v in got.values())
    assert len(np.unique(truth)) < len(truth)                                             # (copies: every read is used 4 times)
    M.check_contract(recs, bucket, k)
    # the order of bucket 0's real records
    live0 = at0[~null[at0]]
    if order == "digit":
        key = d1[live0] * 16 + d2[live0]
        assert np.all(np.diff(key) >= 0)
    elif order == "tiles":                            # 8192 of d1 = 0, 8192 of d1 = 1, 700 of d1 = 511, the other 809 of d1 = 0
        assert d1[live0].tolist() == [0] * 8192 + [1] * 8192 + [511] * 700 + [0] * 809
    elif order == "lanes":                            # d2 0, 3, 7, 15 in turn while all four last
        assert d2[live0][:8].tolist() == [0, 3, 7, 15, 0, 3, 7, 0]
    elif order == "runs64":
        assert d2[live0][:64 * 3 + 2].tolist() == [0] * 64 + [3] * 64 + [7] * 64 + [15, 0]
    else:
        assert np.any(np.diff(d1[live0]) < 0)


def test_crafted_stream_redraws_colliding_reads():
    """at k = 20 (4^20 = 1.1e12 values) 60 000 reads of 32 k-mers each collide across groups; the generator draws them again"""
    rng = np.random.default_rng(0xC011)
    groups = [(0, d1, d2, 120, 1) for d1 in range(512) for d2 in range(1)] + [(1, 0, 0, 1, 1)]
    recs, bucket, truth = M.crafted_stream(20, {"groups": groups, "copies": 1}, rng)
    assert M.crafted_stream.redrawn > 0
    M.check_contract(recs, bucket, 20)


def test_contract_check_rejects_a_planted_violation():
    rng = np.random.default_rng(0xBAD)
    k = 31
    recs, bucket, _ = M.crafted_stream(k, {"groups": [(0, 1, 2, 50, 3), (0, 1, 3, 50, 3), (1, 1, 2, 50, 3)], "copies": 1}, rng)
    M.check_contract(recs, bucket, k)
    w = recs.reshape(-1, 2).copy()
    planted = w.copy()
    planted[60] = w[10]                                # a record of (0, 1, 2) ...
    planted[60, 1] = (w[10, 1] & ~np.uint64(15 << M.D2_SHIFT)) | np.uint64(3 << M.D2_SHIFT)      # ... again under d2 = 3
    with pytest.raises(ValueError):
        M.check_contract(planted.reshape(-1), bucket, k)
    planted = w.copy()
    planted[120] = w[10]                               # the same record in another coarse bucket
    with pytest.raises(ValueError):
        M.check_contract(planted.reshape(-1), bucket, k)
    planted = w.copy()
    planted[60] = w[10]
    planted[60, 1] |= np.uint64(1 << 63)               # (a NULL record holds no k-mer)
    M.check_contract(planted.reshape(-1), bucket, k)
    planted = w.copy()
    planted[11] = w[10]                                # (a copy in its own final bucket is what the engine counts)
    M.check_contract(planted.reshape(-1), bucket, k)


@gpu
def test_geometry_is_the_engines():
    """c0n is dnagpu_sk_buckets over a spread of rows and k; b1 is the width of d1 in real records cut for that geometry;
    the debug flags the rules read are the binding's"""
    from __graft_entry__ import load_package
    from test_gpu_parity import pack_codes
    from test_sk_records import level0_records, random_codes
    pkg = load_package()
    for name in ("FORCE_SUPERKMER", "HEAVY_EXPAND", "NO_SPEC1", "SPEC1_OVERFLOW", "SAMPLE1"):
        assert getattr(M, "DEBUG_" + name) == getattr(pkg, "DEBUG_" + name)
    n = 30_000
    words = pack_codes(random_codes(n, 0x6E0))
    with pkg.Context(0) as ctx:
        for k in (20, 21, 22, 23, 27, 31, 32):
            for rows in (1, 40_000, 160_000, 600_000, 2_500_000, 10_300_000, 21_000_000, 50_000_000, 1_000_000_000,
                         4_000_000_000, 0xFFFFFFFF):
                assert ctx.sk_buckets(rows, k) == M.geometry(rows, k).c0n, (rows, k)
        widths = {}
        for k in (20, 31):
            count = n - k + 1
            for rows in (count, 40_000, 100_000, 160_000, 300_000, 600_000, 1_200_000, 2_500_000, 10_300_000, 21_000_000):
                recs, off = level0_records(ctx, words, n, k, 0, count, rows)
                g = M.geometry(rows, k)
                d1 = M.record_fields(recs)[0]
                assert len(off) == g.c0n + 1 and M.infer_b1(d1) == g.b1, (rows, k, g, M.infer_b1(d1))
                widths[g.b1] = widths.get(g.b1, 0) + 1
        assert set(widths) >= {1, 2, 3, 5, 9}, widths
