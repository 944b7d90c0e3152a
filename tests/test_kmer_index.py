"""The index over a stored kmer column (dnagpu_kmer_index_*): what the reference answers with CREATE INDEX ...
USING spgist (kmer_sequence spgist_kmer_ops) and index scans of `=`, `^@` and `@>` (dna--1.0.sql:304-314, test.sql:156-270).
The reference in every case is the CPU oracle: a column is orc.generate_kmers(words, n_bases, k) (what test.sql:172-176
stores), the expected rows are orc.generate_kmers_contains / _starts_with / _equals, whose positions are the row ids,
re-ordered on the host by (text order of the key under A < T < C < G, row).  Every comparison is integer and exact.
`visited` -- the index entries a query read -- must equal the rows whose first p bases lie in the filter's sets, p from the
prune rule computed here in numpy: a full scan dressed up as an index fails that."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import ROOT, load_package
from operator_model import IUPAC                  # letter -> 4-bit set of codes: the suite's one copy

T = 2048                                          # INDEX_SORT_TILE of csrc/kernels.hpp: keys per workgroup of the sort
MAX_RANGES = 1024                                 # DNAGPU_INDEX_MAX_RANGES
INVALID_K, LEN_MISMATCH, PREFIX_TOO_LONG, QKMER_INVALID, BAD_ARG, TOO_LARGE = 1, 2, 3, 4, 5, 6
SENTINEL = np.uint64(0xC3C3C3C3C3C3C3C3)
N_SCAN = 200_003


@pytest.fixture(scope="module")
def pkg():
    return load_package()


# ------------------------------------------------------------------ the host's own arithmetic (numpy)

def mask_of(k):
    return np.uint64((1 << (2 * k)) - 1 if k < 32 else 0xFFFFFFFFFFFFFFFF)


def rev2(x):
    """the 32 two-bit fields of every uint64 in reverse order"""
    x = np.asarray(x, dtype=np.uint64).copy()
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> np.uint64(sh)) & np.uint64(m)) | ((x & np.uint64(m)) << np.uint64(sh))
    return (x >> np.uint64(32)) | (x << np.uint64(32))


def r_of(keys, k):
    """ascending r = text order of the key under A < T < C < G (base 0 most significant)"""
    return rev2(np.asarray(keys, dtype=np.uint64) & mask_of(k)) >> np.uint64(64 - 2 * k)


def index_order(keys, k):
    """(rows, keys) of the whole index: the host's stable sort"""
    keys = np.asarray(keys, dtype=np.uint64) & mask_of(k)
    o = np.argsort(r_of(keys, k), kind="stable")
    return o.astype(np.uint64), keys[o]


def in_index_order(col, k, pos):
    """row ids `pos` (any order) -> (rows, keys) by (text order of the key, row)"""
    pos = np.asarray(pos, dtype=np.uint64)
    keys = col[pos.astype(np.int64)] & mask_of(k)
    o = np.lexsort((pos, r_of(keys, k)))
    return pos[o], keys[o]


def sets_of_pattern(pattern):
    return [IUPAC[c] for c in pattern]


def sets_of_prefix(k, length, bits):
    return [1 << ((bits >> (2 * i)) & 3) for i in range(length)] + [15] * (k - length)


def prune_depth(sets):
    prod, p = 1, 0
    while p < len(sets) and prod * bin(sets[p]).count("1") <= MAX_RANGES:
        prod *= bin(sets[p]).count("1")
        p += 1
    return p


def expected_visited(col, sets):
    """rows whose first p bases lie in the sets"""
    ok = np.ones(len(col), dtype=bool)
    for i in range(prune_depth(sets)):
        allowed = np.array([(sets[i] >> c) & 1 for c in range(4)], dtype=bool)
        ok &= allowed[((col >> np.uint64(2 * i)) & np.uint64(3)).astype(np.int64)]
    return int(ok.sum())


def column(seed, n, k, motif=0):
    nb = n + k - 1
    words = orc.synth_words_repeat(seed, nb, motif) if motif else orc.synth_words(seed, nb)
    col = orc.generate_kmers(words, nb, k, faithful=False)
    assert len(col) == n
    return words, nb, col


# ------------------------------------------------------------------ CPU: what needs no device

def test_index_math_on_the_host(tmp_path):
    """index_math.hpp (rev2, the order, the range of a prefix, the prune depth), host code of the header the kernels share,
    built with hipcc: no device is touched"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "index_math_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I",
                           os.path.join(ROOT, "dna-sequences-pg-extension_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "index_math_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_the_tests_order_is_text_order():
    """r_of above -- what every GPU test sorts by -- against the decoded text of the oracle, letters renamed so that
    A < T < C < G"""
    rng = np.random.default_rng(11)
    for k in (1, 5, 17, 31, 32):
        keys = rng.integers(0, 1 << 63, 300, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 300, dtype=np.uint64)
        keys[::3] &= np.uint64(0xFFFF)               # long shared prefixes of A's further up
        keys &= mask_of(k)
        text = [orc.kmer_decode(int(x), k).translate(str.maketrans("ATCG", "abcd")) for x in keys]
        by_text = sorted(range(len(keys)), key=lambda i: (text[i], i))
        assert np.array_equal(np.argsort(r_of(keys, k), kind="stable"), np.array(by_text)), k


def test_index_argument_rules_without_a_device(pkg):
    L = pkg.lib()
    out = C.c_void_p(0x1234)
    build = L.dnagpu_kmer_index_build
    for k in (0, 33, -1):                          # k comes first
        out.value = 0x1234
        assert build(None, None, 0, k, 0, C.byref(out)) == INVALID_K
        assert not out.value                       # *out = NULL whenever there is an out
    assert build(None, None, 0, 5, 0, C.byref(out)) == BAD_ARG
    assert build(None, None, 0, 5, 0, None) == BAD_ARG
    n_out = C.c_uint64(7)
    flt = pkg.Filter.contains("MRKYN")
    assert L.dnagpu_kmer_index_scan(None, None, C.byref(flt.c), None, None, 0, C.byref(n_out), None, 0) == BAD_ARG
    assert L.dnagpu_kmer_index_lookup(None, None, None, 0, None, None, 0) == BAD_ARG
    assert L.dnagpu_kmer_index_read(None, None, 0, 0, None, None, 0) == BAD_ARG
    assert L.dnagpu_kmer_index_rows(None) == 0 and L.dnagpu_kmer_index_distinct(None) == 0
    assert L.dnagpu_kmer_index_k(None) == 0
    L.dnagpu_kmer_index_free(None, None)
    assert pkg.abi_version() == 2
    assert hasattr(pkg, "KmerIndex") and hasattr(pkg.Context, "kmer_index")


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def check_whole_index(idx, col, k, what):
    rows, keys = idx.read()
    want_rows, want_keys = index_order(col, k)
    assert idx.rows == len(col) and idx.k == k, what
    assert np.array_equal(keys, want_keys), f"{what}: the keys are not in text order"
    assert np.array_equal(rows, want_rows), f"{what}: rows do not ascend inside equal keys / a row is missing"
    assert np.array_equal(np.sort(rows), np.arange(len(col), dtype=np.uint64)), f"{what}: not every row exactly once"
    assert idx.distinct == len(np.unique(col & mask_of(k))), f"{what}: distinct"


@pytest.mark.gpu
def test_golden_rows_of_the_reference(pkg, ctx):
    """the reference's own answers over single sequences, as index scans of the stored column"""
    def col_of(seq, k):
        w, n = orc.dna_encode(seq)
        return orc.generate_kmers(w, n, k)

    with ctx.kmer_index(col_of("ACGTACGCACGT", 6), 6) as idx:
        rows, keys, n_out, _ = idx.scan(pkg.Filter.contains("DNMSRN"))
        assert n_out == 2 and sorted(rows.tolist()) == [2, 6]
    with ctx.kmer_index(col_of("ACTGACGTACC", 3), 3) as idx:
        rows, _, n_out, visited = idx.scan(pkg.Filter.starts_with(*orc.kmer_encode("AC")))
        assert n_out == 3 == visited and sorted(rows.tolist()) == [0, 4, 8]
    with ctx.kmer_index(col_of("ACGTACGT", 6), 6) as idx:
        rows, keys, n_out, visited = idx.scan(pkg.Filter.equals(*orc.kmer_encode("ACGTAC")))
        assert n_out == 1 == visited and rows.tolist() == [0] and orc.kmer_decode(int(keys[0]), 6) == "ACGTAC"
    with ctx.kmer_index(col_of("ATCGATCGATCGATCGACG", 5), 5) as idx:
        assert idx.rows == 15 and idx.distinct == 6
        rows, keys = idx.read()
        assert [orc.kmer_decode(int(x), 5) for x in keys[[0, -1]]] == ["ATCGA", "GATCG"]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 4, 5, 16, 17, 31, 32])
def test_sort_shapes(ctx, k):
    """partial last digit, one full digit, two passes, 32 bits, 33 bits, eight passes; one key .. several tiles"""
    _, _, col = column(0x1D5000 + k, 200_003, k)
    for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 200_003):
        with ctx.kmer_index(col[:n], k) as idx:
            check_whole_index(idx, col[:n], k, f"k={k} n={n}")


@pytest.mark.gpu
def test_skewed_columns(ctx):
    rng = np.random.default_rng(5)
    n = 3 * T + 17
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    for k in (5, 17, 32):
        m = mask_of(k)
        rnd = rng.integers(0, 1 << 62, n, dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, n, dtype=np.uint64)
        _, in_order = index_order(rnd, k)
        top = np.uint64(2 * k - 2)                   # base 0 is the LOW field of a key and the TOP digit of r
        cases = {
            "all keys equal": np.full(n, rnd[0] & m, dtype=np.uint64),
            "two keys alternating": np.where(np.arange(n) % 2 == 0, rnd[0] & m, rnd[1] & m).astype(np.uint64),
            "already in index order": in_order,
            "in reverse index order": in_order[::-1].copy(),
            "all-ones key present": np.concatenate([rnd[:n - 3] & m, np.array([ones & m, np.uint64(0), ones & m])]),
            "differ only in the top digit of r": (rnd[0] & m & ~np.uint64(0xFF)) | (rnd & np.uint64(0xFF) & m),
            "differ only in the bottom digit of r": (rnd[0] & m & ~(np.uint64(3) << top)) | ((rnd & np.uint64(3)) << top),
        }
        for name, col in cases.items():
            with ctx.kmer_index(col, k) as idx:
                check_whole_index(idx, col, k, f"k={k} {name}")


def check_scan(pkg, ctx, idx, col, k, flt, pos, sets, what):
    """every output form of one scan against the oracle's row ids `pos`; sets = the filter's per-position sets, or None when
    nothing can match (visited = 0)"""
    want_rows, want_keys = in_index_order(col, k, pos)
    want_visited = expected_visited(col, sets) if sets is not None else 0
    rows, keys, n_out, visited = idx.scan(flt)
    assert n_out == len(pos), f"{what}: {n_out} rows, the oracle has {len(pos)}"
    assert visited == want_visited, f"{what}: visited {visited}, the pruned ranges hold {want_visited}"
    assert np.array_equal(rows, want_rows) and np.array_equal(keys, want_keys), f"{what}: rows / keys"
    # cap smaller than the matches: n_out is still the total, the first cap rows of index order are written
    cap = max(len(pos) // 2, 1)
    rows, keys, n_out, visited = idx.scan(flt, cap=cap)
    assert n_out == len(pos) and visited == want_visited, what
    assert np.array_equal(rows, want_rows[:cap]) and np.array_equal(keys, want_keys[:cap]), f"{what}: cap={cap}"
    # either output missing
    rows, keys, n_out, _ = idx.scan(flt, want_keys=False)
    assert keys is None and n_out == len(pos) and np.array_equal(rows, want_rows), f"{what}: rows only"
    rows, keys, n_out, _ = idx.scan(flt, want_rows=False)
    assert rows is None and n_out == len(pos) and np.array_equal(keys, want_keys), f"{what}: keys only"
    # device outputs, a sentinel word behind each
    m = len(pos)
    dr, dk = ctx.buffer_alloc(8 * (m + 1)), ctx.buffer_alloc(8 * (m + 1))
    for d in (dr, dk):
        ctx.upload_u64(d, np.full(m + 1, SENTINEL))
    n_out, visited = idx.scan(flt, cap=m, on_device=True, out=(dr, dk))
    gr, gk = ctx.download_u64(dr, m + 1), ctx.download_u64(dk, m + 1)
    ctx.buffer_free(dr)
    ctx.buffer_free(dk)
    assert n_out == m and visited == want_visited, what
    assert np.array_equal(gr[:m], want_rows) and np.array_equal(gk[:m], want_keys), f"{what}: device outputs"
    assert gr[m] == SENTINEL and gk[m] == SENTINEL, f"{what}: wrote past the matches"


@pytest.fixture(scope="module")
def scan_columns():
    """(words, n_bases, column) per (kind, k), computed once"""
    out = {}
    for kind, motif in (("synthetic", 0), ("repeat-rich", 1000)):
        for k in (5, 11, 32):
            out[kind, k] = column(0x5CA0 + k, N_SCAN, k, motif)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synthetic", "repeat-rich"])
@pytest.mark.parametrize("k", [5, 11, 32])
def test_scans(pkg, ctx, scan_columns, kind, k):
    words, nb, col = scan_columns[kind, k]
    rng = np.random.default_rng(k)
    with ctx.kmer_index(col, k) as idx:
        assert idx.rows == N_SCAN
        # `=`: a present key, an absent key, a key of another length
        present = int(col[N_SCAN // 3])
        col_set = set(col.tolist())
        absent = next(x for x in (int(v) & int(mask_of(k)) for v in rng.integers(0, 1 << 63, 4000, dtype=np.uint64) * 2 + 1)
                      if x not in col_set) if k > 5 else None
        for name, key in (("present", present), ("absent", absent)):
            if key is None:
                continue                             # (k = 5: all 1024 keys occur in 200 003 rows)
            _, pos = orc.generate_kmers_equals(words, nb, k, k, key)
            assert (len(pos) > 0) == (name == "present")
            check_scan(pkg, ctx, idx, col, k, pkg.Filter.equals(k, key), pos, sets_of_prefix(k, k, key), f"{kind} k={k} = {name}")
        other = k - 1 if k > 1 else k + 1
        rows, keys, n_out, visited = idx.scan(pkg.Filter.equals(other, present & int(mask_of(other))))
        assert (len(rows), n_out, visited) == (0, 0, 0), "= of another length"
        # `^@`: prefixes of 1, k - 1 and k bases (k = 32: the 32-base prefix compares all 64 bits)
        for plen in (1, k - 1, k):
            pbits = present & int(mask_of(plen))
            _, pos = orc.generate_kmers_starts_with(words, nb, k, plen, pbits)
            assert len(pos) > 0
            check_scan(pkg, ctx, idx, col, k, pkg.Filter.starts_with(plen, pbits), pos, sets_of_prefix(k, plen, pbits),
                       f"{kind} k={k} ^@ {plen} bases")
            _, _, n_out, visited = idx.scan(pkg.Filter.starts_with(plen, pbits), cap=0)
            assert visited == n_out == len(pos), "^@ visits its matches only"
        # `@>`: MRKYN-like, all N, leading N, with U
        tail = "MRKYNWSBDHVACGTNNMRKYNWSBDHVACGT"
        patterns = [("MRKYN" + tail)[:k], "N" * k, ("NNNNNNNNNNWSNNNNNNNNN" + tail)[:k] if k > 5 else "NNWSN",
                    ("NMRKY" + tail)[:k], ("WSWSWSWSWSWS" + "N" * 32)[:k]]
        for pattern in patterns:
            _, pos = orc.generate_kmers_contains(words, nb, k, pattern)
            check_scan(pkg, ctx, idx, col, k, pkg.Filter.contains(pattern), pos, sets_of_pattern(pattern),
                       f"{kind} k={k} {pattern} @>")
        _, _, n_out, visited = idx.scan(pkg.Filter.contains("N" * k), cap=0)
        assert n_out == visited == N_SCAN, "the all-N pattern visits every row"
        with_u = ("MRUYN" + tail)[:k]
        _, pos = orc.generate_kmers_contains(words, nb, k, with_u)
        assert len(pos) == 0
        check_scan(pkg, ctx, idx, col, k, pkg.Filter.contains(with_u), pos, None, f"{kind} k={k} {with_u} @>")


@pytest.mark.gpu
def test_lookup(pkg, ctx):
    k = 11
    _, _, col = column(0x100C, N_SCAN, k)
    uniq = np.unique(col)
    rng = np.random.default_rng(3)
    absent_pool = np.setdiff1d(rng.integers(0, 1 << (2 * k), 40_000, dtype=np.uint64), uniq)
    want_rows, want_keys = index_order(col, k)
    want_r = r_of(want_keys, k)
    with ctx.kmer_index(col, k) as idx:
        for m in (1, 64, 10_007):
            q = np.empty(m, dtype=np.uint64)
            q[0::2] = rng.choice(uniq, size=len(q[0::2]))
            q[1::2] = rng.choice(absent_pool, size=len(q[1::2]))
            if m > 8:
                q[4] = q[0] | np.uint64(1 << (2 * k))        # bits above 2k: matches nothing
                q[6] = q[2] | np.uint64(1 << 63)
            valid = (q >> np.uint64(2 * k)) == 0
            lo = np.searchsorted(want_r, r_of(q, k), side="left")
            hi = np.searchsorted(want_r, r_of(q, k), side="right")
            want_count = np.where(valid, hi - lo, 0).astype(np.uint64)
            first, count = idx.lookup(q)
            assert np.array_equal(count, want_count), m
            hit = want_count > 0
            assert np.array_equal(first[hit], lo[hit].astype(np.uint64)), m
            assert hit[0] and (m == 1 or not hit[1])
            # the device form
            dq, df, dc = (ctx.buffer_alloc(8 * m) for _ in range(3))
            ctx.upload_u64(dq, q)
            idx.lookup_device(dq, m, df, dc)
            gf, gc = ctx.download_u64(df, m), ctx.download_u64(dc, m)
            assert np.array_equal(ctx.download_u64(dq, m), q)
            for d in (dq, df, dc):
                ctx.buffer_free(d)
            assert np.array_equal(gc, want_count) and np.array_equal(gf[hit], first[hit]), m
            # read(first, count) of a window = the key's rows, ascending
            for j in np.flatnonzero(hit)[:20]:
                rows, keys = idx.read(int(first[j]), int(count[j]))
                assert np.all(keys == q[j])
                assert np.array_equal(rows, np.flatnonzero(col == q[j]).astype(np.uint64))


@pytest.mark.gpu
def test_errors_and_edges(pkg, ctx):
    L = pkg.lib()
    # n = 0: a valid index that holds no device memory; every scan returns 0 rows, operator errors are not raised
    before = ctx.device_bytes()
    with ctx.kmer_index(np.empty(0, dtype=np.uint64), 5) as idx:
        assert (idx.rows, idx.distinct, idx.k) == (0, 0, 5) and ctx.device_bytes() == before
        for flt in (pkg.Filter.contains("MRKYN"), pkg.Filter.contains("MRKY"), pkg.Filter.starts_with(6, 0),
                    pkg.Filter.equals(5, 0)):
            rows, keys, n_out, visited = idx.scan(flt)
            assert (len(rows), len(keys), n_out, visited) == (0, 0, 0, 0)
        with pytest.raises(pkg.DnaGpuError) as ei:            # a malformed filter is always an error
            idx.scan(pkg.Filter.contains("MRXYN"))
        assert ei.value.code == QKMER_INVALID
        first, count = idx.lookup(np.array([0, 5], dtype=np.uint64))
        assert count.tolist() == [0, 0]
        rows, keys = idx.read()
        assert len(rows) == 0 == len(keys)
    # k, NULL arguments, n over the limit (refused before any device work: the pointer is never touched)
    out = C.c_void_p()
    for k in (0, 33):
        assert L.dnagpu_kmer_index_build(ctx.h, None, 0, k, 0, C.byref(out)) == INVALID_K
        with pytest.raises(pkg.DnaGpuError) as ei:
            ctx.kmer_index(np.zeros(4, dtype=np.uint64), k)
        assert ei.value.code == INVALID_K
    assert L.dnagpu_kmer_index_build(ctx.h, None, 3, 5, 0, C.byref(out)) == BAD_ARG
    assert L.dnagpu_kmer_index_build(ctx.h, None, 0, 5, 0, None) == BAD_ARG
    small = ctx.buffer_alloc(64)
    bytes_before = ctx.device_bytes()
    out.value = 0x1234
    assert L.dnagpu_kmer_index_build(ctx.h, small, 1 << 32, 5, 1, C.byref(out)) == TOO_LARGE
    assert not out.value and ctx.device_bytes() == bytes_before
    ctx.buffer_free(small)
    _, _, col = column(0xE44, 3 * T + 17, 5)
    with ctx.kmer_index(col, 5) as idx:
        n_out = C.c_uint64()
        flt = pkg.Filter.contains("MRKYN")
        assert L.dnagpu_kmer_index_scan(ctx.h, idx.h, None, None, None, 0, C.byref(n_out), None, 0) == BAD_ARG
        assert L.dnagpu_kmer_index_scan(ctx.h, idx.h, C.byref(flt.c), None, None, 0, None, None, 0) == BAD_ARG
        assert L.dnagpu_kmer_index_scan(ctx.h, None, C.byref(flt.c), None, None, 0, C.byref(n_out), None, 0) == BAD_ARG
        # the two operator errors, raised only on a non-empty index
        for flt, code in ((pkg.Filter.contains("MRKY"), LEN_MISMATCH), (pkg.Filter.contains("MRKYNN"), LEN_MISMATCH),
                          (pkg.Filter.starts_with(6, 0), PREFIX_TOO_LONG), (pkg.Filter.contains(""), QKMER_INVALID),
                          (pkg.Filter(9), BAD_ARG)):
            with pytest.raises(pkg.DnaGpuError) as ei:
                idx.scan(flt)
            assert ei.value.code == code
        # visited may be NULL
        assert L.dnagpu_kmer_index_scan(ctx.h, idx.h, C.byref(pkg.Filter.contains("NNNNN").c), None, None, 0, C.byref(n_out),
                                        None, 0) == 0 and n_out.value == len(col)
        # the window rule of read
        n = idx.rows
        for first, count, ok in ((0, n, True), (n, 0, True), (n - 1, 1, True), (n + 1, 0, False), (n, 1, False), (1, n, False),
                                 (0, 0, True)):
            if ok:
                rows, keys = idx.read(first, count)
                assert len(rows) == count
            else:
                with pytest.raises(pkg.DnaGpuError) as ei:
                    idx.read(first, count)
                assert ei.value.code == BAD_ARG
        want_rows, want_keys = index_order(col, 5)
        rows, keys = idx.read(100, 1000)
        assert np.array_equal(rows, want_rows[100:1100]) and np.array_equal(keys, want_keys[100:1100])
        rows, keys = idx.read(100, 1000, want_keys=False)
        assert keys is None and np.array_equal(rows, want_rows[100:1100])
        dr = ctx.buffer_alloc(8 * 1000)
        idx.read_device(100, 1000, dr, None)
        assert np.array_equal(ctx.download_u64(dr, 1000), want_rows[100:1100])
        ctx.buffer_free(dr)
    # the caller's device key array is bit-identical after a build; bits above 2k are masked off
    dirty = col | (np.uint64(0xABC) << np.uint64(10))
    dk = ctx.buffer_alloc(8 * len(dirty))
    ctx.upload_u64(dk, dirty)
    with ctx.kmer_index_device(dk, len(dirty), 5) as idx:
        assert np.array_equal(ctx.download_u64(dk, len(dirty)), dirty)
        check_whole_index(idx, col, 5, "device keys with stray bits")
    ctx.buffer_free(dk)


@pytest.mark.gpu
def test_poisoned_and_guarded_pool(pkg):
    k = 11
    words, nb, col = column(0x9015, 3 * T + 17, k)
    pattern = "MRKYNNNWSNN"
    _, pos = orc.generate_kmers_contains(words, nb, k, pattern)
    with pkg.Context(0) as c:
        c.set_debug(pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL)
        idx = c.kmer_index(col, k)
        check_whole_index(idx, col, k, "poisoned pool")
        check_scan(pkg, c, idx, col, k, pkg.Filter.contains(pattern), pos, sets_of_pattern(pattern), "poisoned pool")
        first, count = idx.lookup(col[:100])
        want_r = r_of(index_order(col, k)[1], k)
        assert np.array_equal(first, np.searchsorted(want_r, r_of(col[:100], k), side="left").astype(np.uint64))
        assert np.array_equal(count, (np.searchsorted(want_r, r_of(col[:100], k), side="right") - first.astype(np.int64)).astype(np.uint64))
        assert pkg.lib().dnagpu_synchronize(c.h) == 0          # every guard band intact
        idx.free()
        assert pkg.lib().dnagpu_synchronize(c.h) == 0


@pytest.mark.gpu
def test_sort_and_scan_edges_in_a_guarded_pool(pkg):
    """The sort at its edges -- one key, T and T + 1 keys, T + 1 equal keys (every digit takes one value: only the last pass
    moves anything), at k = 1, 12 and 32 -- and a scan that tests the positions behind its ranges, over two tiles of
    candidates: cap 0 and around the total, rows only and keys only, into host arrays and into device buffers of exactly
    min(total, cap) entries"""
    with pkg.Context(0) as c:
        c.set_debug(pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL)
        for k in (1, 12, 32):
            _, _, col = column(0x50E7 + k, T + 1, k)
            for name, keys in (("one key", col[:1]), ("T keys", col[:T]), ("T + 1 keys", col),
                               ("T + 1 equal keys", np.full(T + 1, col[5], dtype=np.uint64))):
                with c.kmer_index(keys, k) as idx:
                    check_whole_index(idx, keys, k, f"guarded pool, k={k}, {name}")
        k, pattern = 11, "NNNNNNNNNWS"
        words, nb, col = column(0x9017, T + 1, k)
        _, pos = orc.generate_kmers_contains(words, nb, k, pattern)
        want = in_index_order(col, k, pos)
        total = len(pos)
        assert 2 < total < T + 1 == expected_visited(col, sets_of_pattern(pattern))
        flt = pkg.Filter.contains(pattern)
        with c.kmer_index(col, k) as idx:
            for cap in (0, total - 1, total, total + 1):
                m = min(cap, total)
                for wants in ((True, True), (True, False), (False, True), (False, False)):
                    got = idx.scan(flt, cap=cap, want_rows=wants[0], want_keys=wants[1])
                    assert got[2:] == (total, T + 1), f"cap={cap} {wants}"
                    dev = [c.buffer_alloc(8 * m) if w and m else None for w in wants]
                    assert idx.scan(flt, cap=cap, on_device=True, out=tuple(dev)) == (total, T + 1), f"cap={cap} {wants}: device"
                    for host, p, e, w in zip(got[:2], dev, want, wants):
                        assert (host is None) if not w else np.array_equal(host, e[:m]), f"cap={cap} {wants}"
                        if p is not None:
                            assert np.array_equal(c.download_u64(p, m), e[:m]), f"cap={cap} {wants}: device"
                            c.buffer_free(p)
        assert pkg.lib().dnagpu_synchronize(c.h) == 0              # every guard band intact


@pytest.mark.gpu
def test_free_and_trim_give_the_memory_back(pkg):
    _, _, col = column(0xF4EE, 200_003, 17)
    with pkg.Context(0) as c:
        c.trim()
        before = c.device_bytes()
        idx = c.kmer_index(col, 17)
        rows, keys, n_out, _ = idx.scan(pkg.Filter.starts_with(3, 0b100111))
        assert n_out > 0 and c.device_bytes() >= before + 12 * len(col)
        idx.free()
        c.trim()
        assert c.device_bytes() == before


# ------------------------------------------------------------------ the glue (glue/dna_glue.h: kmer_index_*)

@pytest.fixture(scope="module")
def g(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".glue")


def test_glue_refuses_a_column_of_mixed_lengths(g):
    """an index covers one k (a divergence); refused before anything goes to a device"""
    with pytest.raises(g.GlueError) as ei:
        g.kmer_index([g.kmer("ACGTA"), g.kmer("ACGTC"), g.kmer("ACGT")])
    assert str(ei.value) == "kmer_index_create: the column holds kmers of 5 and 4 bases; an index covers one length"


@pytest.mark.gpu
def test_glue_index_scans_equal_a_seq_scan(g):
    """test.sql:172-262 in small: the column is generate_kmers(sequence, 5), the three operators as index scans return the
    row ids, ascending, of a sequential scan with the glue's own per-datum operators"""
    k, n = 5, 10_007
    nb = n + k - 1
    text = orc.dna_decode(orc.synth_words(0x61CE, nb), nb)
    col = g.generate_kmers(text, k)
    assert len(col) == n
    with g.kmer_index(col) as idx:
        assert len(idx) == n
        for q in ("ATCGC", "GGGGG", "ATCG"):                   # test.sql:188-208; a key of another length matches nothing
            rhs = g.kmer(q)
            assert idx.scan("=", rhs) == [i for i, x in enumerate(col) if x == rhs], q
        for q in ("ACTG", "A", "ACTGA"):                       # test.sql:219-237
            rhs = g.kmer(q)
            want = [i for i, x in enumerate(col) if g.starts_with(x, rhs)]
            assert want and idx.scan("^@", rhs) == want, q
        for q in ("MRKYN", "NNNNN", "NANNN", "ATCGU"):         # test.sql:248-262
            rhs = g.qkmer(q)
            want = [i for i, x in enumerate(col) if g.contains(rhs, x)]
            assert (q == "ATCGU") == (not want) and idx.scan("@>", rhs) == want, q
        # the reference's ERROR texts, unchanged
        with pytest.raises(g.GlueError) as ei:
            idx.scan("@>", g.qkmer("MRKY"))
        assert str(ei.value) == "Qkmer pattern and kmer lengths do not match"
        with pytest.raises(g.GlueError) as ei:
            idx.scan("^@", g.kmer("ACTGAC"))
        assert str(ei.value) == "Prefix length cannot exceed kmer length"
    with g.kmer_index([]) as idx:                              # an empty column: no rows, and no operator ERROR
        assert len(idx) == 0 and idx.scan("=", g.kmer("ATCGC")) == [] and idx.scan("@>", g.qkmer("MRKY")) == []
