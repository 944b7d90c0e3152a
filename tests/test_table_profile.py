"""The k-mer profile of every sequence of a table (dnagpu_table_profile) with the glue's table_profile on top.
CPU tests: the argument rules that need no device, the numpy reference on a hand-worked sequence, the glue's texts for a bad k,
profile_math.hpp as a host program (plain and with sanitizers).  GPU tests: numpy over the oracle is the reference -- the rows
of the table (orc.generate_kmers_table), np.bincount(seq * W + key) -- and every comparison is equality.  Every GPU test
runs twice: plainly, and with DNAGPU_DEBUG_POISON_POOL | DNAGPU_DEBUG_GUARD_POOL."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import ROOT, load_package
from test_table_hits import canonical_np, encode_table, rc_np, resident, revcomp_text

INVALID_K, BAD_ARG, TOO_LARGE = 1, 5, 6
SEED = 0x4B1 << 32
SENTINEL32 = 0xC3C3C3C3
KS = [1, 2, 3, 4, 5, 6]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


# ------------------------------------------------------------------ the numpy reference

_REF = {}


def ref_profile(texts, k, canonical=False):
    """(counts uint32[n, 4^k], rows uint64[n]); computed once per table, never modified"""
    key = (tuple(texts), k, canonical)
    if key not in _REF:
        n, width = len(texts), 4 ** k
        words, starts = encode_table(texts)
        lens = np.diff(starts).astype(np.int64)
        rows = np.where(lens >= k, lens - k + 1, 0).astype(np.uint64)
        keys = orc.generate_kmers_table(words, starts, k) if int(starts[-1]) else np.zeros(0, dtype=np.uint64)
        assert len(keys) == int(rows.sum())
        if canonical:
            keys = canonical_np(keys, k)
        seq_of = np.repeat(np.arange(n, dtype=np.int64), rows.astype(np.int64))
        counts = np.bincount(seq_of * width + keys.astype(np.int64), minlength=n * width).reshape(n, width).astype(np.uint32)
        counts.setflags(write=False)
        rows.setflags(write=False)
        _REF[key] = (counts, rows)
    return _REF[key]


def fold_np(fwd, k):
    """canon[c] = fwd[c] + fwd[rc(c)] when c != rc(c), fwd[c] when c == rc(c), 0 where c is not canonical"""
    cols = np.arange(4 ** k, dtype=np.uint64)
    rc = rc_np(cols, k).astype(np.int64)
    is_canon = canonical_np(cols, k) == cols
    out = fwd.astype(np.uint64) + np.where(rc == cols.astype(np.int64), 0, fwd[:, rc].astype(np.uint64))
    out[:, ~is_canon] = 0
    return out.astype(np.uint32)


def random_texts(lengths, seed):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list("ATCG"), n)) if n else "" for n in lengths]


# ------------------------------------------------------------------ CPU: what needs no device

def test_profile_argument_rules_without_a_device(pkg):
    """the test that shows the feature: the three symbols are absent before it"""
    L = pkg.lib()
    assert [pkg.profile_width(k) for k in range(1, 7)] == [4, 16, 64, 256, 1024, 4096]
    for k in (0, 7, 32, 33, -1):
        assert pkg.profile_width(k) == 0
    out = (C.c_uint32 * 4)(*([SENTINEL32] * 4))
    rows = (C.c_uint64 * 1)(77)
    for flags in (0, 1, 2, 3, 0xFFFFFFFF):
        for k in (0, 1, 4, 7, 33):
            assert L.dnagpu_table_profile(None, None, k, flags, 0, 1, out, rows, 0) == BAD_ARG
    assert list(out) == [SENTINEL32] * 4 and rows[0] == 77
    wave_rows, tile_rows = pkg.profile_geometry()
    assert 0 < wave_rows < tile_rows and tile_rows % 32 == 0
    assert L.dnagpu_profile_geometry(None, None) == 0
    assert pkg.PROFILE_CANONICAL == 1 and pkg.PROFILE_MAX_K == 6 and pkg.abi_version() == 2
    assert hasattr(pkg.Context, "table_profile")


def test_the_tests_reference_on_a_hand_worked_sequence():
    """a guard on ref_profile itself: test.sql:95's sequence at k = 5 -- ATCGA 4, CGATC / GATCG / TCGAT 3, TCGAC / CGACG 1 and
    zeros elsewhere; beside it a row too short for a 5-mer and an empty one.  It runs no code of the project."""
    counts, rows = ref_profile(["ATCGATCGATCGATCGACG", "ATCG", ""], 5)
    assert rows.tolist() == [15, 0, 0] and counts.shape == (3, 1024)
    got = {orc.kmer_decode(np.uint64(c), 5): int(counts[0, c]) for c in np.flatnonzero(counts[0])}
    assert got == {"ATCGA": 4, "CGATC": 3, "GATCG": 3, "TCGAT": 3, "TCGAC": 1, "CGACG": 1}
    assert not counts[1:].any()
    # the fold: rc(ATCGA) = TCGAT, rc(CGATC) = GATCG, rc(TCGAC) = GTCGA, rc(CGACG) = CGTCG
    canon = ref_profile(["ATCGATCGATCGATCGACG", "ATCG", ""], 5, canonical=True)[0]
    got = {orc.kmer_decode(np.uint64(c), 5): int(canon[0, c]) for c in np.flatnonzero(canon[0])}
    assert got == {"ATCGA": 7, "CGATC": 6, "TCGAC": 1, "CGACG": 1}
    assert np.array_equal(fold_np(counts, 5), canon)


def test_glue_table_profile_refuses_a_bad_k(g, pkg):
    for k in (0, 33, -1):
        with pytest.raises(g.GlueError) as ei:
            g.table_profile(["ATCG"], k)
        assert str(ei.value) == pkg.strerror(INVALID_K)
    for k in (7, 32):
        with pytest.raises(g.GlueError) as ei:
            g.table_profile(["ATCG"], k)
        assert "table_profile" in str(ei.value) and "k <= 6" in str(ei.value)


SANITIZERS = ["-g", "-Xarch_host", "-fsanitize=address,undefined"]


@pytest.mark.parametrize("extra", [[], SANITIZERS], ids=["plain", "sanitizers"])
def test_profile_math_on_the_host(tmp_path, extra):
    """profile_math.hpp, host code of the header the kernels share, as a stand-alone program (the second build with
    AddressSanitizer and UndefinedBehaviorSanitizer on it) against naive loops: rows, class and items around both limits,
    item -> (sequence, tile, rows) covering every row once, and rc / canonical / fold target of every key at k = 1..6"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "profile_math_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", *extra, "-I",
                           os.path.join(ROOT, "dna-sequences-pg-extension_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "profile_math_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["plain", "poison"])
def dbg(request, ctx, pkg):
    """every GPU test once as it is and once with poisoned, guarded pool buffers; the guard bands are checked afterwards"""
    ctx.set_debug(pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL if request.param == "poison" else 0)
    yield request.param
    assert pkg.lib().dnagpu_synchronize(ctx.h) == 0
    ctx.set_debug(0)


def check_profile(ctx, dna, texts, k, what, canonical=False):
    counts, rows = ref_profile(texts, k, canonical)
    gc, gr = ctx.table_profile(dna, k, canonical=canonical)
    assert gc.shape == counts.shape and gc.dtype == np.uint32
    assert np.array_equal(gr, rows), f"{what}: rows"
    bad = np.flatnonzero((gc != counts).any(axis=1))
    assert not len(bad), f"{what}: sequences {bad[:5]} of lengths {[len(texts[i]) for i in bad[:5]]}"
    assert np.array_equal(gc.sum(axis=1, dtype=np.uint64), rows), f"{what}: row sums"
    return gc


def device_profile(ctx, dna, k, n, width, canonical=False, seq_first=0, pad=0, want_rows=True):
    """the same into device memory: `pad` sentinel cells either side of the matrix -> (before, counts[n, width], after, rows)"""
    cells = n * width
    buf = ctx.buffer_alloc(4 * (cells + 2 * pad) + 8)
    rbuf = ctx.buffer_alloc(8 * max(n, 1))
    try:
        ctx.upload_bytes(buf, np.full(cells + 2 * pad, SENTINEL32, dtype=np.uint32).view(np.uint8))
        ctx.table_profile(dna, k, canonical=canonical, seq_first=seq_first, seq_count=n, out_counts_dev=buf + 4 * pad,
                          out_rows_dev=rbuf if want_rows else None)
        got = ctx.download_bytes(buf, 4 * (cells + 2 * pad)).view(np.uint32)
        rows = ctx.download_u64(rbuf, n) if want_rows else None
    finally:
        ctx.buffer_free(buf)
        ctx.buffer_free(rbuf)
    return got[:pad], got[pad:pad + cells].reshape(n, width), got[pad + cells:], rows


def edge_lengths(pkg, k):
    wave_rows, tile_rows = pkg.profile_geometry()
    wave_len, tile_len = wave_rows + k - 1, tile_rows + k - 1
    return [k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, wave_len - 1, wave_len, wave_len + 1, tile_len - 1, tile_len,
            tile_len + 1, 2 * tile_rows + k - 1, 2 * tile_rows + k, 0, 0, 0, 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_profile_at_every_length_edge(ctx, pkg, dbg, k):
    """lengths around k, the 32-base word and the 64-base read, one either side of both class limits and of two full items,
    with empty sequences and runs of them, shuffled behind a first sequence of 7 bases: every later one starts mid-word.
    Forward and canonical; the canonical result is also numpy's fold of the forward one."""
    lengths = edge_lengths(pkg, k)
    order = np.random.default_rng(SEED + k).permutation(len(lengths))
    texts = random_texts([7] + [lengths[i] for i in order], SEED + 10 + k)
    d = resident(ctx, texts)
    try:
        fwd = check_profile(ctx, d, texts, k, "forward")
        canon = check_profile(ctx, d, texts, k, "canonical", canonical=True)
        assert np.array_equal(canon, fold_np(fwd, k))
    finally:
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_profile_mixed_classes_in_one_call(ctx, pkg, dbg, k):
    """one sequence of 70,000 bases (several items, the atomic path) between 2,000 sequences of exactly k bases and some
    empty ones, and one of three items and a bit at the end: the shared rows are exact and so are their neighbours, so the
    zeroing touched those rows only"""
    tile_rows = pkg.profile_geometry()[1]
    assert 70_000 - k + 1 > tile_rows
    lengths = [k] * 1000 + [0, 0, 70_000, 0] + [k] * 1000 + [0, 3 * tile_rows + 5 + k - 1]
    texts = random_texts(lengths, SEED + 20 + k)
    d = resident(ctx, texts)
    try:
        check_profile(ctx, d, texts, k, "forward")
        check_profile(ctx, d, texts, k, "canonical", canonical=True)
    finally:
        d.free()


@pytest.mark.gpu
def test_profile_contention_and_width(ctx, dbg):
    """every row in one counter: runs of A of 20,000 and of 70,000 bases (a count above 65,535) at k = 1, 2, 3; a
    dinucleotide microsatellite of 20,000 bases at k = 2 and 6"""
    texts = ["A" * 20_000, "A" * 70_000, "AC" * 10_000, "A" * 100]
    d = resident(ctx, texts)
    try:
        for k in (1, 2, 3):
            got = check_profile(ctx, d, texts, k, f"k = {k}")
            assert got[0, 0] == 20_000 - k + 1 and got[1, 0] == 70_000 - k + 1 > 65_535 and got[3, 0] == 100 - k + 1
            check_profile(ctx, d, texts, k, f"k = {k}, canonical", canonical=True)
        for k in (2, 6):
            got = check_profile(ctx, d, texts, k, f"k = {k}")
            assert sorted(got[2][got[2] != 0].tolist()) == sorted([(20_000 - k + 1) // 2, (20_000 - k + 2) // 2])
            check_profile(ctx, d, texts, k, f"k = {k}, canonical", canonical=True)
    finally:
        d.free()


WINDOW_LENGTHS = [5, 0, 0, 0, 33, 100, 9000, 64, 1, 0, 2500, 17, 100, 100, 31, 0, 0, 63, 140_000, 6, 2049, 12]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 5])
def test_profile_windows(ctx, pkg, dbg, k):
    """windows that tile the table, concatenated, equal the whole; an odd seq_first; a window of empty sequences only;
    seq_count = 0; the two bad windows; device output into a larger sentinel buffer (also at an address that is only 4-byte
    aligned) leaves the cells either side alone; out_rows = NULL; host and device output are equal"""
    texts = random_texts(WINDOW_LENGTHS, SEED + 30)
    n, width = len(texts), 4 ** k
    counts, rows = ref_profile(texts, k)
    d = resident(ctx, texts)
    try:
        cuts = [0, 1, 4, 7, 8, 19, n]
        parts = [ctx.table_profile(d, k, seq_first=a, seq_count=b - a) for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), counts)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), rows)
        gc, gr = ctx.table_profile(d, k, seq_first=5)                    # seq_count = None: all from there on
        assert np.array_equal(gc, counts[5:]) and np.array_equal(gr, rows[5:])
        gc, gr = ctx.table_profile(d, k, seq_first=1, seq_count=3)       # empty sequences only
        assert gc.shape == (3, width) and not gc.any() and not gr.any()
        for first in (0, 3, n):
            gc, gr = ctx.table_profile(d, k, seq_first=first, seq_count=0)
            assert gc.shape == (0, width) and gr.shape == (0,)
        for first, count in ((n + 1, 0), (n - 2, 3), (0, n + 1), (n, 1)):
            with pytest.raises(pkg.DnaGpuError) as ei:
                ctx.table_profile(d, k, seq_first=first, seq_count=count)
            assert ei.value.code == BAD_ARG
        for first, count, pad in ((0, n, 64), (3, 9, 64), (17, 3, 1), (6, 1, 3)):
            before, got, after, grows = device_profile(ctx, d, k, count, width, seq_first=first, pad=pad)
            assert (before == SENTINEL32).all() and (after == SENTINEL32).all()
            assert np.array_equal(got, counts[first:first + count]) and np.array_equal(grows, rows[first:first + count])
        before, got, after, _ = device_profile(ctx, d, k, n, width, pad=5, want_rows=False)
        assert (before == SENTINEL32).all() and (after == SENTINEL32).all() and np.array_equal(got, counts)
        buf = np.full(n * width + 2, SENTINEL32, dtype=np.uint32)        # host output, rows not wanted
        assert pkg.lib().dnagpu_table_profile(ctx.h, d.h, k, 0, 0, n, buf[1:].ctypes.data, None, 0) == 0
        assert buf[0] == SENTINEL32 and buf[-1] == SENTINEL32 and np.array_equal(buf[1:-1].reshape(n, width), counts)
    finally:
        d.free()


@pytest.mark.gpu
def test_profile_of_a_wrapped_view(ctx, dbg):
    """a dnagpu_dna_wrap view whose bits and words behind the last base are poisoned gives what a clean upload gives"""
    k = 4
    texts = random_texts([100, 0, 9000, 37, 2100], SEED + 40)            # 11,237 bases: the last word is partial
    words, starts = encode_table(texts)
    n_bases = int(starts[-1])
    nw = (n_bases + 31) // 32
    assert n_bases % 32
    dirty = words[:nw].copy()
    dirty[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(2 * (n_bases % 32))
    buf = ctx.buffer_alloc(8 * (nw + 4))
    try:
        ctx.upload_u64(buf, np.concatenate([dirty, np.full(4, 0x9E9E9E9E9E9E9E9E, dtype=np.uint64)]))
        view = ctx.wrap(buf, nw, n_bases)
        view.set_sequences(starts)
        check_profile(ctx, view, texts, k, "wrapped view")
        check_profile(ctx, view, texts, k, "wrapped view, canonical", canonical=True)
        view.free()
    finally:
        ctx.buffer_free(buf)


PALINDROMES = {2: ["AT", "TA", "CG", "GC"], 4: ["ATAT", "ACGT", "GGCC", "TTAA"], 6: ["AAATTT", "ACGCGT", "GATATC"]}


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_profile_canonical(ctx, pkg, dbg, k):
    """the canonical profile equals numpy's fold of the forward result; non-canonical columns are 0; a k-mer that is its own
    reverse complement counts once; the table of reverse complements (dnagpu_dna_take with every flip set) has the same
    canonical profile"""
    pal = PALINDROMES.get(k, [])
    texts = random_texts([300, 0, 2500, k, 9000, 64], SEED + 50 + k) + pal
    cols = np.arange(4 ** k, dtype=np.uint64)
    not_canon = canonical_np(cols, k) != cols
    d = resident(ctx, texts)
    try:
        fwd = check_profile(ctx, d, texts, k, "forward")
        canon = check_profile(ctx, d, texts, k, "canonical", canonical=True)
        assert np.array_equal(canon, fold_np(fwd, k))
        assert not canon[:, not_canon].any() and fwd[:, not_canon].any()
        for i, p in enumerate(pal):
            assert revcomp_text(p) == p
            row = canon[len(texts) - len(pal) + i]
            assert row.sum() == 1 and row[int(orc.dna_encode(p)[0][0])] == 1
        back = ctx.dna_take(d, np.arange(len(texts)), flip=np.ones(len(texts)))
        try:
            gc, gr = ctx.table_profile(back, k, canonical=True)
            assert np.array_equal(gc, canon)
            assert np.array_equal(gc, ref_profile([revcomp_text(t) for t in texts], k, canonical=True)[0])
        finally:
            back.free()
    finally:
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_profile_against_the_count_engine(ctx, dbg, k):
    """row sums = out_rows = the oracle's rows; column sums over the whole table = dnagpu_count_kmers_table's histogram"""
    texts = random_texts([100] * 50 + [0, 5, 12_000, 2047 + k, 2048 + k, 3], SEED + 60 + k)
    d = resident(ctx, texts)
    try:
        gc = check_profile(ctx, d, texts, k, "forward")
        h = ctx.count_kmers_table(d, k)
        try:
            hk, hc = h.download()
        finally:
            h.free()
        col = gc.sum(axis=0, dtype=np.uint64)
        at = np.flatnonzero(col)
        order = np.argsort(hk)
        assert np.array_equal(hk[order], at.astype(np.uint64)) and np.array_equal(hc[order], col[at])
    finally:
        d.free()


@pytest.mark.gpu
def test_profile_errors_write_nothing(ctx, pkg, dbg):
    """k = 0 and 33 are INVALID_K, k = 7 and 32 TOO_LARGE (with a text), flags = 2 BAD_ARG, a stream without a sequence set
    BAD_ARG, a NULL out_counts BAD_ARG: a host and a device output pre-filled with a sentinel are untouched after each"""
    L = pkg.lib()
    texts = random_texts([40, 0, 3000], SEED + 70)
    n = len(texts)
    d = resident(ctx, texts)
    words, starts = encode_table(texts)
    bare = ctx.upload(words, int(starts[-1]))
    host = np.full(n * 4096, SENTINEL32, dtype=np.uint32)
    hrows = np.full(n, 77, dtype=np.uint64)
    dev = ctx.buffer_alloc(4 * n * 4096)
    drows = ctx.buffer_alloc(8 * n)
    try:
        ctx.upload_bytes(dev, host.view(np.uint8))
        ctx.upload_u64(drows, hrows)
        cases = [(d, 0, 0, INVALID_K), (d, 33, 0, INVALID_K), (d, -1, 1, INVALID_K), (d, 7, 0, TOO_LARGE), (d, 32, 1, TOO_LARGE),
                 (d, 4, 2, BAD_ARG), (d, 0, 2, BAD_ARG), (bare, 4, 0, BAD_ARG)]
        for dna, k, flags, code in cases:
            count = n if dna is d else 0                                  # (a table without a set has no sequence to ask for)
            assert L.dnagpu_table_profile(ctx.h, dna.h, k, flags, 0, count, host.ctypes.data, hrows.ctypes.data, 0) == code
            assert L.dnagpu_table_profile(ctx.h, dna.h, k, flags, 0, count, dev, drows, 1) == code
            if code == TOO_LARGE:
                assert b"dense profile" in L.dnagpu_last_error()
        assert L.dnagpu_table_profile(ctx.h, bare.h, 4, 0, 0, 1, host.ctypes.data, hrows.ctypes.data, 0) == BAD_ARG
        assert L.dnagpu_table_profile(ctx.h, d.h, 4, 0, 0, n, None, hrows.ctypes.data, 0) == BAD_ARG
        assert L.dnagpu_table_profile(ctx.h, d.h, 4, 0, 0, n, None, drows, 1) == BAD_ARG
        assert L.dnagpu_table_profile(ctx.h, d.h, 4, 0, 0, 0, None, None, 0) == 0      # nothing asked for: nothing needed
        assert (host == SENTINEL32).all() and (hrows == 77).all()
        assert (ctx.download_bytes(dev, 4 * n * 4096).view(np.uint32) == SENTINEL32).all()
        assert (ctx.download_u64(drows, n) == 77).all()
    finally:
        ctx.buffer_free(dev)
        ctx.buffer_free(drows)
        bare.free()
        d.free()


class EmptyRow:
    """a row of no bases as the glue's C interface takes it (glue/dna_glue.h: struct Dna); the `dna` type itself has no
    empty value, dna_in refuses one"""

    class _Dna(C.Structure):
        _fields_ = [("length", C.c_uint64), ("bit_sequence", C.c_void_p), ("dev", C.c_void_p)]

    def __init__(self):
        self._row = self._Dna(0, None, None)
        self.p = C.addressof(self._row)


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [False, True], ids=["forward", "canonical"])
def test_glue_table_profile(g, ctx, dbg, canonical):
    """at least five batches through the glue with a small flush size -- one row longer than a batch, empty rows -- against the
    reference in add order"""
    k = 3
    lengths = [100] * 14 + [0, 2, 400, 0] + [100] * 34 + [0, 0, 37]
    lengths[20] = 2600                                                    # longer than a batch: a batch of its own
    texts = random_texts(lengths, SEED + 80)
    assert 5 * 1500 <= sum(lengths)
    counts, rows = ref_profile(texts, k, canonical)
    g.set_agg_flush_bases(1500)
    try:
        got = list(g.table_profile([t if t else EmptyRow() for t in texts], k, canonical=canonical))
    finally:
        g.set_agg_flush_bases(1 << 30)
    assert [s for s, _, _ in got] == list(range(len(texts)))
    assert np.array_equal(np.array([r for _, r, _ in got], dtype=np.uint64), rows)
    assert np.array_equal(np.stack([c for _, _, c in got]).astype(np.uint32), counts)
