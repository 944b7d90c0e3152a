"""Strand-neutral k-mers: the reverse complement of a dna and of a kmer, the canonical form, and the
canonical add of the accumulator (dnagpu_dna_revcomp, dnagpu_kmer_strand, dnagpu_acc_add_canonical) with the glue on top.
CPU tests: strand_math.hpp as a host program (plain and with sanitizers), the argument rules that need no device, the glue's
per-datum functions.  GPU tests: numpy is the reference -- rc and the canonical choice are loops over the k fields of uint64
arrays, the canonical groups are the oracle's forward groups folded with them."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import ROOT, load_package
from acc_model import splitmix64 as splitmix64_np

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
EVEN = 0x5555555555555555
A32, T32, C32, G32 = np.uint64(0), np.uint64(EVEN), np.uint64(~EVEN & (2 ** 64 - 1)), ONES
INVALID_K, BAD_ARG, DNA_EMPTY = 1, 5, 11
COMPLEMENT = str.maketrans("ATCG", "TAGC")
EXAMPLE = "ATCGATCGATCGATCGACG"                     # test.sql:95


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


def revcomp_text(t):
    return t[::-1].translate(COMPLEMENT)


# ------------------------------------------------------------------ the numpy reference

def mask_of(k):
    return np.uint64((1 << (2 * k)) - 1)


def rc_np(keys, k):
    """rc of every key: field i of the result = field k - 1 - i of the key, complemented (code ^ 1)"""
    keys = np.asarray(keys, dtype=np.uint64) & mask_of(k)
    out = np.zeros_like(keys)
    for i in range(k):
        out |= (((keys >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)) ^ np.uint64(1)) << np.uint64(2 * i)
    return out


def rank_np(keys, k):
    """the number whose order is text order under A < T < C < G: base 0 in the top field"""
    keys = np.asarray(keys, dtype=np.uint64)
    out = np.zeros_like(keys)
    for i in range(k):
        out |= ((keys >> np.uint64(2 * i)) & np.uint64(3)) << np.uint64(2 * (k - 1 - i))
    return out


def canonical_np(keys, k):
    keys = np.asarray(keys, dtype=np.uint64) & mask_of(k)
    rc = rc_np(keys, k)
    return np.where(rank_np(keys, k) <= rank_np(rc, k), keys, rc)


def add_up(keys, counts):
    """equal keys summed -> (keys ascending, uint64 counts)"""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts).astype(np.uint64)
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    if not len(keys):
        return keys, counts
    at = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return keys[at], np.add.reduceat(counts, at).astype(np.uint64)


def fold_np(keys, counts, k):
    """forward groups -> canonical groups: count(x) + count(rc(x)), a palindrome's count as it is"""
    return add_up(canonical_np(keys, k), counts)


_SEQ = {}


def both_strands(seed, n, motif=0):
    """n synthetic bases whose second half is the reverse complement of the first: every k-mer's partner is there too.
    -> (text, words, forward groups by k) -- computed once, never modified"""
    key = (seed, n, motif)
    if key not in _SEQ:
        h = n // 2
        w = orc.synth_words_repeat(seed, h, motif) if motif else orc.synth_words(seed, h)
        t = orc.dna_decode(w, h)
        text = t + revcomp_text(t)
        _SEQ[key] = (text, orc.dna_encode(text)[0], {})
    return _SEQ[key]


def forward_groups(seed, n, k, motif=0):
    text, words, by_k = both_strands(seed, n, motif)
    if k not in by_k:
        by_k[k] = orc.count_kmers(words, len(text), k)
    return by_k[k]


def check_acc(acc, ek, ec, what):
    gk, gc = acc.download()
    assert acc.distinct == len(ek), f"{what}: {acc.distinct} groups, expected {len(ek)}"
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], ek), what + " keys"
    assert np.array_equal(gc[order], ec), what + " counts"
    assert acc.total == int(ec.sum(dtype=np.uint64)), what + " total"
    assert acc.summary() == orc.hist_summary(ek, ec), what + " summary"


# ------------------------------------------------------------------ CPU: what needs no device

SANITIZERS = ["-g", "-Xarch_host", "-fsanitize=address,undefined"]


@pytest.mark.parametrize("extra", [[], SANITIZERS], ids=["plain", "sanitizers"])
def test_strand_math_on_the_host(tmp_path, extra):
    """strand_math.hpp, host code of the header the kernels share, as a stand-alone program (the second build with
    AddressSanitizer and UndefinedBehaviorSanitizer on it): rc against a per-base loop for k in 1, 2, 5, 16, 31, 32, the
    r <= key ^ M identity, 16 and 0 palindromes at k = 4 and 5, the 32-base corners, the windows of the dna kernel"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "strand_math_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", *extra, "-I",
                           os.path.join(ROOT, "dna-sequences-pg-extension_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "strand_math_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_tests_reference_on_the_worked_example():
    """a guard on the numpy reference itself, against text: test.sql:95's groups fold into ATCGA 7, CGATC 6, CGACG 1,
    TCGAC 1.  It runs no code of the project (so it passes with or without the feature): what it protects is every GPU
    test below, which trusts rc_np, canonical_np and fold_np"""
    fk, fc = orc.count_kmers(*orc.dna_encode(EXAMPLE), 5)
    for key in fk:
        t = orc.kmer_decode(key, 5)
        assert orc.kmer_decode(rc_np([key], 5)[0], 5) == revcomp_text(t)
        order = "ATCG"
        first = min(t, revcomp_text(t), key=lambda s: [order.index(c) for c in s])
        assert orc.kmer_decode(canonical_np([key], 5)[0], 5) == first
    ck, cc = fold_np(fk, fc, 5)
    assert {orc.kmer_decode(a, 5): int(b) for a, b in zip(ck, cc)} == {"ATCGA": 7, "CGATC": 6, "CGACG": 1, "TCGAC": 1}
    assert orc.hist_summary(ck, cc)[:3] == (15, 4, 2)
    assert revcomp_text(EXAMPLE) == "CGTCGATCGATCGATCGAT"
    pal4 = [x for x in range(256) if rc_np([x], 4)[0] == x]
    assert len(pal4) == 16 and not any(rc_np([x], 5)[0] == x for x in range(1024))


def test_strand_argument_rules_without_a_device(pkg):
    L = pkg.lib()
    out = C.c_void_p(77)
    assert L.dnagpu_dna_revcomp(None, None, 0, 1, C.byref(out)) == BAD_ARG
    assert L.dnagpu_dna_revcomp(None, None, 0, 0, None) == BAD_ARG
    assert out.value == 77
    keys = np.arange(4, dtype=np.uint64)
    res = np.full(4, 99, dtype=np.uint64)
    for mode in (-1, 2, 100):                     # the mode first ...
        assert L.dnagpu_kmer_strand(None, keys.ctypes.data, 4, 0, mode, res.ctypes.data, None, 0) == BAD_ARG
    for mode in (pkg.STRAND_REVCOMP, pkg.STRAND_CANONICAL):
        for k in (0, 33, -1):                     # ... then k ...
            assert L.dnagpu_kmer_strand(None, None, 4, k, mode, None, None, 0) == INVALID_K
        assert L.dnagpu_kmer_strand(None, keys.ctypes.data, 4, 5, mode, res.ctypes.data, None, 0) == BAD_ARG   # ... then NULLs
        assert L.dnagpu_kmer_strand(None, None, 0, 5, mode, None, None, 0) == BAD_ARG                         # (no context)
    assert np.all(res == 99)
    assert L.dnagpu_acc_add_canonical(None, None, None) == BAD_ARG
    assert (pkg.STRAND_REVCOMP, pkg.STRAND_CANONICAL) == (0, 1)
    assert pkg.abi_version() == 2


def test_glue_strand_functions_of_one_value(g):
    assert str(g.reverse_complement(g.dna(EXAMPLE))) == "CGTCGATCGATCGATCGAT"
    for n in (1, 31, 32, 33, 64, 65, 100):
        t = orc.dna_decode(orc.synth_words(0x57A0 + n, n), n)
        r = g.reverse_complement(g.dna(t))
        assert str(r) == revcomp_text(t) and len(r) == n
        assert str(g.reverse_complement(r)) == t
    want = {"ATCGA": "ATCGA", "TCGAT": "ATCGA", "CGATC": "CGATC", "GATCG": "CGATC", "CGACG": "CGACG", "TCGAC": "TCGAC",
            "CGTCG": "CGACG", "GTCGA": "TCGAC"}
    for t, c in want.items():
        assert str(g.reverse_complement(g.kmer(t))) == revcomp_text(t)
        assert str(g.canonical(g.kmer(t))) == c
    for pal in ("ATAT", "ACGT", "GGCC", "AT", "G" * 16 + "C" * 16):      # a palindrome is its own canonical form
        assert str(g.reverse_complement(g.kmer(pal))) == pal and str(g.canonical(g.kmer(pal))) == pal
    assert str(g.canonical(g.kmer("G" * 32))) == "C" * 32 and str(g.canonical(g.kmer("T" * 32))) == "A" * 32
    assert str(g.canonical(g.kmer("A" * 32))) == "A" * 32 and str(g.canonical(g.kmer("C" * 32))) == "C" * 32
    rng = np.random.default_rng(3)
    for k in (1, 2, 15, 16, 31, 32):
        for key in rng.integers(0, 1 << 63, 50, dtype=np.uint64) * np.uint64(2) & mask_of(k):
            km = g.kmer(orc.kmer_decode(key, k))
            assert g.reverse_complement(km).c.bit_sequence == int(rc_np([key], k)[0])
            assert g.canonical(km).c.bit_sequence == int(canonical_np([key], k)[0])


def test_glue_canonical_aggregate_bad_k_is_the_references_error(g):
    for k in (0, 33, -1):
        with pytest.raises(g.GlueError) as ei:
            g.count_kmers_agg_canonical([], k)
        assert str(ei.value) == "Invalid k value: must be between 1 and 32"          # dna.c:773


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def check_revcomp(ctx, d, text, first, count, what):
    r = ctx.dna_revcomp(d, first, count)
    try:
        want = revcomp_text(text[first:first + count])
        assert r.n_bases == count, what
        assert ctx.unpack(r) == want, what
        words = r.download()
        assert len(words) == (count + 31) // 32
        if count % 32:
            assert int(words[-1]) >> (2 * (count % 32)) == 0, what + ": bits behind the last base"
        assert np.array_equal(words, orc.dna_encode(want)[0]), what + " words"
        back = ctx.dna_revcomp(r)
        assert ctx.unpack(back) == text[first:first + count], what + " twice"
        assert np.array_equal(back.download(), orc.dna_encode(text[first:first + count])[0]), what + " twice, words"
        back.free()
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 1000, 4097])
def test_dna_revcomp_lengths_and_windows(ctx, pkg, n):
    words = orc.synth_words(0x57A1000 + n, n)
    text = orc.dna_decode(words, n)
    d = ctx.upload(words, n)
    check_revcomp(ctx, d, text, 0, n, f"n={n}")
    if n == 4097:
        for first, count in ((5, 70), (31, 2), (32, 32), (1, 4095), (4096, 1), (4065, 32), (0, 4096)):
            check_revcomp(ctx, d, text, first, count, f"window ({first}, {count})")
        out = C.c_void_p()
        L = pkg.lib()
        for first, count in ((4098, 0), (4097, 1), (0, 4098), (5, 4093), (1, 2 ** 64 - 1)):
            assert L.dnagpu_dna_revcomp(ctx.h, d.h, first, count, C.byref(out)) == BAD_ARG, (first, count)
        assert L.dnagpu_dna_revcomp(ctx.h, d.h, 0, 0, C.byref(out)) == DNA_EMPTY
        assert L.dnagpu_dna_revcomp(ctx.h, d.h, 4097, 0, C.byref(out)) == DNA_EMPTY
        assert L.dnagpu_dna_revcomp(ctx.h, d.h, 0, 10, None) == BAD_ARG
        assert L.dnagpu_dna_revcomp(ctx.h, None, 0, 10, C.byref(out)) == BAD_ARG
    d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n_bases", [135, 128, 1])
def test_dna_revcomp_of_a_view_inside_a_buffer(ctx, n_bases):
    """a dnagpu_dna_wrap view in the middle of a buffer of random words: nonzero bits behind its last base and all around
    it; the result is that of the view's own bases, whatever the surroundings hold"""
    rng = np.random.default_rng(0x57A2)
    w0, nw = 3, (n_bases + 31) // 32
    results = []
    for trial in range(2):
        buf = rng.integers(0, 1 << 63, 16, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        if trial == 0:
            view = buf[w0:w0 + nw].copy()
        else:                                     # the same bases, everything behind and around them different
            keep = view.copy()
            if n_bases % 32:
                m = mask_of(n_bases % 32)
                keep[-1] = (keep[-1] & m) | (buf[w0 + nw - 1] & ~m)
            buf[w0:w0 + nw] = keep
        text = orc.dna_decode(buf[w0:w0 + nw], n_bases)
        if n_bases % 32:
            assert int(buf[w0 + nw - 1]) >> (2 * (n_bases % 32)) != 0
        ptr = ctx.buffer_alloc(8 * len(buf))
        ctx.upload_u64(ptr, buf)
        v = ctx.wrap(ptr + 8 * w0, nw, n_bases)
        check_revcomp(ctx, v, text, 0, n_bases, f"view of {n_bases} bases")
        if n_bases > 40:
            check_revcomp(ctx, v, text, 7, n_bases - 7, "window to the view's end")
            check_revcomp(ctx, v, text, 33, 64, "window inside the view")
        r = ctx.dna_revcomp(v)
        results.append(r.download())
        r.free()
        v.free()
        assert np.array_equal(ctx.download_u64(ptr, len(buf)), buf)             # (the source is read only)
        ctx.buffer_free(ptr)
    assert np.array_equal(results[0], results[1])


def strand_keys(k):
    rng = np.random.default_rng(0x57A3 + k)
    keys = rng.integers(0, 1 << 63, 10_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 10_000, dtype=np.uint64)
    keys[:5_000] &= mask_of(k)                    # (the rest keep their bits above 2k)
    pal4 = np.array([x for x in range(256) if rc_np([x], 4)[0] == x], dtype=np.uint64)
    assert len(pal4) == 16
    extra = np.array([0, int(mask_of(k)), EVEN & int(mask_of(k)), int(ONES), 1 << 63], dtype=np.uint64)
    return np.concatenate([keys, extra, pal4])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 4, 15, 16, 31, 32])
def test_kmer_strand_host_and_device(ctx, pkg, k):
    keys = strand_keys(k)
    n = len(keys)
    masked = keys & mask_of(k)
    want = {pkg.STRAND_REVCOMP: rc_np(keys, k), pkg.STRAND_CANONICAL: canonical_np(keys, k)}
    if k == 4:
        pal = keys[-16:]
        assert np.array_equal(want[pkg.STRAND_REVCOMP][-16:], pal) and np.array_equal(want[pkg.STRAND_CANONICAL][-16:], pal)
    for mode, exp in want.items():
        out, fl = ctx.kmer_strand(keys, k, mode)
        assert np.array_equal(out, exp), f"k={k} mode={mode} host"
        assert np.array_equal(fl, exp != masked), f"k={k} mode={mode} host flags"
        out2, none = ctx.kmer_strand(keys, k, mode, want_flipped=False)
        assert none is None and np.array_equal(out2, exp)
        # host arrays, in place
        inplace = keys.copy()
        rc = pkg.lib().dnagpu_kmer_strand(ctx.h, inplace.ctypes.data, n, k, mode, inplace.ctypes.data, None, 0)
        assert rc == 0 and np.array_equal(inplace, exp), f"k={k} mode={mode} host in place"
        # device arrays: out of place with flags, then in place
        dk, do, df = ctx.buffer_alloc(8 * n), ctx.buffer_alloc(8 * n), ctx.buffer_alloc(n)
        ctx.upload_u64(dk, keys)
        ctx.kmer_strand_device(dk, n, k, mode, do, df)
        assert np.array_equal(ctx.download_u64(do, n), exp), f"k={k} mode={mode} device"
        assert np.array_equal(ctx.download_bytes(df, n).astype(bool), exp != masked), f"k={k} mode={mode} device flags"
        assert np.array_equal(ctx.download_u64(dk, n), keys)
        ctx.kmer_strand_device(dk, n, k, mode, dk, df)
        assert np.array_equal(ctx.download_u64(dk, n), exp), f"k={k} mode={mode} device in place"
        assert np.array_equal(ctx.download_bytes(df, n).astype(bool), exp != masked)
        for p in (dk, do, df):
            ctx.buffer_free(p)
    L = pkg.lib()
    assert L.dnagpu_kmer_strand(ctx.h, None, 0, k, 1, None, None, 0) == 0                # n == 0
    assert L.dnagpu_kmer_strand(ctx.h, None, 5, k, 1, None, None, 0) == BAD_ARG
    assert L.dnagpu_kmer_strand(ctx.h, keys.ctypes.data, 5, 33, 1, None, None, 0) == INVALID_K
    assert L.dnagpu_kmer_strand(ctx.h, keys.ctypes.data, 5, 33, 7, None, None, 0) == BAD_ARG


@pytest.mark.gpu
def test_canonical_add_worked_example(ctx):
    d = ctx.pack(EXAMPLE)
    h = ctx.count_kmers(d, 5)
    acc = ctx.accumulator(5)
    acc.add(h, canonical=True)
    gk, gc = acc.download()
    assert {orc.kmer_decode(a, 5): int(b) for a, b in zip(gk, gc)} == {"ATCGA": 7, "CGATC": 6, "CGACG": 1, "TCGAC": 1}
    assert acc.summary()[:3] == (15, 4, 2) and acc.distinct == 4 and acc.total == 15
    check_acc(acc, *fold_np(*orc.count_kmers(*orc.dna_encode(EXAMPLE), 5), 5), "worked example")
    for o in (acc, h, d):
        o.free()


@pytest.mark.gpu
def test_canonical_add_dense_k4(ctx):
    """k = 4 over 5,000 bases: all 256 keys, both strands in one dense histogram, 16 palindromes -> 136 groups"""
    n, k = 5_000, 4
    words = orc.synth_words(0x57A4, n)
    fk, fc = orc.count_kmers(words, n, k)
    assert len(fk) == 256
    ek, ec = fold_np(fk, fc, k)
    assert len(ek) == 136
    pal = rc_np(fk, k) == fk
    assert pal.sum() == 16 and np.array_equal(ec[np.isin(ek, fk[pal])], fc[pal])      # (kept, not doubled)
    d = ctx.upload(words, n)
    h = ctx.count_kmers(d, k)
    acc = ctx.accumulator(k)
    acc.add(h, canonical=True)
    check_acc(acc, ek, ec, "k=4 dense")
    acc.add(h, canonical=True)
    check_acc(acc, ek, ec * np.uint64(2), "k=4 dense twice")
    for o in (acc, h, d):
        o.free()


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["ordered", "superkmer"])
@pytest.mark.parametrize("k", [5, 10, 21, 31, 32])
def test_canonical_add_exact_groups(ctx, pkg, k, engine):
    """200,000 synthetic bases, the second half the reverse complement of the first (so that at every k both strands of a
    k-mer are in ONE histogram), through count_kmers and through count_kmers_unordered with the super-k-mer engine forced
    (repeat-rich input: its histogram has padding slots): groups, summary and distinct == the folded forward groups"""
    n, seed = 200_000, 0x57A5 << 32
    motif = 1_000 if engine == "superkmer" else 0
    text, words, _ = both_strands(seed, n, motif)
    fk, fc = forward_groups(seed, n, k, motif)
    ek, ec = fold_np(fk, fc, k)
    assert len(ek) < len(fk)
    d = ctx.upload(words, n)
    if engine == "ordered":
        h = ctx.count_kmers(d, k)
    else:
        ctx.set_debug(pkg.DEBUG_FORCE_SUPERKMER)
        try:
            h = ctx.count_kmers_unordered(d, k)
        finally:
            ctx.set_debug(0)
        print(f"k={k}: sorted={h.is_sorted} extent={h.extent} distinct={h.distinct}")
        assert h.extent >= h.distinct
        if k >= 21:                               # (below that the engine is not taken: an ordered histogram)
            assert not h.is_sorted and h.extent > h.distinct, "no padding slots in the unordered histogram"
    assert h.distinct == len(fk) and h.total == n - k + 1
    acc = ctx.accumulator(k)
    acc.add(h, canonical=True)
    check_acc(acc, ek, ec, f"k={k} {engine}")
    assert acc.total == h.total
    for o in (acc, h, d):
        o.free()


@pytest.mark.gpu
def test_canonical_add_of_the_32_base_corners(ctx):
    """a hand-made key array at k = 32 through count_keys_device: A x 32, T x 32, C x 32, G x 32 and duplicates -> 2 groups;
    G x 32 (the all-ones key) folds into C x 32, T x 32 into key 0"""
    keys = np.array([A32, T32, C32, G32, G32, T32, T32, A32, G32, C32, G32], dtype=np.uint64)
    ptr = ctx.buffer_alloc(8 * len(keys))
    ctx.upload_u64(ptr, keys)
    h = ctx.count_keys_device(ptr, len(keys), 32)
    assert h.distinct == 4
    acc = ctx.accumulator(32)
    acc.add(h, canonical=True)
    gk, gc = acc.download()
    assert dict(zip(gk.tolist(), gc.tolist())) == {int(A32): 5, int(C32): 6}
    check_acc(acc, *fold_np(*orc.count_keys(keys), 32), "corners")
    acc.add(h)                                    # a plain add afterwards: G x 32 and T x 32 are groups of their own again
    assert acc.distinct == 4 and acc.total == 22
    for o in (acc, h):
        o.free()
    ctx.buffer_free(ptr)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 32])
def test_canonical_counts_are_strand_neutral(ctx, k):
    """add_canonical(count(d)) and add_canonical(count(dna_revcomp(d))): the same summary and the same sorted download.
    No numpy fold involved."""
    n = 100_000
    d = ctx.synth(0x57A6 << 32, n)
    r = ctx.dna_revcomp(d)
    accs = []
    for x in (d, r):
        h = ctx.count_kmers_unordered(x, k)
        a = ctx.accumulator(k)
        a.add(h, canonical=True)
        h.free()
        accs.append(a)
    assert accs[0].summary() == accs[1].summary() and accs[0].distinct == accs[1].distinct > 0
    (k0, c0), (k1, c1) = accs[0].download(), accs[1].download()
    o0, o1 = np.argsort(k0, kind="stable"), np.argsort(k1, kind="stable")
    assert np.array_equal(k0[o0], k1[o1]) and np.array_equal(c0[o0], c1[o1])
    # ... and the forward sets of the two strands share next to nothing: the figure the canonical mode is for
    fwd = []
    for x in (d, r):
        h = ctx.count_kmers_unordered(x, k)
        a = ctx.accumulator(k)
        a.add(h)
        h.free()
        fwd.append(a)
    st_f = fwd[0].join(fwd[1], want_rows=False)[3]
    st_c = accs[0].join(accs[1], want_rows=False)[3]
    assert st_c.rows == accs[0].distinct and st_f.rows < fwd[0].distinct // 100
    for o in accs + fwd + [d, r]:
        o.free()


@pytest.mark.gpu
def test_canonical_add_into_a_resident_accumulator(ctx):
    """30,000 bases, then 200,000: growth past 16 partitions -- the arrivals overflow every bin, so the table is grown from
    the upper bound distinct + arrivals WITHOUT a dry run and the canonical merge commits into the grown table (the dry
    run is test_canonical_dry_run_counts_a_pair_once's); the same histogram again (every count doubles, distinct stays:
    phase A with paired arrivals), then a forward add of another sequence (the plain path composes); numpy throughout;
    windows of download tile the groups"""
    k = 21
    seeds = (0x57A7 << 32, 0x57A8 << 32, 0x57A9 << 32)
    acc = ctx.accumulator(k)
    have_k, have_c = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    hists = []
    for seed, n in ((seeds[0], 30_000), (seeds[1], 200_000)):
        text, words, _ = both_strands(seed, n)
        d = ctx.upload(words, n)
        h = ctx.count_kmers_unordered(d, k)
        d.free()
        acc.add(h, canonical=True)
        hists.append(h)
        ck, cc = fold_np(*forward_groups(seed, n, k), k)
        have_k, have_c = add_up(np.concatenate([have_k, ck]), np.concatenate([have_c, cc]))
        check_acc(acc, have_k, have_c, f"after {n} bases")
        if n == 30_000:
            assert acc.partitions == 16
    assert acc.partitions > 16
    distinct = acc.distinct
    acc.add(hists[1], canonical=True)
    ck, cc = fold_np(*forward_groups(seeds[1], 200_000, k), k)
    have_k, have_c = add_up(np.concatenate([have_k, ck]), np.concatenate([have_c, cc]))
    assert acc.distinct == distinct == len(have_k)
    check_acc(acc, have_k, have_c, "the same histogram again")
    # a forward add: its keys go in as they are
    n3 = 50_000
    w3 = orc.synth_words(seeds[2], n3)
    d3 = ctx.upload(w3, n3)
    h3 = ctx.count_kmers_unordered(d3, k)
    d3.free()
    acc.add(h3)
    fk, fc = orc.count_kmers(w3, n3, k)
    have_k, have_c = add_up(np.concatenate([have_k, fk]), np.concatenate([have_c, fc]))
    check_acc(acc, have_k, have_c, "+ a forward add")
    got_k, got_c, first = [], [], 0
    for w in (1, 49_999, 3, 70_001, acc.distinct):
        w = min(w, acc.distinct - first)
        a, b = acc.download(first, w)
        got_k.append(a)
        got_c.append(b)
        first += w
    assert first == acc.distinct
    gk, gc = np.concatenate(got_k), np.concatenate(got_c)
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], have_k) and np.array_equal(gc[order], have_c)
    for o in hists + [h3, acc]:
        o.free()


def per_partition(keys, pbits):
    """keys per partition of a table of 2^pbits partitions: the top pbits bits of splitmix64(key) (acc_kernels.hip)"""
    return np.bincount((splitmix64_np(keys) >> np.uint64(64 - pbits)).astype(np.int64), minlength=1 << pbits)


ACC_SLOTS, ACC_BOUND = 4096, 3584                 # (dnagpu_api.hip: a merge runs only when no partition can end above the bound)


@pytest.mark.gpu
def test_canonical_dry_run_counts_a_pair_once(ctx):
    """the dry run of the canonical merge (commit == 0): the host takes it when occ + arrivals of some partition is above
    the bound although the bins fit, and sizes the table from the number of NEW keys it reports.  A 16-partition table
    holding 24,980 groups (about 1,560 a partition) takes a both-strands histogram of 34,980 groups, 17,490 pairs: about
    2,186 arrivals a partition, so occ + arrivals is about 3,747 > 3,584 while occ + new keys is about 2,654.  A dry run
    that reports the pairs once lets the merge commit into the 16 partitions; one that counted a pair twice (or a table
    sized from the arrivals) would grow it.  Then the same histogram again, now at occ about 2,655: every arrival is
    resident and paired, the dry run reports 0 new keys, and nothing grows.  The three conditions are asserted with numpy
    from the keys' partitions, so the test cannot pass by missing the branch; the groups are numpy's throughout."""
    k, pbits = 21, 4
    n1, n2 = 25_000, 35_000
    w1 = orc.synth_words(0x57B0 << 32, n1)
    f1k, f1c = orc.count_kmers(w1, n1, k)
    have_k, have_c = fold_np(f1k, f1c, k)
    text2, w2, _ = both_strands(0x57B1 << 32, n2)
    f2k, f2c = forward_groups(0x57B1 << 32, n2, k)
    c2k, c2c = fold_np(f2k, f2c, k)
    assert len(c2k) * 2 == len(f2k)               # every arrival has its partner in the same histogram
    acc = ctx.accumulator(k)
    hs = []
    for words, n in ((w1, n1), (w2, n2)):
        d = ctx.upload(words, n)
        hs.append(ctx.count_kmers_unordered(d, k))
        d.free()
    acc.add(hs[0], canonical=True)
    assert acc.partitions == 1 << pbits
    check_acc(acc, have_k, have_c, "the resident groups")
    for step in ("pairs new to the table", "the same pairs again"):
        occ = per_partition(have_k, pbits)
        arrivals = per_partition(canonical_np(f2k, k), pbits)
        new = per_partition(np.setdiff1d(c2k, have_k), pbits)
        mean = -(-len(f2k) // (1 << pbits))
        cap = min(ACC_SLOTS, (mean + 8 * int(np.sqrt(mean)) + 32 + 31) // 32 * 32)          # the host's bin size
        assert arrivals.max() <= cap, "the bins overflow: the host would skip the dry run"
        assert (occ + arrivals).max() > ACC_BOUND, "no dry run: the add commits at once"
        assert (occ + new).max() <= ACC_BOUND
        assert new.sum() == (len(c2k) if step.startswith("pairs") else 0)
        acc.add(hs[1], canonical=True)
        have_k, have_c = add_up(np.concatenate([have_k, c2k]), np.concatenate([have_c, c2c]))
        assert acc.partitions == 1 << pbits, f"{step}: the table grew to {acc.partitions} partitions"
        check_acc(acc, have_k, have_c, step)
    for o in hs + [acc]:
        o.free()


@pytest.mark.gpu
def test_canonical_add_of_a_merge_result_and_errors(ctx, pkg):
    """a dnagpu_hist_merge result as the source; a histogram of another k is BAD_ARG and leaves summary() and download()
    as they were"""
    k, n = 31, 60_000
    seed_a, seed_b = 0x57AA << 32, 0x57AB << 32
    ta, wa, _ = both_strands(seed_a, n)
    tb, wb, _ = both_strands(seed_b, n)
    da, db = ctx.upload(wa, n), ctx.upload(wb, n)
    ha, hb = ctx.count_kmers(da, k), ctx.count_kmers_unordered(db, k)
    m = ha.merge(hb)
    acc = ctx.accumulator(k)
    acc.add(m, canonical=True)
    fa, fb = forward_groups(seed_a, n, k), forward_groups(seed_b, n, k)
    ek, ec = fold_np(np.concatenate([fa[0], fb[0]]), np.concatenate([fa[1], fb[1]]), k)
    check_acc(acc, ek, ec, "merge result")
    before = (acc.distinct, acc.total, acc.summary(), [x.tolist() for x in acc.download()])
    h21 = ctx.count_kmers(da, 21)
    with pytest.raises(pkg.DnaGpuError) as ei:
        acc.add(h21, canonical=True)
    assert ei.value.code == BAD_ARG
    L = pkg.lib()
    assert L.dnagpu_acc_add_canonical(ctx.h, acc.h, None) == BAD_ARG
    assert L.dnagpu_acc_add_canonical(ctx.h, None, ha.h) == BAD_ARG
    assert L.dnagpu_acc_add_canonical(None, acc.h, ha.h) == BAD_ARG
    assert (acc.distinct, acc.total, acc.summary(), [x.tolist() for x in acc.download()]) == before
    for o in (acc, m, ha, hb, h21, da, db):
        o.free()


@pytest.mark.gpu
def test_canonical_add_takes_histograms_of_several_parts(pkg):
    """the one-process multi-rank count on one device, as test_acc_takes_histograms_of_several_parts makes its histograms
    (several parts, no recorded k): added canonically head by head, and part by part through dnagpu_hist_part views.
    64 M groups are too many to fold and sort with numpy in a few seconds (an argsort of that size alone takes over ten),
    so the reference here is the canonical add of the one-context histogram of the same sequence -- the path the tests
    above hold against numpy.  The groups are compared exactly, on the device: the INNER join (test_kmer_join.py holds it
    against numpy) of either accumulator with the reference pairs every group, and sum(min(a, b)) equal to both sums
    leaves no key with two different counts.  numpy checks what it can afford: the total, distinct <= the forward groups,
    and that a window of 200,000 downloaded keys is canonical and distinct."""
    seed, k, n = 0x57AC, 31, 64_000_000
    L = pkg.lib()
    with pkg.Multi([0, 0], pkg.MULTI_COPY) as m:
        m.set_parts(3)
        d = m.synth(seed, n)
        hs = m.count_unordered(d, k)
        m.dna_free(d)
        assert any(h.n_parts > 1 for h in hs), [h.n_parts for h in hs]
        c0 = m.ranks[0]
        heads, views = c0.accumulator(k), c0.accumulator(k)
        for h in hs:
            heads.add(h, canonical=True)
            for i in range(h.n_parts):
                part = L.dnagpu_hist_part(h.h, i)
                assert part
                assert L.dnagpu_acc_add_canonical(c0.h, views.h, part) == 0
        forward = sum(h.distinct for h in hs)
        for h in hs:
            h.free()
        one = c0.synth(seed, n)
        h1 = c0.count_kmers_unordered(one, k)
        one.free()
        ref = c0.accumulator(k)
        ref.add(h1, canonical=True)
        h1.free()
        assert heads.total == n - k + 1 and views.total == heads.total
        assert heads.summary() == ref.summary() == views.summary()
        assert 0 < heads.distinct <= forward
        for a in (heads, views):
            st = a.join(ref, want_rows=False)[3]
            assert st.rows == a.distinct == ref.distinct
            assert st.sum_left == st.sum_right == st.sum_min == ref.total
        wk, wc = heads.download(heads.distinct // 3, 200_000)
        assert np.array_equal(canonical_np(wk, k), wk) and len(np.unique(wk)) == len(wk) and wc.min() >= 1
        for a in (heads, views, ref):
            a.free()


@pytest.mark.gpu
def test_glue_canonical_aggregate_is_strand_neutral(g):
    """count_kmers_agg_begin_canonical(31) over a small table of reads and over the same reads reverse-complemented row by
    row: the groups are equal (and the numpy fold of the oracle's groups); count_kmers_join of the two gives Jaccard 1"""
    k = 31
    rng = np.random.default_rng(0x57AD)
    genome = orc.dna_decode(orc.synth_words(0x57AE << 32, 6_000), 6_000)
    reads = []
    for _ in range(300):
        at, ln = int(rng.integers(0, 5_800)), int(rng.integers(20, 200))
        reads.append(genome[at:at + ln])
    reads.append("ACGT" * 20)                     # (its 31-mers come in reverse-complement pairs inside one row)
    flipped = [revcomp_text(r) for r in reads]
    keys = np.concatenate([orc.generate_kmers(*orc.dna_encode(r), k, faithful=False) for r in reads if len(r) >= k])
    ek, ec = fold_np(*orc.count_keys(keys), k)
    g.set_agg_flush_bases(3_000)
    try:
        with g.count_kmers_table_agg(k, reads, canonical=True) as a, g.count_kmers_table_agg(k, flipped, canonical=True) as b:
            rows, (n_rows, sum_l, sum_r, sum_min) = g.count_kmers_join(a, b, "i")
            ga, gb = a.groups(), b.groups()
        got, totals = g.count_kmers_agg_canonical(reads, k)
    finally:
        g.set_agg_flush_bases(1 << 30)
    for what, groups in (("reads", ga), ("reverse complements", gb), ("one call", got)):
        gk = np.array([km.c.bit_sequence for km, _ in groups], dtype=np.uint64)
        gc = np.array([c for _, c in groups], dtype=np.uint64)
        order = np.argsort(gk, kind="stable")
        assert np.array_equal(gk[order], ek) and np.array_equal(gc[order], ec), what
        assert all(km.c.length == k for km, _ in groups)
    assert totals == (int(ec.sum()), len(ek), int((ec == 1).sum()))
    d = len(ek)
    assert n_rows == d and n_rows / (d + d - n_rows) == 1.0                           # Jaccard
    assert sum_l == sum_r == sum_min == int(ec.sum())
    assert all(cl == cr for _, cl, cr in rows) and len(rows) == d
