"""Equal sequences on the device (dnagpu_dna_equals, dnagpu_table_classes, dnagpu_table_match) with the glue's
equals / dna_ne / table_distinct / table_match on top.  CPU tests: the argument rules that need no device, the Python reference on
test.sql:1-24's vectors, seqeq_math.hpp as a host program (plain and with sanitizers).  GPU tests: Python over the texts is the
reference -- rep[s] = the first index of texts[s], copies from a Counter, match = the first index in the build texts -- and
every comparison is equality.  Every GPU test runs twice: plainly, and with DNAGPU_DEBUG_POISON_POOL | DNAGPU_DEBUG_GUARD_POOL."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from test_table_hits import check_select_forms, encode_table, resident

BAD_ARG = 5
SEED = 0x5E9 << 32
SENTINEL = 0xC3C3C3C3C3C3C3C3
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


# ------------------------------------------------------------------ the Python reference

def ref_equals(a, b):
    return len(a) == len(b) and all(x == y for x, y in zip(a, b))


def ref_classes(texts):
    """-> (rep uint64[n], copies uint64[n], distinct)"""
    first, cnt = {}, Counter(texts)
    rep = np.array([first.setdefault(t, i) for i, t in enumerate(texts)], dtype=np.uint64)
    copies = np.array([cnt[t] for t in texts], dtype=np.uint64)
    return rep, copies, len(first)


def ref_match(probe, build):
    """-> (match uint64[n], copies uint64[n], n_matched)"""
    first, cnt = {}, Counter(build)
    for i, t in enumerate(build):
        first.setdefault(t, i)
    match = np.array([first.get(t, NONE) for t in probe], dtype=np.uint64)
    copies = np.array([cnt.get(t, 0) for t in probe], dtype=np.uint64)
    return match, copies, int((match != np.uint64(NONE)).sum())


def random_text(rng, n):
    return "".join(rng.choice(list("ATCG"), n)) if n else ""


def mutate(text, pos):
    return text[:pos] + "ATCG"[("ATCG".index(text[pos]) + 1) % 4] + text[pos + 1:]


# ------------------------------------------------------------------ CPU: what needs no device

def test_seq_equal_argument_rules_without_a_device(pkg):
    """the test that shows the feature: the symbols are absent before it"""
    L = pkg.lib()
    assert pkg.MATCH_NONE == 2 ** 64 - 1 and pkg.DEBUG_WEAK_FINGERPRINT == 8192 and pkg.abi_version() == 2
    wave_bases, tile_bases = pkg.seq_equal_geometry()
    assert 0 < wave_bases < tile_bases <= 2 ** 20 and tile_bases % 32 == 0
    assert L.dnagpu_seq_equal_geometry(None, None) == 0
    for name in ("dna_equals", "table_classes"):
        assert hasattr(pkg.Context, name)
    for name in ("read", "select", "members", "match", "free"):
        assert hasattr(pkg.SeqClasses, name)
    eq = C.c_int(77)
    assert L.dnagpu_dna_equals(None, None, None, C.byref(eq)) == BAD_ARG and eq.value == 77
    out = C.c_void_p(0x1234)
    assert L.dnagpu_table_classes(None, None, C.byref(out)) == BAD_ARG and out.value == 0x1234
    a = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
    b = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
    n = C.c_uint64(SENTINEL)
    assert L.dnagpu_seq_classes_read(None, None, 0, 2, a, b, 0) == BAD_ARG
    assert L.dnagpu_seq_classes_select(None, None, 1, NONE, a, b, 2, C.byref(n), 0) == BAD_ARG
    assert L.dnagpu_seq_classes_members(None, None, 0, a, 2, C.byref(n), 0) == BAD_ARG
    assert L.dnagpu_table_match(None, None, None, 0, 2, a, b, C.byref(n), 0) == BAD_ARG
    assert list(a) == [SENTINEL] * 2 and list(b) == [SENTINEL] * 2 and n.value == SENTINEL
    assert L.dnagpu_seq_classes_sequences(None) == 0 and L.dnagpu_seq_classes_distinct(None) == 0
    assert L.dnagpu_seq_classes_rounds(None) == 0
    L.dnagpu_seq_classes_free(None, None)


SQL_VECTORS = [("ATCG", "ATGCG", False), ("ATCG", "ATCG", True), ("ATCG", "GTCA", False)]       # test.sql:1-17


def test_the_tests_reference_on_test_sql(g):
    """a guard on the Python reference with test.sql:1-24's vectors, and the same four through the glue's equals / dna_ne"""
    for a, b, want in SQL_VECTORS:
        assert ref_equals(a, b) == want
        assert g.equals(a, b) == want and g.dna_ne(a, b) == (not want)
    assert not (not ref_equals("ATCG", "ATCG")) and g.dna_ne("ATCG", "ATCG") is False            # test.sql:20
    rep, copies, distinct = ref_classes(["ACG", "ACGA", "ACG", "T", "ACGAA"])
    assert rep.tolist() == [0, 1, 0, 3, 4] and copies.tolist() == [2, 1, 2, 1, 1] and distinct == 4
    match, copies, n = ref_match(["T", "G", "ACG"], ["ACG", "T", "ACG"])
    assert match.tolist() == [1, NONE, 0] and copies.tolist() == [1, 0, 2] and n == 2
    # the glue compares bases, not tail bits, and length is part of the identity
    assert not g.equals("ACG", "ACGA") and g.equals("A" * 33, "A" * 33) and not g.equals("A" * 32, "A" * 33)
    assert not g.equals("A" * 64 + "C", "A" * 64 + "G")
    assert not hasattr(g.dna, "__eq__") or g.dna.__eq__ is object.__eq__                        # hashing stays as it was


SANITIZERS = ["-g", "-Xarch_host", "-fsanitize=address,undefined"]


@pytest.mark.parametrize("extra", [[], SANITIZERS], ids=["plain", "sanitizers"])
def test_seqeq_math_on_the_host(tmp_path, extra):
    """seqeq_math.hpp, host code of the header the kernels share, as a stand-alone program (the second build with
    AddressSanitizer and UndefinedBehaviorSanitizer on it) against base-by-base restatements: the realigned word from a heap
    buffer of exactly n_words words, the fingerprint's invariances, the item sums and the item arithmetic"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "seqeq_math_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", *extra, "-I",
                           os.path.join(ROOT, "dna-sequences-pg-extension_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "seqeq_math_check.cpp"), "-o", exe])
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
    """every GPU test once as it is and once with poisoned, guarded pool buffers; the guard bands are checked afterwards.
    Yields the flags, so that a test can add DNAGPU_DEBUG_WEAK_FINGERPRINT to them."""
    flags = pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL if request.param == "poison" else 0
    ctx.set_debug(flags)
    yield flags
    assert pkg.lib().dnagpu_synchronize(ctx.h) == 0
    ctx.set_debug(0)


def check_classes(c, texts, what):
    rep, copies, distinct = ref_classes(texts)
    assert c.sequences == len(texts), what
    grep, gcop = c.read()
    bad = np.flatnonzero((grep != rep) | (gcop != copies))
    assert not len(bad), f"{what}: sequence {bad[:5]}: rep {grep[bad[:5]]} / {rep[bad[:5]]}, copies {gcop[bad[:5]]} / {copies[bad[:5]]}"
    assert c.distinct == distinct, what
    return rep, copies, distinct


def rounds_needed(pkg, flags, distinct):
    """the weak flag leaves four fingerprint values: a round settles at most four classes"""
    return (distinct + 3) // 4 if flags & pkg.DEBUG_WEAK_FINGERPRINT else min(distinct, 1)


@pytest.mark.gpu
def test_dna_equals(ctx, pkg, dbg):
    """lengths around the word, the read and one item: equal copies; variants that differ in the first base only, in the last
    base only, in length only (by trailing A's); two wrapped views of equal content with different junk behind the last base;
    the same object"""
    tile_bases = pkg.seq_equal_geometry()[1]
    rng = np.random.default_rng(SEED + 1)
    for n in (1, 31, 32, 33, 64, 65, tile_bases + 1):
        text = random_text(rng, n)
        w, _ = encode_table([text])
        a, b = ctx.upload(w, n), ctx.upload(w.copy(), n)
        others = [(mutate(text, 0), n), (mutate(text, n - 1), n), (text + "A", n + 1), (text + "AA", n + 2)]
        if n > 1:
            others.append((text[:-1], n - 1))
        try:
            assert ctx.dna_equals(a, b) and ctx.dna_equals(b, a) and ctx.dna_equals(a, a), n
            for t, m in others:
                o = ctx.upload(encode_table([t])[0], m)
                try:
                    assert not ctx.dna_equals(a, o) and not ctx.dna_equals(o, a), (n, m, t[:8])
                finally:
                    o.free()
            nw = (n + 31) // 32
            bufs = [ctx.buffer_alloc(8 * (nw + 2)) for _ in range(2)]
            try:
                views = []
                for buf, junk in zip(bufs, (0xFFFFFFFFFFFFFFFF, 0x5A5A5A5A5A5A5A5A)):
                    dirty = w[:nw].copy()
                    if n % 32:
                        dirty[-1] |= np.uint64(junk) << np.uint64(2 * (n % 32))
                    ctx.upload_u64(buf, np.concatenate([dirty, np.full(2, junk, dtype=np.uint64)]))
                    views.append(ctx.wrap(buf, nw + 2, n))
                assert ctx.dna_equals(views[0], views[1]) and ctx.dna_equals(views[0], a) and ctx.dna_equals(a, views[1]), n
                for v in views:
                    v.free()
            finally:
                for buf in bufs:
                    ctx.buffer_free(buf)
        finally:
            a.free()
            b.free()


def alignment_lengths(pkg):
    wave_bases = pkg.seq_equal_geometry()[0]
    return [1, 31, 32, 33, 63, 64, 65, wave_bases - 1, wave_bases, wave_bases + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(10))
def test_classes_at_every_alignment(ctx, pkg, dbg, which):
    """32 copies of one random content, copy i at alignment i of its word: each is preceded by a different random filler
    sequence of 0 .. 31 bases.  All copies fall into one class of 32 and the fillers are classed correctly too."""
    n = alignment_lengths(pkg)[which]
    rng = np.random.default_rng(SEED + 100 + which)
    content = random_text(rng, n)
    texts, end, aligns = [], 0, set()
    for i in range(32):
        filler = random_text(rng, (i - end) % 32)
        texts += [filler, content]
        aligns.add((end + len(filler)) % 32)
        end += len(filler) + n
    assert aligns == set(range(32))
    d = resident(ctx, texts)
    try:
        with ctx.table_classes(d) as c:
            rep, copies, _ = check_classes(c, texts, f"length {n}")
            assert copies[1] == 32 + (content in texts[0::2]) and (rep[1::2] == 1).all()
    finally:
        d.free()


def length_texts():
    """'A' * n for n in 0 .. 70, a second empty sequence, and pairs where one sequence is a prefix of the other"""
    texts = ["A" * n for n in range(71)] + ["", "ACGT" * 10, "ACGT" * 10 + "A", "ACGT" * 10 + "AA", "ACGT" * 8, "ACGT" * 16,
                                            "ACGT" * 16 + "T"]
    return texts


def mixed_texts(pkg):
    """5,000 sequences drawn from 300 distinct contents of lengths 0 .. 200 plus four long ones of which two are equal,
    shuffled"""
    wave_bases, tile_bases = pkg.seq_equal_geometry()
    rng = np.random.default_rng(SEED + 200)
    pool = list(dict.fromkeys([""] + [random_text(rng, int(n)) for n in rng.integers(1, 201, 330)]))[:300]
    assert len(pool) == 300
    twin = random_text(rng, tile_bases + 77)
    longs = [twin, random_text(rng, wave_bases + 1), twin, mutate(twin, tile_bases + 76)]
    texts = [pool[int(i)] for i in rng.integers(0, 300, 5000)] + longs
    return [texts[int(i)] for i in rng.permutation(len(texts))]


_TEXTS = {}


def cached(name, make, *a):
    if name not in _TEXTS:
        _TEXTS[name] = make(*a)
    return _TEXTS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("weak", [False, True], ids=["strong", "weak"])
def test_length_is_identity(ctx, pkg, dbg, weak):
    """runs of A of every length 0 .. 70 have the same words up to their last one: 71 classes, and the two empty sequences
    share one.  Under DNAGPU_DEBUG_WEAK_FINGERPRINT the results are identical and the build needs at least ceil(D / 4) rounds."""
    texts = cached("length", length_texts)
    flags = dbg | (pkg.DEBUG_WEAK_FINGERPRINT if weak else 0)
    ctx.set_debug(flags)
    d = resident(ctx, texts)
    try:
        with ctx.table_classes(d) as c:
            rep, copies, distinct = check_classes(c, texts, "runs of A")
            assert distinct == 77 and len(set(rep[:71].tolist())) == 71 and rep[71] == 0 and copies[0] == 2
            assert c.rounds >= rounds_needed(pkg, flags, distinct)
            if not weak:
                assert c.rounds == 1
    finally:
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("weak", [False, True], ids=["strong", "weak"])
@pytest.mark.parametrize("which", ["short", "one item", "three items - 1", "three items + 1"])
def test_one_base_differences(ctx, pkg, dbg, which, weak):
    """a base sequence, one variant each that differs at base 0, 31, 32, the last base and the bases either side of every
    item border, and two exact copies: every variant is a class of its own and the copies join the original.  With the weak
    flag the variants share fingerprints, so the comparison itself -- by items for the long ones -- tells them apart."""
    wave_bases, tile_bases = pkg.seq_equal_geometry()
    flags = dbg | (pkg.DEBUG_WEAK_FINGERPRINT if weak else 0)
    ctx.set_debug(flags)
    n = {"short": 100, "one item": wave_bases + 501, "three items - 1": 3 * tile_bases - 1, "three items + 1": 3 * tile_bases + 1}[which]
    rng = np.random.default_rng(SEED + 300 + n)
    base = random_text(rng, n)
    at = sorted({0, 31, 32, n - 1} | {p for b in range(tile_bases, n, tile_bases) for p in (b - 1, b)})
    texts = [base] + [mutate(base, p) for p in at[:len(at) // 2]] + [base] + [mutate(base, p) for p in at[len(at) // 2:]] + [base]
    d = resident(ctx, texts)
    try:
        with ctx.table_classes(d) as c:
            rep, copies, distinct = check_classes(c, texts, which)
            assert distinct == 1 + len(at) and copies[0] == 3 and sorted(copies.tolist())[:len(at)] == [1] * len(at)
            assert c.rounds >= rounds_needed(pkg, flags, distinct) and (weak or c.rounds == 1)
    finally:
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("weak", [False, True], ids=["strong", "weak"])
def test_mixed_table_with_heavy_duplication(ctx, pkg, dbg, weak):
    """rep, copies and distinct; read windows tile; select for 1 .. max, 2 .. max, 1 .. 1 and min > max, with a cap below
    n_out; members of a singleton, of a large class and of a member that is not the representative; one round (without the
    weak flag)"""
    texts = cached("mixed", mixed_texts, pkg)
    n = len(texts)
    flags = dbg | (pkg.DEBUG_WEAK_FINGERPRINT if weak else 0)
    ctx.set_debug(flags)
    d = resident(ctx, texts)
    try:
        with ctx.table_classes(d) as c:
            rep, copies, distinct = check_classes(c, texts, "mixed")
            assert c.rounds >= rounds_needed(pkg, flags, distinct) and (weak or c.rounds == 1)
            cuts = [0, 1, 700, 2049, 4096, n - 1, n]
            parts = [c.read(a, b - a) for a, b in zip(cuts, cuts[1:])]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), rep)
            assert np.array_equal(np.concatenate([p[1] for p in parts]), copies)
            assert c.read(n, 0)[0].shape == (0,)
            for first, count in ((n + 1, 0), (n - 1, 2)):
                with pytest.raises(pkg.DnaGpuError) as ei:
                    c.read(first, count)
                assert ei.value.code == BAD_ARG
            is_rep = rep == np.arange(n, dtype=np.uint64)
            for lo, hi in ((1, NONE), (0, NONE), (2, NONE), (1, 1), (3, 2), (5, 30)):
                want = np.flatnonzero(is_rep & (copies >= max(lo, 1)) & (copies <= hi)).astype(np.uint64)
                seq, cop, n_out = c.select(lo, hi)
                assert n_out == len(want) and np.array_equal(seq, want) and np.array_equal(cop, copies[want]), (lo, hi)
            want = np.flatnonzero(is_rep).astype(np.uint64)
            assert len(want) == distinct > 40
            seq, cop, n_out = c.select(cap=40)                                # the FIRST cap of the ascending order
            assert n_out == distinct and np.array_equal(seq, want[:40]) and np.array_equal(cop, copies[want[:40]])
            seq, cop, n_out = c.select(cap=40, want=(True, False))
            assert cop is None and np.array_equal(seq, want[:40])
            singles = np.flatnonzero(copies == 1)
            big = int(np.argmax(copies))
            later = int(np.flatnonzero(~is_rep)[-1])
            assert len(singles) and copies[big] > 20
            for s in (int(singles[0]), big, later):
                want = np.flatnonzero(rep == rep[s]).astype(np.uint64)
                ids, n_out = c.members(s)
                assert n_out == len(want) and np.array_equal(ids, want), s
            want = np.flatnonzero(rep == rep[big]).astype(np.uint64)
            ids, n_out = c.members(big, cap=5)
            assert n_out == len(want) and np.array_equal(ids, want[:5])
            with pytest.raises(pkg.DnaGpuError) as ei:
                c.members(n)
            assert ei.value.code == BAD_ARG
    finally:
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2048, 2049])
@pytest.mark.parametrize("last", ["unique", "copy"])
def test_selects_at_the_tile_edge(ctx, pkg, dbg, n, last):
    """select and members over one full select tile and over one entry more -- that entry a representative of its own, or a
    copy of sequence 0 -- in every output form (check_select_forms), with a select of nothing"""
    rng = np.random.default_rng(SEED + 800)
    pool = [random_text(rng, 40) for _ in range(300)]
    texts = [pool[i] for i in rng.integers(0, 300, n)]
    texts[n - 1] = "A" * 41 if last == "unique" else texts[0]
    rep, copies, distinct = ref_classes(texts)
    is_rep = rep == np.arange(n, dtype=np.uint64)
    d = resident(ctx, texts)
    try:
        with ctx.table_classes(d) as c:
            assert c.distinct == distinct

            def select(lo, hi):
                def run(cap, on_device, outs):
                    if on_device:
                        return None, c.select(lo, hi, cap=cap, on_device=True, out=tuple(outs))
                    got = c.select(lo, hi, cap=cap, want=tuple(outs))
                    return got[:2], got[2]
                return run

            for lo, hi in ((1, NONE), (2, NONE), (3, 2)):
                want = np.flatnonzero(is_rep & (copies >= lo) & (copies <= hi)).astype(np.uint64)
                assert (len(want) == 0) == (lo > hi)
                check_select_forms(ctx, select(lo, hi), (want, copies[want]), f"n={n} {last}: select({lo}, {hi})")
            assert (last == "unique") == bool(is_rep[n - 1])

            def members(s):
                def run(cap, on_device, outs):
                    if on_device:
                        return None, c.members(s, cap=cap, on_device=True, out=outs[0])
                    if not outs[0]:
                        n_out = C.c_uint64()
                        assert pkg.lib().dnagpu_seq_classes_members(ctx.h, c.h, s, None, cap, C.byref(n_out), 0) == 0
                        return (None,), n_out.value
                    ids, n_out = c.members(s, cap=cap)
                    return (ids,), n_out
                return run

            for s in (0, n - 1, int(np.argmax(copies))):
                want = np.flatnonzero(rep == rep[s]).astype(np.uint64)
                check_select_forms(ctx, members(s), (want,), f"n={n} {last}: members({s})")
    finally:
        d.free()


def classes_phase_names(c):
    """the phase names dnagpu_last_phase_times reports after dnagpu_table_classes over 20 reads, two of them longer than
    65,536 bases"""
    rng = np.random.default_rng(SEED + 900)
    texts = [random_text(rng, 150) for _ in range(20)]
    texts[3], texts[11] = random_text(rng, 70_000), random_text(rng, 66_000)
    d = resident(c, texts)
    c.set_profiling(True)
    try:
        with c.table_classes(d) as cl:
            names = [name for name, _ in c.last_phase_times()]
            assert cl.distinct == 20
    finally:
        c.set_profiling(False)
        d.free()
    return names


CLASSES_PHASE_NAMES = ["seqeq_fingerprint", "seqeq_sort", "seqeq_verify", "seqeq_copies"]   # (profiles and tools key on these names)


@pytest.mark.gpu
def test_phase_names_of_the_classes(ctx):
    assert classes_phase_names(ctx) == CLASSES_PHASE_NAMES


@pytest.mark.gpu
def test_hot_class(ctx, dbg):
    """one read 20,000 times plus ten singletons: copies is exact"""
    rng = np.random.default_rng(SEED + 400)
    read = random_text(rng, 150)
    texts = [read] * 20_000
    for i in range(10):
        texts.insert(int(rng.integers(0, len(texts))), random_text(rng, 150))
    d = resident(ctx, texts)
    try:
        with ctx.table_classes(d) as c:
            rep, copies, distinct = check_classes(c, texts, "hot class")
            assert distinct == 11 and int(copies.max()) == 20_000 and c.rounds == 1
    finally:
        d.free()


@pytest.mark.gpu
def test_classes_of_nothing_and_of_a_bare_stream(ctx, pkg, dbg):
    """a table of 0 sequences gives a valid object that holds nothing; a stream without a sequence set is BAD_ARG; a table of
    empty sequences only is one class"""
    L = pkg.lib()
    w = np.zeros(1, dtype=np.uint64)
    empty = ctx.upload(w, 0)
    bare = ctx.upload(encode_table(["ACGT"])[0], 4)
    try:
        with ctx.table_classes(empty) as c:
            assert (c.sequences, c.distinct, c.rounds) == (0, 0, 0)
            assert c.select()[2] == 0 and c.read()[0].shape == (0,)
            match, copies, n = c.match(empty)
            assert match.shape == (0,) and n == 0
        out = C.c_void_p(0x1234)
        assert L.dnagpu_table_classes(ctx.h, bare.h, C.byref(out)) == BAD_ARG and out.value == 0x1234
    finally:
        empty.free()
        bare.free()
    texts = ["", "", ""]
    d = resident(ctx, texts)
    try:
        with ctx.table_classes(d) as c:
            check_classes(c, texts, "empty sequences")
            assert c.distinct == 1
    finally:
        d.free()


def match_texts(pkg):
    """a build and a probe of 3,000 sequences each with about half shared, at different alignments on the two sides, and long
    sequences on both: one shared, one of the length of a build sequence that differs in its last base, one in neither"""
    wave_bases, tile_bases = pkg.seq_equal_geometry()
    rng = np.random.default_rng(SEED + 500)
    pool = list(dict.fromkeys(random_text(rng, int(n)) for n in rng.integers(0, 201, 2600)))
    shared, only_b, only_p = pool[:800], pool[800:1600], pool[1600:2400]
    twin = random_text(rng, 2 * tile_bases + 9)
    same_len = [random_text(rng, wave_bases + 40) for _ in range(12)]      # long, one length: candidates of each other's walks
    build = [(shared + only_b)[int(i)] for i in rng.integers(0, 1600, 2992)] + [twin, twin] + same_len[:6]
    probe = [(shared + only_p)[int(i)] for i in rng.integers(0, 1600, 2988)] + [twin, mutate(twin, len(twin) - 1), mutate(same_len[0], 0),
                                                                               random_text(rng, wave_bases + 41)] + same_len[4:]
    build = [build[int(i)] for i in rng.permutation(len(build))]
    probe = [probe[int(i)] for i in rng.permutation(len(probe))]
    return build, probe


def device_match(ctx, c, probe, first, count, pad):
    """the match into device memory, `pad` sentinel cells either side -> (match, copies, n_matched), the pads checked"""
    bufs = [ctx.buffer_alloc(8 * (count + 2 * pad + 1)) for _ in range(2)]
    try:
        for b in bufs:
            ctx.upload_u64(b, np.full(count + 2 * pad, SENTINEL, dtype=np.uint64))
        n = c.match(probe, first, count, on_device=True, out=(bufs[0] + 8 * pad, bufs[1] + 8 * pad))
        got = [ctx.download_u64(b, count + 2 * pad) for b in bufs]
    finally:
        for b in bufs:
            ctx.buffer_free(b)
    for a in got:
        assert (a[:pad] == SENTINEL).all() and (a[pad + count:] == SENTINEL).all()
    return got[0][pad:pad + count], got[1][pad:pad + count], n


@pytest.mark.gpu
@pytest.mark.parametrize("weak", [False, True], ids=["strong", "weak"])
def test_match(ctx, pkg, dbg, weak):
    """match, copies and n_matched; probe windows tile and leave the cells outside a window alone; device outputs equal host
    outputs; the built table as its own probe gives rep / copies; a probe of one sequence; an empty build and an empty
    probe; long sequences on both sides; the argument rules"""
    L = pkg.lib()
    build, probe = cached("match", match_texts, pkg)
    want_match, want_copies, want_n = ref_match(probe, build)
    assert 1000 < want_n < 2000
    n = len(probe)
    ctx.set_debug(dbg | (pkg.DEBUG_WEAK_FINGERPRINT if weak else 0))
    db, dp = resident(ctx, build), resident(ctx, probe)
    try:
        with ctx.table_classes(db) as c:
            check_classes(c, build, "build")
            match, copies, n_matched = c.match(dp)
            bad = np.flatnonzero((match != want_match) | (copies != want_copies))
            assert not len(bad), f"probe {bad[:5]}: {match[bad[:5]]} / {want_match[bad[:5]]}"
            assert n_matched == want_n
            cuts = [0, 1, 33, 1500, n - 1, n]
            total = 0
            for a, b in zip(cuts, cuts[1:]):
                m, cp, k = c.match(dp, a, b - a)
                assert np.array_equal(m, want_match[a:b]) and np.array_equal(cp, want_copies[a:b])
                dm, dc, dk = device_match(ctx, c, dp, a, b - a, 3)
                assert np.array_equal(dm, m) and np.array_equal(dc, cp) and dk == k
                total += k
            assert total == want_n
            rep, cop, _ = ref_classes(build)
            m, cp, k = c.match(db)
            assert np.array_equal(m, rep) and np.array_equal(cp, cop) and k == len(build)
            for text in (probe[0], build[5], "ACGTT" * 9):                    # WHERE sequence = $1
                one = resident(ctx, [text])
                try:
                    m, cp, k = c.match(one)
                    wm, wc, wk = ref_match([text], build)
                    assert np.array_equal(m, wm) and np.array_equal(cp, wc) and k == wk
                finally:
                    one.free()
            assert c.match(dp, 7, 0)[2] == 0 and c.match(dp, n, 0)[2] == 0
            none = ctx.upload(np.zeros(1, dtype=np.uint64), 0)                # an empty probe table
            try:
                m, cp, k = c.match(none)
                assert m.shape == (0,) and cp.shape == (0,) and k == 0
            finally:
                none.free()
            # only n_matched; only one of the arrays
            k = C.c_uint64()
            assert L.dnagpu_table_match(ctx.h, c.h, dp.h, 0, n, None, None, C.byref(k), 0) == 0 and k.value == want_n
            only = np.full(n + 2, SENTINEL, dtype=np.uint64)
            assert L.dnagpu_table_match(ctx.h, c.h, dp.h, 0, n, None, only[1:].ctypes.data, None, 0) == 0
            assert only[0] == SENTINEL and only[-1] == SENTINEL and np.array_equal(only[1:-1], want_copies)
            # errors write nothing
            host = np.full(n, SENTINEL, dtype=np.uint64)
            bare = ctx.upload(encode_table(["ACGT"])[0], 4)
            try:
                for pr, first, count in ((dp, n + 1, 0), (dp, n - 1, 2), (dp, 0, n + 1), (bare, 0, 1)):
                    assert L.dnagpu_table_match(ctx.h, c.h, pr.h, first, count, host.ctypes.data, host.ctypes.data, C.byref(k), 0) == BAD_ARG
                assert L.dnagpu_table_match(ctx.h, c.h, dp.h, 0, n, None, None, None, 0) == BAD_ARG
                assert L.dnagpu_table_match(ctx.h, c.h, dp.h, 0, 0, None, None, None, 0) == 0
                assert L.dnagpu_table_match(ctx.h, None, dp.h, 0, n, host.ctypes.data, None, None, 0) == BAD_ARG
            finally:
                bare.free()
            assert (host == SENTINEL).all()
        empty = ctx.upload(np.zeros(1, dtype=np.uint64), 0)
        try:
            with ctx.table_classes(empty) as c0:                              # an empty build matches nothing
                m, cp, k = c0.match(dp)
                assert (m == np.uint64(NONE)).all() and not cp.any() and k == 0
                dm, dc, dk = device_match(ctx, c0, dp, 3, 10, 2)
                assert (dm == np.uint64(NONE)).all() and not dc.any() and dk == 0
        finally:
            empty.free()
    finally:
        db.free()
        dp.free()


@pytest.mark.gpu
def test_select_feeds_take(ctx, pkg, dbg):
    """the distinct reads as a new resident table: select's device output goes straight into dnagpu_dna_take; the result
    holds every content once, in ascending id of its first copy, and its own classes are all singletons"""
    texts = cached("mixed", mixed_texts, pkg)
    rep, copies, distinct = ref_classes(texts)
    want_ids = np.flatnonzero(rep == np.arange(len(texts), dtype=np.uint64))
    d = resident(ctx, texts)
    ids = ctx.buffer_alloc(8 * distinct)
    try:
        with ctx.table_classes(d) as c:
            n_out = c.select(cap=distinct, on_device=True, out=(ids, None))
            assert n_out == distinct and np.array_equal(ctx.download_u64(ids, distinct), want_ids.astype(np.uint64))
        taken = ctx.dna_take_device(d, ids, distinct)
        try:
            starts = taken.sequence_starts()
            whole = ctx.unpack(taken)
            got = [whole[int(a):int(b)] for a, b in zip(starts, starts[1:])]
            assert got == [texts[int(i)] for i in want_ids]
            with ctx.table_classes(taken) as c2:
                assert c2.distinct == distinct and c2.select(2)[2] == 0
                m, cp, k = c2.match(d)                                        # every read of the table finds its content
                assert k == len(texts) and np.array_equal(cp, np.ones(len(texts), dtype=np.uint64))
                assert [got[int(i)] for i in m] == texts
        finally:
            taken.free()
    finally:
        ctx.buffer_free(ids)
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
def test_glue_table_distinct_and_match(g, pkg, dbg):
    """table_distinct yields the representatives in ascending ordinal of the add call with their copies; table_match the
    matched probe rows only; empty rows are rows like any other; an empty side gives no row"""
    rng = np.random.default_rng(SEED + 600)
    pool = [random_text(rng, int(n)) for n in rng.integers(1, 120, 40)] + [""]
    texts = [pool[int(i)] for i in rng.integers(0, len(pool), 400)] + ["", random_text(rng, 3000)]
    rows = [t if t else EmptyRow() for t in texts]
    rep, copies, distinct = ref_classes(texts)
    want = np.flatnonzero(rep == np.arange(len(texts), dtype=np.uint64))
    seq, cop = g.table_distinct(rows)
    assert np.array_equal(seq, want.astype(np.int64)) and np.array_equal(cop, copies[want].astype(np.int64))
    seq, cop = g.table_distinct([])
    assert seq.shape == (0,) and cop.shape == (0,)
    seq, cop = g.table_distinct([EmptyRow(), EmptyRow()])
    assert seq.tolist() == [0] and cop.tolist() == [2]
    probe = [random_text(rng, 50), texts[3], "", texts[-1], texts[-1][:-1], texts[10]]
    wm, wc, _ = ref_match(probe, texts)
    hit = np.flatnonzero(wm != np.uint64(NONE))
    ps, bs, cp = g.table_match([t if t else EmptyRow() for t in probe], rows)
    assert np.array_equal(ps, hit.astype(np.int64)) and np.array_equal(bs, wm[hit].astype(np.int64))
    assert np.array_equal(cp, wc[hit].astype(np.int64))
    for pr, bu in (([], rows), (probe[:2], [])):
        ps, bs, cp = g.table_match(pr, bu)
        assert ps.shape == (0,) and bs.shape == (0,) and cp.shape == (0,)
