"""dnagpu_generate_kmers_table: the ROWS of a table of sequences -- FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k)
AS k(kmer) [WHERE <op>] (test.sql:140-150, 172-176, 187-262) -- through the C-ABI, the binding and the glue's table_kmers_*.

Expected rows come from the CPU oracle alone: orc.generate_kmers over the packed stream gives the stream keys, the
in-one-sequence rule is numpy (seq = searchsorted(starts, p, 'right') - 1; valid = p + k <= starts[seq + 1]),
orc.generate_kmers_table checks that rule independently, and the oracle's filtered stream forms give the matching positions,
kept where valid.  Every comparison is exact: keys, seq, pos, n_out."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import load_package

BAD_ARG, QKMER_LEN_MISMATCH, PREFIX_TOO_LONG = 5, 2, 3
TILE = 8192
SENTINEL = 0xC3
PATTERN21 = "NNNNNNNNNNWSNNNNNNNNN"


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def glue(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


@pytest.fixture(scope="module")
def _ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture
def ctx(_ctx):
    yield _ctx
    _ctx.synchronize()                            # (under DNAGPU_TEST_GUARD=1: raises if a kernel wrote past a pooled buffer)


# ------------------------------------------------------------------ CPU: the new surface exists and checks its arguments

def test_symbol_null_arguments(pkg):
    L = C.CDLL(pkg.lib_path())
    L.dnagpu_generate_kmers_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    n = C.c_uint64(77)
    assert L.dnagpu_generate_kmers_table(None, None, 21, None, 0, 0, None, None, None, 0, C.byref(n), 0) == BAD_ARG
    assert pkg.abi_version() == 2


def test_binding_and_glue_surface(pkg, glue):
    assert callable(pkg.Context.generate_kmers_table) and callable(pkg.Context.generate_kmers_table_device)
    for name in ("table_kmers_begin", "table_kmers_add", "table_kmers_next", "table_kmers_failed", "table_kmers_end"):
        assert hasattr(glue.lib(), name), name
    assert callable(glue.table_kmers)


@pytest.mark.parametrize("k", [0, 33])
def test_glue_begin_bad_k(glue, k):
    assert not glue.lib().table_kmers_begin(k, b"\0", None, None)
    assert glue.lib().dna_glue_errmsg().decode() == "Invalid k value: must be between 1 and 32"      # dna.c:773
    with pytest.raises(glue.GlueError) as ei:
        glue.table_kmers(["ACGT"], k)
    assert str(ei.value) == "Invalid k value: must be between 1 and 32"


# ------------------------------------------------------------------ expected rows, from the oracle

class Table:
    """a packed stream cut into sequences: words, n bases, starts[0 .. n_seqs]"""

    def __init__(self, words, n, lengths):
        self.words, self.n = words, int(n)
        self.starts = np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.int64)
        assert self.starts[-1] == self.n
        self._rows = {}

    @classmethod
    def synth(cls, seed, lengths, motif=0):
        n = int(np.sum(lengths))
        words = orc.synth_words_repeat(seed, n, motif) if motif else orc.synth_words(seed, n)
        return cls(words, n, lengths)

    @classmethod
    def of_texts(cls, texts):
        words, n = orc.dna_encode("".join(texts))
        return cls(words, n, [len(t) for t in texts])

    def rows(self, k):
        """(stream keys, seq of every stream row, valid) -- computed once per k"""
        if k not in self._rows:
            allk = orc.generate_kmers(self.words, self.n, k, faithful=False)
            p = np.arange(len(allk), dtype=np.int64)
            seq = np.searchsorted(self.starts, p, "right") - 1
            valid = p + k <= self.starts[seq + 1]
            # the independent check of the numpy rule
            assert np.array_equal(allk[valid], orc.generate_kmers_table(self.words, self.starts, k))
            self._rows[k] = (allk, seq, valid)
        return self._rows[k]

    def matching(self, k, spec):
        """bool per stream row: the oracle's filtered stream form"""
        allk = self.rows(k)[0]
        m = np.ones(len(allk), dtype=bool)
        if spec is not None:
            kind, a, b = spec
            if kind == "contains":
                _, pos = orc.generate_kmers_contains(self.words, self.n, k, a)
            elif kind == "starts_with":
                _, pos = orc.generate_kmers_starts_with(self.words, self.n, k, a, b)
            else:
                _, pos = orc.generate_kmers_equals(self.words, self.n, k, a, b)
            m[:] = False
            m[pos.astype(np.int64)] = True
        return m

    def expected(self, k, spec=None, first=0, count=None, match=None):
        allk, seq, valid = self.rows(k)
        if count is None:
            count = len(allk) - first
        sel = valid & (self.matching(k, spec) if match is None else match)
        sel[:first] = False
        sel[first + count:] = False
        p = np.flatnonzero(sel)
        return allk[p], seq[p].astype(np.uint64), (p - self.starts[seq[p]]).astype(np.uint64)

    def upload(self, ctx):
        d = ctx.upload(self.words, self.n)
        d.set_sequences(self.starts.astype(np.uint64))
        return d


def make_filter(pkg, spec):
    if spec is None:
        return None
    kind, a, b = spec
    if kind == "contains":
        return pkg.Filter.contains(a)
    return pkg.Filter.starts_with(a, b) if kind == "starts_with" else pkg.Filter.equals(a, b)


def assert_rows(got, want, what):
    gk, gs, gp, n = got
    wk, ws, wp = want
    assert n == len(wk), f"{what}: n_out = {n}, oracle {len(wk)}"
    for name, g, w in (("keys", gk, wk), ("seq", gs, ws), ("pos", gp, wp)):
        if g is None:
            continue
        assert len(g) == len(w), f"{what}: {len(g)} {name}, oracle {len(w)}"
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{what}: {name} differ first at row {at}: got {g[at]} want {w[at]}")


def specs_for(t, k, pick):
    """no filter and one filter of each kind; `=` asks for the key of a table row"""
    allk, _, valid = t.rows(k)
    q = int(allk[np.flatnonzero(valid)[pick]])
    pat = "N" * (k // 2) + "W" + "N" * (k - k // 2 - 1)
    ln, bits = orc.kmer_encode("G")
    return [None, ("contains", pat, None), ("starts_with", ln, bits), ("equals", k, q)]


# ------------------------------------------------------------------ 1. the reference's own vectors

REF_TABLE = ["ATCGATCGATCGATCGACG", "ACGTACGCACGT", "ACTGACGTACC", "ATCGTAGCGT"]


def ref_checks(run):
    """run(k, op, rhs text) -> (keys, seq, pos); the statements of test.sql:46-92 asked of a table of its literals"""
    for k in (3, 5, 6):
        keys, seq, pos = run(k, None, None)
        for s, text in enumerate(REF_TABLE):
            w, n = orc.dna_encode(text)
            own = orc.generate_kmers(w, n, k, faithful=False)
            assert np.array_equal(keys[seq == s], own), f"k={k} sequence {s}"
            assert np.array_equal(pos[seq == s], np.arange(len(own))), f"k={k} sequence {s}"
    keys, seq, pos = run(3, "^@", "AC")                                       # test.sql:67-73
    assert list(pos[seq == 2]) == [0, 4, 8]
    assert all(orc.kmer_decode(x, 3).startswith("AC") for x in keys)
    keys, seq, pos = run(6, "@>", "DNMSRN")                                   # test.sql:86-92
    assert [orc.kmer_decode(x, 6) for x in keys[seq == 1]] == ["GTACGC", "GCACGT"]
    keys, seq, pos = run(6, "=", "ACGTAC")                                    # test.sql:61-65
    # the statement's literal is sequence 1, where it finds its one row; over the table 'ACTGACGTACC' holds the k-mer too
    want = [(s, p) for s, text in enumerate(REF_TABLE) for p in range(len(text) - 5) if text[p:p + 6] == "ACGTAC"]
    assert want == [(1, 0), (2, 4)]
    assert [orc.kmer_decode(x, 6) for x in keys] == ["ACGTAC"] * 2 and list(zip(seq, pos)) == want


def spec_of(op, rhs):
    if op is None:
        return None
    if op == "@>":
        return ("contains", rhs, None)
    ln, bits = orc.kmer_encode(rhs)
    return ("starts_with" if op == "^@" else "equals", ln, bits)


@pytest.mark.gpu
def test_reference_vectors(ctx, pkg):
    t = Table.of_texts(REF_TABLE)
    d = t.upload(ctx)

    def run(k, op, rhs):
        spec = spec_of(op, rhs)
        got = ctx.generate_kmers_table(d, k, make_filter(pkg, spec))
        assert_rows(got, t.expected(k, spec), f"reference table k={k} {op} {rhs}")
        return got[:3]
    ref_checks(run)
    d.free()


@pytest.mark.gpu
def test_reference_vectors_glue(glue):
    t = Table.of_texts(REF_TABLE)

    def run(k, op, rhs):
        r = None if op is None else (glue.qkmer(rhs) if op == "@>" else glue.kmer(rhs))
        seq, pos, keys = glue.table_kmers(REF_TABLE, k, op, r)
        wk, ws, wp = t.expected(k, spec_of(op, rhs))
        assert np.array_equal(keys, wk) and np.array_equal(seq, ws.astype(np.int64)) and np.array_equal(pos, wp.astype(np.int64))
        return keys, seq, pos
    ref_checks(run)


# ------------------------------------------------------------------ 2. edges of the mask

def edge_lengths(k):
    rng = np.random.default_rng(0x7AB1E)
    return [0, 0, 1, k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 150, 0, 8191, 8192, 8193, 0, 150, 20, 20, 21, 0] + \
        [int(x) for x in rng.integers(0, 300, 400)]


_edge_tables = {}


def edge_table(k, data):
    if (k, data) not in _edge_tables:
        _edge_tables[(k, data)] = Table.synth(0xED6E + k, edge_lengths(k), motif=0 if data == "uniform" else 64)
    return _edge_tables[(k, data)]


@pytest.mark.gpu
@pytest.mark.parametrize("data", ["uniform", "repeat"])
@pytest.mark.parametrize("k", [1, 2, 5, 21, 31, 32])
def test_mask_edges(ctx, pkg, k, data):
    """sequences of every length around k, around the 32 rows of a thread and around the 8192 rows of a tile, empty ones and
    runs of them; uniform data and a repeat-rich stream whose `=` and `@>` matches are dense"""
    t = edge_table(k, data)
    d = t.upload(ctx)
    for spec in specs_for(t, k, -7):               # (a row of the repeat-rich half)
        want = t.expected(k, spec)
        if spec is not None and data == "repeat":
            assert len(want[0]) > 50
        assert_rows(ctx.generate_kmers_table(d, k, make_filter(pkg, spec)), want, f"edges k={k} {data} {spec}")
    d.free()


# ------------------------------------------------------------------ 3. windows

@pytest.mark.gpu
@pytest.mark.parametrize("first", [0, 7])
@pytest.mark.parametrize("filtered", [False, True])
def test_windows_concatenate(ctx, pkg, first, filtered):
    k = 21
    t = edge_table(k, "uniform")
    spec = ("contains", PATTERN21, None) if filtered else None
    flt = make_filter(pkg, spec)
    match = t.matching(k, spec)
    d = t.upload(ctx)
    rows = t.n - k + 1
    whole = ctx.generate_kmers_table(d, k, flt, first=first)
    assert_rows(whole, t.expected(k, first=first, match=match), f"whole from {first}")
    parts, at = [], first
    for size in (1, 31, 32, 33, 8191, 8193, None):
        n = rows - at if size is None else size
        got = ctx.generate_kmers_table(d, k, flt, first=at, count=n)
        assert_rows(got, t.expected(k, first=at, count=n, match=match), f"window [{at}, +{n})")
        parts.append(got)
        at += n
    for i in range(3):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), whole[i])
    assert sum(p[3] for p in parts) == whole[3]
    # a window that starts and ends inside one sequence (the one of 8193 bases)
    s = edge_lengths(k).index(8193)
    a = int(t.starts[s]) + 100
    got = ctx.generate_kmers_table(d, k, flt, first=a, count=5000)
    assert_rows(got, t.expected(k, first=a, count=5000, match=match), "window inside a sequence")
    assert np.all(got[1] == s) and (filtered or got[3] == 5000)
    d.free()


@pytest.mark.gpu
def test_operator_errors_need_a_table_row(ctx, pkg):
    """a window whose stream rows all span boundaries evaluates no operator: 0 rows and no ERROR, whatever the pattern's length;
    one table row in the window and the reference's ERROR is raised (dna.c:1106-1108, 854-856)"""
    k = 21
    lengths = edge_lengths(k)
    t = edge_table(k, "uniform")
    d = t.upload(ctx)
    s = next(i for i in range(len(lengths)) if lengths[i:i + 3] == [20, 20, 21])      # (k - 1 = 20 comes earlier, on its own)
    a = int(t.starts[s])
    bad = [(pkg.Filter.contains("ACG"), QKMER_LEN_MISMATCH), (pkg.Filter.starts_with(22, 0), PREFIX_TOO_LONG)]
    assert not t.rows(k)[2][a:a + 40].any() and t.rows(k)[2][a + 40]
    for flt, code in bad:
        got = ctx.generate_kmers_table(d, k, flt, first=a, count=40)
        assert got[3] == 0 and len(got[0]) == 0
        assert ctx.generate_kmers_table(d, k, flt, first=a, count=0)[3] == 0
        with pytest.raises(pkg.DnaGpuError) as ei:
            ctx.generate_kmers_table(d, k, flt, first=a, count=41)
        assert ei.value.code == code
    # a malformed filter is an error with or without rows
    for count in (40, 41):
        with pytest.raises(pkg.DnaGpuError):
            ctx.generate_kmers_table(d, k, pkg.Filter.contains("AZG"), first=a, count=count)
    # `=` of another length matches nothing; 'U' matches nothing
    assert ctx.generate_kmers_table(d, k, pkg.Filter.equals(20, 5))[3] == 0
    assert ctx.generate_kmers_table(d, k, pkg.Filter.contains("U" + "N" * 20))[3] == 0
    with pytest.raises(pkg.DnaGpuError) as ei:
        ctx.generate_kmers_table(d, k, None, first=t.n - k + 1, count=1)
    assert ei.value.code == BAD_ARG
    d.free()


# ------------------------------------------------------------------ 4. the bounded search

def check_all_forms(ctx, pkg, t, k, what, specs):
    d = t.upload(ctx)
    for spec in specs:
        assert_rows(ctx.generate_kmers_table(d, k, make_filter(pkg, spec)), t.expected(k, spec), f"{what} k={k} {spec}")
    d.free()


@pytest.mark.gpu
def test_search_every_row_its_own_sequence(ctx, pkg):
    """10,000 sequences of one base at k = 1: a tile holds 8192 sequences, far more than the starts it keeps in LDS"""
    t = Table.synth(0x5EA1, [1] * 10_000)
    check_all_forms(ctx, pkg, t, 1, "one base per sequence", [None, ("contains", "S", None)])
    # ... and with runs of empty sequences between them
    rng = np.random.default_rng(5)
    t = Table.synth(0x5EA2, [int(x) for x in rng.integers(0, 3, 30_000)])
    check_all_forms(ctx, pkg, t, 1, "0..2 bases per sequence", [None, ("contains", "S", None)])
    check_all_forms(ctx, pkg, t, 2, "0..2 bases per sequence", [None])


@pytest.mark.gpu
def test_search_tile_inside_one_sequence(ctx, pkg):
    t = Table.synth(0x5EA3, [150, 3 * TILE + 5, 150])
    check_all_forms(ctx, pkg, t, 21, "a tile-long sequence", [None, ("contains", PATTERN21, None)])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31])
def test_search_reads(ctx, pkg, k):
    t = Table.synth(0x5EA4, [150] * 20_000)
    pat = PATTERN21 + "N" * (k - 21)
    check_all_forms(ctx, pkg, t, k, "20,000 reads", [None, ("contains", pat, None)])


# ------------------------------------------------------------------ 5. a table of one sequence

@pytest.mark.gpu
def test_one_sequence_equals_the_single_sequence_call(ctx, pkg):
    n, k = 70_001, 21
    t = Table.synth(0x0E5E, [n])
    d = t.upload(ctx)
    flt = pkg.Filter.contains(PATTERN21)
    for first, count in ((0, None), (33, 50_000)):
        fk, fp, ftot = ctx.generate_kmers_filtered(d, k, flt, first=first, count=count)
        gk, gs, gp, tot = ctx.generate_kmers_table(d, k, flt, first=first, count=count)
        assert tot == ftot > 1000
        assert np.array_equal(gk, fk) and np.array_equal(gp, fp) and not gs.any()
    d.free()


# ------------------------------------------------------------------ 6. outputs

@pytest.mark.gpu
def test_caps_and_single_arrays(ctx, pkg):
    k = 21
    t = edge_table(k, "uniform")
    d = t.upload(ctx)
    before = ctx.count_kmers_table(d, k)
    spec = ("contains", PATTERN21, None)
    flt = make_filter(pkg, spec)
    wk, ws, wp = t.expected(k, spec)
    total = len(wk)
    assert total > 1000
    for cap in (0, 1, 1000, 1001, total - 1):         # (1001: the last slot is the first half of a 16-byte pair)
        gk, gs, gp, n = ctx.generate_kmers_table(d, k, flt, cap=cap)
        assert n == total
        assert np.array_equal(gk, wk[:cap]) and np.array_equal(gs, ws[:cap]) and np.array_equal(gp, wp[:cap])
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
        got = ctx.generate_kmers_table(d, k, flt, want_keys=want[0], want_seq=want[1], want_pos=want[2])
        assert got[3] == total
        for g, w, asked in zip(got[:3], (wk, ws, wp), want):
            assert (g is None) if not asked else np.array_equal(g, w)
    # the table is left as it was
    after = ctx.count_kmers_table(d, k)
    assert after.summary() == before.summary()
    assert after.summary()[0] == int(t.rows(k)[2].sum())
    for h in (before, after):
        h.free()
    d.free()
    # a stream without a sequence set
    plain = ctx.upload(t.words, t.n)
    with pytest.raises(pkg.DnaGpuError) as ei:
        ctx.generate_kmers_table(plain, k, flt)
    assert ei.value.code == BAD_ARG
    plain.free()


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [True, False])
def test_device_outputs_every_parity(ctx, pkg, filtered):
    """out_on_device: the three arrays at every combination of 8-byte parity, alone and together, into sentinel-filled memory:
    nothing but the first min(n_out, cap) slots of each array changes"""
    k = 21
    t = edge_table(k, "uniform")
    d = t.upload(ctx)
    spec = ("contains", PATTERN21, None) if filtered else None
    flt = make_filter(pkg, spec)
    want = t.expected(k, spec)
    total = len(want[0])
    room = (total + 64) * 8                        # bytes per array: sentinel words behind every cap
    stride = (room + 4096 + 255) & ~255
    size = 3 * stride + 4096
    base = ctx.buffer_alloc(size)
    assert base % 256 == 0
    clean = np.full(size, SENTINEL, dtype=np.uint8)
    places = [(a, b, c) for a in (0, 8) for b in (0, 8) for c in (0, 8)] + \
        [(0, None, None), (None, 8, None), (None, None, 0), (8, None, 0), (None, 0, 8), (8, 0, None)]
    for cap in (total + 7, 1001):
        for offs in places:
            ctx.upload_bytes(base, clean)
            img = clean.copy()
            ptrs = []
            for i, off in enumerate(offs):
                if off is None:
                    ptrs.append(None)
                    continue
                at = 2048 + i * stride + off
                ptrs.append(C.c_void_p(base + at))
                w = want[i][:min(cap, total)]
                img[at:at + 8 * len(w)] = w.view(np.uint8)
            n = ctx.generate_kmers_table_device(d, k, flt, 0, t.n - k + 1, ptrs[0], ptrs[1], ptrs[2], cap)
            assert n == total
            got = ctx.download_bytes(base, size)
            if not np.array_equal(got, img):
                at = int(np.flatnonzero(got != img)[0])
                raise AssertionError(f"arrays at +{offs} cap={cap}: byte {at} (array {at // stride}, slot {(at % stride - 2048) // 8})")
    ctx.buffer_free(base)
    d.free()


# ------------------------------------------------------------------ 7. more than one tile per workgroup

@pytest.mark.gpu
def test_two_tiles_per_workgroup(ctx, pkg):
    """67,108,864 + 3 x 8192 + 17 stream rows: two tiles per workgroup, so the bounds of a tile are carried into the next"""
    k = 21
    rows = 67_108_864 + 3 * TILE + 17
    n = rows + k - 1
    lengths = [150] * (n // 150) + ([n % 150] if n % 150 else [])
    starts = np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64))))
    words = orc.synth_words(0xD2A0001, n)
    _, pos = orc.generate_kmers_contains(words, n, k, PATTERN21)
    allk = orc.generate_kmers(words, n, k, faithful=False)
    p = pos.astype(np.int64)
    seq = np.searchsorted(starts, p, "right") - 1
    p = p[p + k <= starts[seq + 1]]
    wk = allk[p]
    wp = (p - starts[np.searchsorted(starts, p, "right") - 1]).astype(np.uint64)
    del allk, pos, seq
    d = ctx.upload(words, n)
    d.set_sequences(starts.astype(np.uint64))
    gk, gs, gp, tot = ctx.generate_kmers_table(d, k, pkg.Filter.contains(PATTERN21), want_seq=False)
    d.free()
    assert tot == len(wk) and gs is None
    assert np.array_equal(gp, wp)
    assert np.array_equal(gk, wk)


# ------------------------------------------------------------------ 8. the glue

@pytest.mark.gpu
def test_glue_batches(glue):
    """300 rows under a flush size of 1,000 bases: dozens of batches, a row longer than a batch; seq runs on across batches"""
    k = 5
    rng = np.random.default_rng(0x61CE)
    lengths = [int(x) for x in rng.integers(1, 121, 300)]
    lengths[57] = 2500
    lengths[58] = 3                                # shorter than k
    t = Table.synth(0x61CF, lengths)
    text = orc.dna_decode(t.words, t.n)
    rows = [text[a:b] for a, b in zip(t.starts[:-1], t.starts[1:])]
    allk, _, valid = t.rows(k)
    q = orc.kmer_decode(int(allk[np.flatnonzero(valid)[1000]]), k)
    glue.set_agg_flush_bases(1000)
    try:
        for op, rhs in ((None, None), ("@>", "NNWSN"), ("^@", "GA"), ("=", q)):
            r = None if op is None else (glue.qkmer(rhs) if op == "@>" else glue.kmer(rhs))
            seq, pos, keys = glue.table_kmers(rows, k, op, r)
            wk, ws, wp = t.expected(k, spec_of(op, rhs))
            assert len(wk) > 0
            assert np.array_equal(keys, wk), op
            assert np.array_equal(seq, ws.astype(np.int64)), op
            assert np.array_equal(pos, wp.astype(np.int64)), op
            if op is None:
                assert set(seq) == {i for i, n in enumerate(lengths) if n >= k}
        # the operator ERRORs come with the first row
        for op, r, msg in (("@>", glue.qkmer("ACG"), "Qkmer pattern and kmer lengths do not match"),
                           ("^@", glue.kmer("ACGTAC"), "Prefix length cannot exceed kmer length")):
            with pytest.raises(glue.GlueError) as ei:
                glue.table_kmers(rows, k, op, r)
            assert str(ei.value) == msg
            # ... and a table without a single row of k bases evaluates nothing
            seq, pos, keys = glue.table_kmers(["ACG", "T", "ACGT"], k, op, r)
            assert len(seq) == len(pos) == len(keys) == 0
        seq, pos, keys = glue.table_kmers([], k)
        assert len(keys) == 0
        # rows may not be added once the scan has started
        L = glue.lib()
        tk = L.table_kmers_begin(k, b"\0", None, None)
        one = glue.dna("ACGTACGT")
        assert L.table_kmers_add(tk, one.p)
        km, sq, ps = glue._Kmer(), C.c_int64(), C.c_int64()
        assert L.table_kmers_next(tk, C.byref(sq), C.byref(ps), C.byref(km)) and (sq.value, ps.value) == (0, 0)
        assert not L.table_kmers_add(tk, one.p)
        L.table_kmers_end(tk)
    finally:
        glue.set_agg_flush_bases(1 << 30)
