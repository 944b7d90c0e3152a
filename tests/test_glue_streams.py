"""The streaming objects of the glue (glue/) at the level of the shape they share: the life cycle (rows in, a last flush on
the first _next, rows out), the same rows whatever the batch or chunk size, an object that saw no row, the three forms of a
filter, and the input errors that the loaders hand on.  Every object is driven call by call through glue.lib(), since
glue.py's generators hide the state machine.  The texts of the refusals are literals copied from the glue's source."""
import ctypes as C
import importlib

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

K = 3
SEED = 20240611
DEFAULT_FLUSH = 1 << 30
DEFAULT_CHUNK = 64 << 20
# rows without a base, a batch of them only (the first two, before a row that spills at 1 and at 64), rows longer than a
# batch of 64 (200, 65), and every length around k and around a word
LENGTHS = [0, 0, 200, 1, K - 1, K, 31, 32, 33, 64, 65, 0, 1, 200, 0, 0, K, 33, 65, 64, 31, K - 1, 32, 0]
MSG_QUAL_LENGTH = "FASTQ quality line length differs from the sequence's"

REFUSALS = {
    "count_kmers_table_agg": "count_kmers_agg: row added after the aggregate finished or failed",
    "table_kmers": "table_kmers: row added after the first row was served or the scan failed",
    "table_hits": "table_hits: row added after the first row was served or the scan failed",
    "table_profile": "table_profile: row added after the first row was served or the scan failed",
    "table_screen": "table_screen: row added after the first row was served or the scan failed",
    "table_distinct": "table_distinct: row added after the first row was served or the scan failed",
    "table_match": "table_match: row added after the first row was served or the scan failed",
    "copy_dna": "copy_dna: bytes fed after the last ones or after the load failed",
    "copy_reads": "copy_dna: bytes fed after the last ones or after the load failed",
    "trim_reads": "copy_dna: bytes fed after the last ones or after the load failed",
    "copy_dna_to": "copy_dna_to: a row added after the last one or after the COPY failed",
    "copy_reads_to": "copy_reads_to: a row added after the last one or after the COPY failed",
}
MSG_AGG_ORDER = "count_kmers_agg_order: called after the first row was served or the aggregate failed"
MSG_AGG_TOP = "count_kmers_agg_top: called after the first row was served or the aggregate failed"
COPY_OBJECTS = ("copy_dna", "copy_reads", "trim_reads", "copy_dna_to", "copy_reads_to")
OBJECTS = tuple(REFUSALS)


@pytest.fixture(scope="module")
def g():
    pkg = load_package()
    return importlib.import_module(pkg.__name__ + ".glue")


class EmptyRow:
    """a row of no bases as the glue's C interface takes it (glue/dna_glue.h: struct Dna); dna_in refuses one"""

    class _Dna(C.Structure):
        _fields_ = [("length", C.c_uint64), ("bit_sequence", C.c_void_p), ("dev", C.c_void_p)]

    def __init__(self):
        self._row = self._Dna(0, None, None)
        self.p = C.addressof(self._row)


def random_texts(lengths, seed):
    rng = np.random.default_rng(seed)
    return ["".join("ATCG"[c] for c in rng.integers(0, 4, n)) for n in lengths]


@pytest.fixture(scope="module")
def data(g):
    """the inputs, made once: the table's rows (with repeats, for the equal-row objects), the same as values, the rows of the
    counted set, a text of lines and a FASTQ text of the rows that have a base"""
    texts = random_texts(LENGTHS, SEED)
    texts[13] = texts[2]                                                  # equal rows of 200, 65 and 3 bases
    texts[18] = texts[10]
    texts[16] = texts[5]
    rows = [g.dna(t) if t else EmptyRow() for t in texts]
    full = [t for t in texts if t]
    quals = ["".join(chr(33 + (7 * i + 3 * j) % 40) for j in range(len(t))) for i, t in enumerate(texts)]
    lines = "".join(t + "\n" for t in full).encode()
    fastq = "".join(f"@r{i}\n{t}\n+\n{q}\n" for i, (t, q) in enumerate(zip(texts, quals)) if t).encode()
    return dict(texts=texts, rows=rows, set_rows=texts[2:8], quals=[q.encode() for q in quals], lines=lines, fastq=fastq)


class Stream:
    """one streaming object, call by call: add(item) -> bool, finish() -> bool (the objects that have one), next() -> a row or
    None, failed(), end().  items() = what the object is fed: rows, or the pieces of a file."""

    def __init__(self, g, name, data):
        self.g, self.L, self.name, self.data = g, g.lib(), name, data
        self.set = None
        L = self.L
        if name == "count_kmers_table_agg":
            self.h = L.count_kmers_agg_begin(K)
        elif name == "table_kmers":
            self.h = L.table_kmers_begin(K, b"\0", None, None)
        elif name in ("table_hits", "table_screen"):
            self.set = g.count_kmers_table_agg(K, rows=data["set_rows"])
            self.h = (L.table_hits_begin(self.set.a, False, 1, -1) if name == "table_hits" else
                      L.table_screen_begin(self.set.a, False, 1, -1, 0, -1, 0, 1))
        elif name == "table_profile":
            self.h = L.table_profile_begin(K, False)
        elif name == "table_distinct":
            self.h = L.table_distinct_begin()
        elif name == "table_match":
            self.h = L.table_match_begin()
        elif name == "copy_dna":
            self.h = L.copy_dna_begin(1)
        elif name == "copy_reads":
            self.h = L.copy_reads_begin(3, 0, 0, 0)
        elif name == "trim_reads":
            self.h = L.trim_reads_begin(0, 0, 0, 0, 0, 0, 0, 0, 0)
        elif name == "copy_dna_to":
            self.h = L.copy_dna_to_begin(1, 0, False)
        elif name == "copy_reads_to":
            self.h = L.copy_reads_to_begin(False)
        assert self.h, L.dna_glue_errmsg()

    def items(self):
        d = self.data
        if self.name in ("copy_dna", "copy_reads", "trim_reads"):
            text = d["lines"] if self.name == "copy_dna" else d["fastq"]
            return [text[a:a + 50] for a in range(0, len(text), 50)] + [None]    # None: the call with last = true
        if self.name == "copy_reads_to":
            return list(zip(d["rows"], d["quals"]))
        if self.name == "table_match":
            return [("build", r) for r in d["rows"][::2]] + [("probe", r) for r in d["rows"]]
        return list(d["rows"])

    def add(self, item):
        L, h, n = self.L, self.h, self.name
        if n in ("copy_dna", "copy_reads", "trim_reads"):
            return bool(L.copy_dna_feed(h, item, len(item), False) if item is not None else L.copy_dna_feed(h, None, 0, True))
        if n == "copy_reads_to":
            return bool(L.copy_reads_to_add(h, item[0].p, item[1], len(item[1])))
        if n == "table_match":
            return bool((L.table_match_add_build if item[0] == "build" else L.table_match_add_probe)(h, item[1].p))
        fn = {"count_kmers_table_agg": L.count_kmers_agg_add, "table_kmers": L.table_kmers_add, "table_hits": L.table_hits_add,
              "table_profile": L.table_profile_add, "table_screen": L.table_screen_add, "table_distinct": L.table_distinct_add,
              "copy_dna_to": L.copy_dna_to_add}[n]
        return bool(fn(h, item.p))

    def finish(self):
        if self.name == "copy_dna_to":
            return bool(self.L.copy_dna_to_finish(self.h))
        if self.name == "copy_reads_to":
            return bool(self.L.copy_reads_to_finish(self.h))
        return True

    def next(self):
        L, h, n, g = self.L, self.h, self.name, self.g
        v = [C.c_int64() for _ in range(3)]
        km, p, q, sz = g._Kmer(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        if n == "count_kmers_table_agg":
            return (km.bit_sequence, v[0].value) if L.count_kmers_agg_next(h, C.byref(km), C.byref(v[0])) else None
        if n == "table_kmers":
            ok = L.table_kmers_next(h, C.byref(v[0]), C.byref(v[1]), C.byref(km))
            return (v[0].value, v[1].value, km.length, km.bit_sequence) if ok else None
        if n == "table_hits":
            return tuple(x.value for x in v) if L.table_hits_next(h, *[C.byref(x) for x in v]) else None
        if n == "table_profile":
            counts = np.empty(L.table_profile_width(h), dtype=np.int64)
            ok = L.table_profile_next(h, C.byref(v[0]), C.byref(v[1]), counts.ctypes.data_as(C.POINTER(C.c_int64)))
            return (v[0].value, v[1].value, tuple(int(c) for c in counts)) if ok else None
        if n == "table_screen":
            if not L.table_screen_next(h, *[C.byref(x) for x in v], C.byref(p)):
                return None
            return tuple(x.value for x in v) + (str(g.dna(p=p.value)),)
        if n == "table_distinct":
            return (v[0].value, v[1].value) if L.table_distinct_next(h, C.byref(v[0]), C.byref(v[1])) else None
        if n == "table_match":
            return tuple(x.value for x in v) if L.table_match_next(h, *[C.byref(x) for x in v]) else None
        if n == "copy_dna":
            return (str(g.dna(p=p.value)), v[0].value) if L.copy_dna_next(h, C.byref(p), C.byref(v[0])) else None
        if n == "copy_reads":
            ok = L.copy_reads_next(h, C.byref(p), C.byref(v[0]), C.byref(v[1]))
            return (str(g.dna(p=p.value)), v[0].value, v[1].value) if ok else None
        if n == "trim_reads":
            if not L.trim_reads_next(h, C.byref(p), C.byref(v[0]), C.byref(v[1]), C.byref(q)):
                return None
            qual = C.string_at(q.value)
            g._libc.free(q.value)
            return (str(g.dna(p=p.value)), v[0].value, v[1].value, qual)
        ok = (L.copy_dna_to_next if n == "copy_dna_to" else L.copy_reads_to_next)(h, C.byref(p), C.byref(sz))
        return C.string_at(p.value, sz.value) if ok else None

    def failed(self):
        n = self.name
        fn = {"count_kmers_table_agg": "count_kmers_agg_failed", "copy_reads": "copy_dna_failed", "trim_reads": "copy_dna_failed"}.get(n, n + "_failed")
        return bool(getattr(self.L, fn)(self.h))

    def end(self):
        n = self.name
        fn = {"count_kmers_table_agg": "count_kmers_agg_end", "copy_reads": "copy_dna_end", "trim_reads": "copy_dna_end"}.get(n, n + "_end")
        getattr(self.L, fn)(self.h)
        self.h = None
        if self.set:
            self.set.end()

    def drain(self):
        out = []
        while (r := self.next()) is not None:
            out.append(r)
        return out

    def errmsg(self):
        return self.L.dna_glue_errmsg().decode()


def settings(g, flush, chunk):
    g.set_agg_flush_bases(flush)
    g.set_copy_chunk_bytes(chunk)


def whole(name, rows):
    """what a run serves, in a form that does not depend on where the batches end: the writers' chunks joined; the groups of
    the aggregate as a set (GROUP BY promises no order, and the accumulator places groups by the batches it was given)"""
    if name in ("copy_dna_to", "copy_reads_to"):
        return b"".join(rows)
    if name == "count_kmers_table_agg":
        return sorted(rows)
    return rows


def run(g, name, data, flush, chunk):
    """every item in, everything served; the COPY ... FROM objects are drained after every piece, as COPY does"""
    settings(g, flush, chunk)
    s = Stream(g, name, data)
    try:
        out = []
        for item in s.items():
            assert s.add(item), s.errmsg()
            if name in ("copy_dna", "copy_reads", "trim_reads"):
                out += s.drain()
        assert s.finish(), s.errmsg()
        out += s.drain()
        assert not s.failed(), s.errmsg()
        return whole(name, out)
    finally:
        s.end()


@pytest.fixture(scope="module")
def served(g, data):
    """every object's rows with the default batch and chunk sizes, computed once"""
    try:
        return {name: run(g, name, data, DEFAULT_FLUSH, DEFAULT_CHUNK) for name in OBJECTS}
    finally:
        settings(g, DEFAULT_FLUSH, DEFAULT_CHUNK)


def test_the_default_run_serves_the_expected_rows(g, data, served):
    """the anchor of the other tests: what the objects serve with the default sizes, against the inputs themselves"""
    texts = data["texts"]
    full = [t for t in texts if t]
    n_kmers = sum(max(0, len(t) - K + 1) for t in texts)
    assert sum(c for _, c in served["count_kmers_table_agg"]) == n_kmers
    assert len(served["table_kmers"]) == n_kmers
    assert [(s, p) for s, p, _, _ in served["table_kmers"]] == [(i, j) for i, t in enumerate(texts) for j in range(max(0, len(t) - K + 1))]
    assert [(s, r) for s, r, _ in served["table_hits"]] == [(i, max(0, len(t) - K + 1)) for i, t in enumerate(texts)]
    assert [(s, r, sum(c)) for s, r, c in served["table_profile"]] == [(i, max(0, len(t) - K + 1), max(0, len(t) - K + 1)) for i, t in enumerate(texts)]
    assert [(s, t) for s, _, _, t in served["table_screen"]] == list(enumerate(texts))       # min_hits 0: every row passes
    first = {}
    for i, t in enumerate(texts):
        first.setdefault(t, i)
    assert served["table_distinct"] == [(i, texts.count(t)) for t, i in sorted(first.items(), key=lambda x: x[1])]
    build = texts[::2]
    assert served["table_match"] == [(i, build.index(t), build.count(t)) for i, t in enumerate(texts) if t in build]
    assert served["copy_dna"] == [(t, i + 1) for i, t in enumerate(full)]
    assert served["copy_reads"] == [(t, i, 0) for i, t in enumerate(full)]
    assert served["trim_reads"] == [(t, i, 0, q) for i, (t, q) in enumerate((t, q) for t, q in zip(texts, data["quals"]) if t)]
    assert served["copy_dna_to"] == "".join(t + "\n" for t in texts).encode()
    assert served["copy_reads_to"] == "".join(f"@{i}\n{t}\n+\n{q.decode()}\n" for i, (t, q) in enumerate(zip(texts, data["quals"]))).encode()


@pytest.mark.parametrize("size", [1, 64])
@pytest.mark.parametrize("name", OBJECTS)
def test_batch_invariance(g, data, served, name, size):
    """the served rows do not depend on the batch size (dna_glue_set_agg_flush_bases) nor, for the COPY objects, on the chunk
    size (dna_glue_set_copy_chunk_bytes): 1, 64 and the default.  The rows include rows without a base, a batch of them only
    and rows longer than a batch; the COPY ... FROM files have no empty row, which the loaders refuse"""
    try:
        if name in COPY_OBJECTS:
            got = run(g, name, data, DEFAULT_FLUSH, size)
        else:
            got = run(g, name, data, size, DEFAULT_CHUNK)
    finally:
        settings(g, DEFAULT_FLUSH, DEFAULT_CHUNK)
    assert got == served[name]


@pytest.mark.parametrize("name", OBJECTS)
def test_life_cycle_refusals(g, data, served, name):
    """after the first served row (the readers: after the last bytes; the writers: after the finish) an _add / _feed returns
    false with the text of the source, the object has not failed, and it serves the rest of its rows"""
    settings(g, 64, 64)
    try:
        s = Stream(g, name, data)
        try:
            items = s.items()
            for item in items:
                assert s.add(item), s.errmsg()
            assert s.finish(), s.errmsg()
            first = s.next()
            assert first is not None
            extra = items[-2] if items[-1] is None else items[-1]
            for _ in range(2):
                assert not s.add(extra)
                assert s.errmsg() == REFUSALS[name]
                assert not s.failed()
            if name == "count_kmers_table_agg":
                assert not s.L.count_kmers_agg_order(s.h, True) and s.errmsg() == MSG_AGG_ORDER and not s.failed()
                assert not s.L.count_kmers_agg_top(s.h, 5) and s.errmsg() == MSG_AGG_TOP and not s.failed()
            assert whole(name, [first] + s.drain()) == served[name]
            assert not s.failed()
            assert not s.add(extra) and s.errmsg() == REFUSALS[name] and not s.failed()      # also after the last row
        finally:
            s.end()
    finally:
        settings(g, DEFAULT_FLUSH, DEFAULT_CHUNK)


@pytest.mark.parametrize("name", OBJECTS)
def test_no_row_at_all(g, data, name):
    """_begin, _next, _end (the readers get their last, empty piece; the writers their finish): no row, no error"""
    s = Stream(g, name, data)
    try:
        if name in ("copy_dna", "copy_reads", "trim_reads"):
            assert s.add(None), s.errmsg()
        assert s.finish(), s.errmsg()
        assert s.next() is None and not s.failed()
        assert s.next() is None and not s.failed()
    finally:
        s.end()


def test_filter_forms(g, data):
    """=, ^@ and @> each give the same rows through generate_kmers_where on one sequence, table_kmers on a table of that
    sequence only and kmer_index.scan over the column of its k-mers; an operator none of them knows is refused by name"""
    text = data["texts"][2]
    d = g.dna(text)
    column = g.generate_kmers(d, K)
    assert len(column) == len(text) - K + 1
    with g.kmer_index(column) as index:
        for op, rhs in (("=", g.kmer(text[40:40 + K])), ("^@", g.kmer(text[40:40 + K - 1])), ("@>", g.qkmer(text[40] + "N" + text[42]))):
            want = [i for i in range(len(column)) if
                    (g.contains(rhs, column[i]) if op == "@>" else g.starts_with(column[i], rhs) if op == "^@" else column[i] == rhs)]
            assert want and len(want) < len(column)
            one = g.generate_kmers_where(d, K, op, rhs)
            seq, pos, keys = g.table_kmers([d], K, op, rhs)
            assert [x.c.bit_sequence for x in one] == [column[i].c.bit_sequence for i in want], op
            assert list(pos) == want and not seq.any() and [int(x) for x in keys] == [x.c.bit_sequence for x in one], op
            assert index.scan(op, rhs) == want, op
    rhs = g.kmer(text[:K])
    L = g.lib()
    assert not L.generate_kmers_where_begin(d.p, K, b"x", C.byref(rhs.c), None)
    assert L.dna_glue_errmsg() == b"unknown operator"
    L.dna_in(b"")                                                         # (another text in between)
    assert not L.table_kmers_begin(K, b"x", C.byref(rhs.c), None)
    assert L.dna_glue_errmsg() == b"unknown operator"


def test_loader_errors(g, data):
    """an invalid byte in the second record: the same text, and the second line / record, through copy_dna, copy_reads and
    trim_reads; a quality line of the wrong length: the library's text through trim_reads, and the same text from
    copy_reads_to"""
    with pytest.raises(g.GlueError) as ei:
        g.copy_dna([b"ACGT\nACZT\nAC\n"])
    assert str(ei.value) == "Invalid character in DNA sequence: Z" and ei.value.line == 2
    fastq = b"@a\nACGT\n+\nIIII\n@b\nACZT\n+\nIIII\n@c\nAC\n+\nII\n"
    for load in (g.copy_reads, g.trim_reads):
        with pytest.raises(g.GlueError) as ei:
            load([fastq])
        assert str(ei.value) == "Invalid character in DNA sequence: Z" and ei.value.record + 1 == 2, load.__name__
    with pytest.raises(g.GlueError) as ei:
        g.trim_reads([b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIII\n@c\nAC\n+\nII\n"])
    assert str(ei.value) == MSG_QUAL_LENGTH and ei.value.record + 1 == 2
    with pytest.raises(g.GlueError) as ei:
        g.copy_reads_to([g.dna("ACGT"), g.dna("ACGT")], [b"IIII", b"III"])
    assert str(ei.value) == MSG_QUAL_LENGTH
