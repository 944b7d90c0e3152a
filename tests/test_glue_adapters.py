"""Adapter trimming composed with the rest of the read pipeline: a named FASTQ loaded into a resident table
with its names and qualities, quality-trimmed, cut at its 3' adapters by dnagpu_dna_adapters on the trim's lists, gathered,
and written back with names and qualities -- byte for byte the text that the models render; the glue's trim_reads handle with
adapters gives the same rows, and without adapters exactly what it gave before."""
import ctypes as C
import importlib

import numpy as np
import pytest

import adapters_model as am
import export_model
import names_model as N
import quals_model as Q
import reads_model
from __graft_entry__ import load_package
from test_read_names import fastq, random_name, random_seq

FASTQ = 3
SEED = 0x3AD4
ADAPTERS = ["AGATCGGAAGAGCACACGTCTGAACTCCAGTC", "CTGTCTCTTATACACATCT"]        # 32 and 19 letters


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


@pytest.fixture(scope="module")
def reads():
    """about 300 named reads of 1 .. 160 bases: a third with an adapter read-through (whole, or clipped by the read's end, one
    letter substituted in some), qualities that fall towards the 3' end so that the quality trim cuts too"""
    rng = np.random.default_rng(SEED)
    seqs, quals, names = [], [], []
    for i in range(300):
        n = int(rng.integers(1, 161))
        s = bytearray(random_seq(rng, n))
        if i % 3 == 0:
            ad = bytearray(ADAPTERS[i % 2].encode())
            if i % 4 == 0:
                ad[int(rng.integers(0, len(ad)))] = ord("A")
            at = int(rng.integers(0, n))
            s = (s[:at] + ad + s[at + len(ad):])[:n]
        q = np.clip(rng.integers(25, 42, size=n) - (np.arange(n) > n - 1 - int(rng.integers(0, 12))) * 25, 0, 93)
        seqs.append(bytes(s))
        quals.append(bytes(int(x) + 33 for x in q))
        names.append(random_name(rng, int(rng.integers(1, 30)), blanks=True))
    return names, seqs, quals


QUALS_OPT = dict(cut_front=20, cut_tail=20, min_bases=15)
AD_OPT = dict(err=(1, 10), min_overlap=3)


def model_rows(text, first_word=False, adapters=True):
    """what the pipeline keeps, from the models alone: (bases, record, offset, quality text, name) of every surviving read"""
    p = reads_model.parse(text, reads_model.Options(format=FASTQ, ambiguous=2))
    starts = N.offsets_of(p.sequences)
    stream = "".join(p.sequences)
    col = Q.column(text, [len(s) for s in p.sequences], p.src_record, p.src_offset)
    nm = N.names_of(text, FASTQ, p.pos, p.src_record, first_word)
    if adapters:
        _, t = am.trim_after_quals(stream, col, starts, ADAPTERS, AD_OPT["err"], AD_OPT["min_overlap"], **QUALS_OPT)
        lists = zip(t.pass_seq, t.pass_first, t.pass_len)
    else:
        t = Q.trim(col, starts, **QUALS_OPT)
        lists = zip(t.seg_seq, t.seg_first, t.seg_len)
    return [(stream[a:a + n], p.src_record[s], p.src_offset[s] + a - starts[s], col[a:a + n], nm[s]) for s, a, n in lists]


def test_glue_adapter_surface_and_refusals(g):
    """the entry points exist; what needs no device: a bad adapter, bad options, another kind of handle, a call after a feed"""
    L = g.lib()
    assert hasattr(L, "trim_reads_add_adapter") and hasattr(L, "trim_reads_adapter_options")
    c = L.trim_reads_begin(0, 0, 0, 0, 0, 0, 0, 0, 0)
    try:
        assert L.trim_reads_add_adapter(c, b"AGATCGGAAGAGC") and L.trim_reads_add_adapter(c, b"NNRYU")
        assert not L.trim_reads_add_adapter(c, b"AGAXC") and "Invalid character in qkmer pattern: X" in str(g._err())
        assert not L.trim_reads_add_adapter(c, b"") and not L.trim_reads_add_adapter(c, b"A" * 33)
        assert L.trim_reads_adapter_options(c, 1, 10, 3, 0) and L.trim_reads_adapter_options(c, 0, 1, 32, 2)
        for bad in ((2, 1, 3, 0), (1, 0, 3, 0), (1, 10, 0, 0), (1, 10, 33, 0), (1, 10, 3, 3), (1, 10, 3, 4)):
            assert not L.trim_reads_adapter_options(c, *bad), bad
        for _ in range(30):
            assert L.trim_reads_add_adapter(c, b"ACGT")
        assert not L.trim_reads_add_adapter(c, b"ACGT") and "at most 32 adapters" in str(g._err())
        assert L.copy_dna_feed(c, b"@r", 2, False)                   # (two bytes: below every chunk size, nothing is loaded)
        assert not L.trim_reads_add_adapter(c, b"ACGT") and "after the first bytes were fed" in str(g._err())
        assert not L.trim_reads_adapter_options(c, 1, 10, 3, 0) and "after the first bytes were fed" in str(g._err())
    finally:
        L.copy_dna_end(c)
    c = L.copy_reads_begin(FASTQ, 0, 0, 0)
    try:
        assert not L.trim_reads_add_adapter(c, b"ACGT") and "only a trim_reads handle" in str(g._err())
        assert not L.trim_reads_adapter_options(c, 1, 10, 3, 0)
    finally:
        L.copy_dna_end(c)


@pytest.mark.gpu
def test_pipeline_byte_for_byte(ctx, pkg, reads):
    """load, names, qualities, dnagpu_quals_trim into device memory, dnagpu_dna_adapters on those lists, the two gathers and
    dnagpu_names_take on its lists, the named FASTQ image with its qualities: equal to the models' rendering"""
    names, seqs, quals = reads
    text = fastq(names, seqs, quals)
    want = model_rows(text)
    plain = model_rows(text, adapters=False)
    assert 0 < len(want) < len(plain) < len(seqs) and sum(len(w[0]) for w in want) < sum(len(w[0]) for w in plain)
    d, rep = ctx.reads_from_text(text, FASTQ, record_pos=True, source=True)
    nm = ctx.names_from_text(text, FASTQ, rep.record_pos, rep.src_record)
    q, _ = ctx.quals_from_fastq(text, d, rep.src_record, rep.src_offset)
    n = d.n_sequences
    dev = ctx.buffer_alloc(3 * 8 * n)
    try:
        tr = ctx.quals_trim_device(d, q, QUALS_OPT, dev_seg=(dev, dev + 8 * n, dev + 16 * n), cap=n)
        out = [np.empty(n, dtype=np.uint64) for _ in range(3)]
        r = ctx.dna_adapters_device(d, ADAPTERS, tr.passed, (dev, dev + 8 * n, dev + 16 * n), 1, (None,) * 3,
                                    [a.ctypes.data for a in out], n, 0, min_bases=QUALS_OPT["min_bases"], **AD_OPT)
        assert r.segments == tr.passed and r.passed == len(want) and r.trimmed > 20
        seg_seq, seg_first, seg_len = (a[:r.passed] for a in out)
        t = ctx.dna_gather(d, seg_first, seg_len)
        qt = ctx.quals_gather(q, seg_first, seg_len)
        nt = ctx.names_take(nm, seg_seq)
        try:
            with ctx.table_to_text_named(t, nt, FASTQ) as img:
                assert img.read_quals(qt) == N.render_named([w[0] for w in want], [w[4] for w in want], [w[3] for w in want],
                                                            export_model.Options(FASTQ))
        finally:
            for o in (t, qt, nt):
                o.free()
    finally:
        ctx.buffer_free(dev)
        for o in (q, nm, d):
            o.free()


@pytest.mark.gpu
def test_glue_trim_reads_with_and_without_adapters(ctx, g, reads):
    """the trim_reads handle with adapters gives the models' rows -- the file whole and in pieces, chunks so small that records
    straddle them, with names and without -- and without adapters exactly the rows of the quality trim alone"""
    names, seqs, quals = reads
    text = fastq(names[:120], seqs[:120], quals[:120])
    want, plain = model_rows(text), model_rows(text, adapters=False)
    assert 0 < len(want) < len(plain)
    ad = dict(adapters=ADAPTERS, adapter_opt=(*AD_OPT["err"], AD_OPT["min_overlap"], 0))
    try:
        for chunk in (97, 64 << 20):
            g.set_copy_chunk_bytes(chunk)
            for pieces in ([text], [text[a:a + 500] for a in range(0, len(text), 500)]):
                rows, rec, off, qs, nms = g.trim_reads_named(pieces, ambiguous=2, **QUALS_OPT, **ad)
                assert [(str(r), a, b, q_, n_) for r, a, b, q_, n_ in zip(rows, rec, off, qs, nms)] == want, (chunk, len(pieces))
            rows, rec, off, qs = g.trim_reads([text], ambiguous=2, **QUALS_OPT, **ad)
            assert [(str(r), a, b, q_) for r, a, b, q_ in zip(rows, rec, off, qs)] == [w[:4] for w in want], chunk
            rows, rec, off, qs, nms = g.trim_reads_named([text], ambiguous=2, **QUALS_OPT)
            assert [(str(r), a, b, q_, n_) for r, a, b, q_, n_ in zip(rows, rec, off, qs, nms)] == plain, chunk
        # the discard flag: only the reads that were cut
        rows, rec, off, qs = g.trim_reads([text], ambiguous=2, **QUALS_OPT, adapters=ad["adapters"],
                                          adapter_opt=(1, 10, 3, 1))
        assert 0 < len(rows) < len(want) and set(rec) <= {w[1] for w in want}
    finally:
        g.set_copy_chunk_bytes(64 << 20)
