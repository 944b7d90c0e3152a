"""The names column of a table of reads (dnagpu_names_*, dnagpu_table_to_text_named): loaded from the FASTA /
FASTQ bytes the table came from, taken beside the table, written into the headers of the text image.

The reference of every comparison is tests/names_model.py, plain Python loops that state the contract of include/dnagpu.h and
share nothing with the C++; the model itself is guarded by vectors written out by hand and by the loader's model
(reads_model.parse), at whose record_pos its names must sit.  Every GPU test runs twice: as it is, and with poisoned, guarded
pool buffers.  All sizes come from the library's geometry calls."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import export_model
import names_model as N
import quals_model as Q
import reads_model
from __graft_entry__ import ROOT, load_package
from test_device_io import Arena
from test_dna_take import TAKE_IDS, check_table, encode_table

BAD_ARG, TOO_LARGE = 5, 6
LINES, FASTA, FASTQ = 1, 2, 3
SEED = 0x7A3E
U64_MAX = 2 ** 64 - 1
EDGE_LENGTHS = [1, 15, 16, 17, 31, 32, 33]
NAME_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33]
NAME_BYTES = bytes(b for b in range(33, 127) if b not in b"@>+")        # no blank, no terminator


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def random_seq(rng, n, letters=b"ATCG"):
    return bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), n)) if n else b""


def random_qual(rng, n):
    return bytes(rng.integers(33, 127, size=n, dtype=np.uint8)) if n else b""


def random_name(rng, n, blanks=False):
    """n bytes without CR / LF; blanks: a blank or a tab somewhere inside (not first), where n allows"""
    b = bytearray(rng.choice(np.frombuffer(NAME_BYTES, dtype=np.uint8), n)) if n else bytearray()
    if blanks and n >= 3:
        b[int(rng.integers(1, n - 1))] = 0x20 if rng.integers(2) else 0x09
    return bytes(b)


def fastq(names, seqs, quals, crlf=False, last_newline=True):
    t = b"\r\n" if crlf else b"\n"
    out = b"".join(b"@" + nm + t + s + t + b"+" + t + q + t for nm, s, q in zip(names, seqs, quals))
    return out if last_newline else out[:-len(t)]


def fasta(names, seqs, width=0, crlf=False):
    t = b"\r\n" if crlf else b"\n"
    out = bytearray()
    for nm, s in zip(names, seqs):
        out += b">" + nm + t
        w = width if 0 < width < len(s) else len(s)
        for at in range(0, len(s), max(w, 1)):
            out += s[at:at + w] + t
    return bytes(out)


def positions(text, fmt):
    """the offsets of the header lines: FASTQ every fourth line, FASTA the lines that begin with '>'"""
    pos, at, line = [], 0, 0
    while at < len(text):
        if (line % 4 == 0) if fmt == FASTQ else text[at] == ord(">"):
            pos.append(at)
        nl = text.find(b"\n", at)
        at = len(text) if nl < 0 else nl + 1
        line += 1
    return pos


# ------------------------------------------------------------------ CPU: the reference itself

def test_the_model_on_hand_written_vectors():
    """a guard on the reference itself.  It runs no code of the project."""
    text = b"@a b\nAC\n+\nII\n@\nG\n+\nI\n@cc\td e\nT\n+\nI\n"
    pos = [0, 13, 21]
    assert N.names_of(text, FASTQ, pos) == [b"a b", b"", b"cc\td e"]
    assert N.names_of(text, FASTQ, pos, first_word=True) == [b"a", b"", b"cc"]          # a blank, nothing, a tab
    assert N.names_of(text, FASTQ, pos, [2, 2, 0, 1]) == [b"cc\td e", b"cc\td e", b"a b", b""]    # SPLIT: copies of the record's name
    # CRLF: the '\r' belongs to the terminator, with and without FIRST_WORD; an empty name of a CRLF file
    text = b">x y\r\nAC\r\n>\r\nG\r\n"
    assert N.names_of(text, FASTA, [0, 10]) == [b"x y", b""]
    assert N.names_of(text, FASTA, [0, 10], first_word=True) == [b"x", b""]
    # a lone '\r': inside the name it is an error at its offset; behind the first word FIRST_WORD never sees it
    text = b">ab\rc d\nAC\n>e \rf\nG\n"
    for fw in (False, True):
        with pytest.raises(N.NamesError) as ei:
            N.names_of(text, FASTA, [0, 11], first_word=fw)
        assert (ei.value.pos, ei.value.record) == (3, 0)
    with pytest.raises(N.NamesError) as ei:
        N.names_of(text, FASTA, [0, 11], [1, 0])                     # the lowest-numbered SEQUENCE wins, not the lowest offset
    assert (ei.value.pos, ei.value.record) == (14, 1)
    assert N.names_of(text, FASTA, [0, 11], [1], first_word=True) == [b"e"]
    # a header that is the text's unterminated last line: it ends at the text's end, and a '\r' there is content
    assert N.names_of(b">a\nAC\n>last one", FASTA, [0, 6]) == [b"a", b"last one"]
    assert N.names_of(b">a\nAC\n>last one", FASTA, [0, 6], first_word=True) == [b"a", b"last"]
    with pytest.raises(N.NamesError) as ei:
        N.names_of(b">a\nAC\n>last\r", FASTA, [0, 6])
    assert (ei.value.pos, ei.value.record) == (11, 1)
    assert N.names_of(b">", FASTA, [0]) == [b""]
    # sources that are no record
    for pos, rec in (([0, 7], None), ([1], None), ([0], [1]), ([16], None)):
        with pytest.raises(N.SourceError):
            N.names_of(b">a\nAC\n>last one", FASTA, pos, rec)
    with pytest.raises(N.SourceError):
        N.names_of(b">a\nAC\n", FASTQ, [0])                          # the other format's marker
    # take, offsets, render
    assert N.take([b"a", b"", b"cc"], [2, 0, 2, 1]) == [b"cc", b"a", b"cc", b""] and N.take([b"a"], []) == []
    with pytest.raises(IndexError):
        N.take([b"a"], [1])
    assert N.offsets_of([b"a", b"", b"cc"]) == [0, 1, 1, 3]
    opt = export_model.Options(FASTQ, crlf=True, prefix=b"ignored", name_base=7)
    assert N.render_named(["AC", "", "G"], [b"n 1", b"", b"x"], [b"!~", b"", b"#"], opt) == \
        b"@n 1\r\nAC\r\n+\r\n!~\r\n@\r\n\r\n+\r\n\r\n@x\r\nG\r\n+\r\n#\r\n"
    assert N.render_named(["AC"], [b"q"], None, export_model.Options(FASTQ, quality=b"#")) == b"@q\nAC\n+\n##\n"
    opt = export_model.Options(FASTA, line_width=2)
    assert N.render_named(["ACGTA", ""], [b"one", b"none"], None, opt) == b">one\nAC\nGT\nA\n>none\n"


def test_the_model_beside_the_loaders_model():
    """for random FASTQ and FASTA under ERROR, DROP, SPLIT and min_bases the names the model yields from reads_model.parse's
    record_pos and src_record are the names the file was written with.  It runs no code of the project."""
    rng = np.random.default_rng(SEED)
    for it in range(40):
        letters = b"ATCG" if it % 4 == 0 else b"ATCGATCGATCGN"
        seqs = [random_seq(rng, int(n), letters) for n in rng.integers(1, 60, size=int(rng.integers(1, 9)))]
        names = [random_name(rng, int(n), blanks=bool(it & 2)) for n in rng.integers(0, 40, size=len(seqs))]
        quals = [random_qual(rng, len(s)) for s in seqs]
        crlf = bool(it & 1)
        for fmt, text in ((FASTQ, fastq(names, seqs, quals, crlf, it % 3 != 0)), (FASTA, fasta(names, seqs, 7 * (it % 3), crlf))):
            for amb, min_bases in ((reads_model.ERROR, 0), (reads_model.DROP, 0), (reads_model.SPLIT, 0), (reads_model.SPLIT, 5)):
                p = reads_model.parse(text, reads_model.Options(format=fmt, ambiguous=amb, min_bases=min_bases))
                if p.error is not None:
                    assert amb == reads_model.ERROR
                    continue
                assert p.pos == positions(text, fmt)
                assert N.names_of(text, fmt, p.pos, p.src_record) == [names[r] for r in p.src_record]
                first = [nm.replace(b"\t", b" ").split(b" ")[0] for nm in names]
                assert N.names_of(text, fmt, p.pos, p.src_record, first_word=True) == [first[r] for r in p.src_record]


SANITIZERS = ["-g", "-Xarch_host", "-fsanitize=address,undefined"]


@pytest.mark.parametrize("extra", [[], SANITIZERS], ids=["plain", "sanitizers"])
def test_names_math_on_the_host(tmp_path, extra):
    """names_math.hpp, host code of the header the kernels share, as a stand-alone program (the second build with
    AddressSanitizer and UndefinedBehaviorSanitizer on it): the end of a name from the masks and the suffix minima, built as the
    kernels build them in arrays of the driver's sizes, must agree with a naive walk inside the same program"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "names_math_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", *extra, "-I",
                           os.path.join(ROOT, "dna-sequences-pg-extension_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "names_math_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


NEW_SYMBOLS = ("dnagpu_names_upload", "dnagpu_names_sequences", "dnagpu_names_bytes", "dnagpu_names_offsets", "dnagpu_names_read",
               "dnagpu_names_free", "dnagpu_names_from_text", "dnagpu_names_take", "dnagpu_table_to_text_named",
               "dnagpu_names_geometry")


def test_names_symbols_and_geometry(pkg):
    """every new symbol of the header resolves in the built library; the ABI version stays 2; the geometry needs no device"""
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert pkg.abi_version() == 2
    chunk, tile, group = pkg.names_geometry()
    assert tile == pkg.text_geometry() and tile % chunk == 0 and group >= 2
    one = C.c_uint64()
    assert L.dnagpu_names_geometry(None, C.byref(one), C.byref(one)) == BAD_ARG
    assert C.sizeof(pkg.binding._NamesReportC) == 24
    for name in ("n_sequences", "n_bytes", "offsets", "read", "read_device", "download", "free"):
        assert hasattr(pkg.Names, name)
    assert pkg.NAMES_FIRST_WORD == 1


def test_names_argument_rules_without_a_device(pkg):
    """the checks that need no device, in their documented order, with a context and objects that are never dereferenced; *out
    left as it was; the report cleared"""
    L = pkg.lib()
    Rep = pkg.binding._NamesReportC
    out = C.c_void_p(77)
    ctx, obj = C.c_void_p(1), C.c_void_p(1)                                    # (never dereferenced below)
    text = C.create_string_buffer(b"@a\nA\n+\nI\n")
    off = (C.c_uint64 * 2)(0, 1)
    rep = Rep(bad_pos=5, bad_record=5, bad_char=b"x")
    up = L.dnagpu_names_upload
    assert up(None, text, off, 1, 0, C.byref(out), C.byref(rep)) == BAD_ARG
    assert (rep.bad_pos, rep.bad_record, rep.bad_char) == (U64_MAX, U64_MAX, b"\0")
    assert up(ctx, text, off, 1, 0, None, None) == BAD_ARG
    assert up(ctx, text, None, 1, 0, C.byref(out), None) == BAD_ARG
    assert up(None, text, off, 1 << 32, 0, C.byref(out), None) == BAD_ARG      # the NULL before the size
    assert up(ctx, text, off, 1 << 32, 0, C.byref(out), None) == TOO_LARGE
    assert up(ctx, None, off, 1, 0, C.byref(out), None) == BAD_ARG             # host offsets: NULL bytes with a non-zero total
    # the accessors on NULL
    assert L.dnagpu_names_sequences(None) == 0 and L.dnagpu_names_bytes(None) == 0
    for count in (0, 1):
        assert L.dnagpu_names_read(ctx, None, 0, count, text, 0) == BAD_ARG
        assert L.dnagpu_names_read(None, obj, 0, count, text, 0) == BAD_ARG
        assert L.dnagpu_names_offsets(ctx, None, 0, count, off, 0) == BAD_ARG
        assert L.dnagpu_names_offsets(None, obj, 0, count, off, 0) == BAD_ARG
    L.dnagpu_names_free(ctx, None)
    L.dnagpu_names_free(None, None)
    # from_text: the NULLs, the format, the flags, the counts, the sizes
    call = L.dnagpu_names_from_text
    pos = (C.c_uint64 * 1)(0)
    rep = Rep(bad_pos=5, bad_record=5, bad_char=b"x")
    assert call(None, text, 9, 0, FASTQ, 0, pos, 1, None, 1, C.byref(out), C.byref(rep)) == BAD_ARG
    assert (rep.bad_pos, rep.bad_record, rep.bad_char) == (U64_MAX, U64_MAX, b"\0")
    assert call(ctx, text, 9, 0, FASTQ, 0, pos, 1, None, 1, None, None) == BAD_ARG
    assert call(ctx, None, 9, 0, FASTQ, 0, pos, 1, None, 1, C.byref(out), None) == BAD_ARG
    assert call(ctx, text, 9, 0, FASTQ, 0, None, 1, None, 1, C.byref(out), None) == BAD_ARG
    for fmt in (LINES, 0, 4):
        assert call(ctx, text, 9, 0, fmt, 0, pos, 1, None, 1, C.byref(out), None) == BAD_ARG
    assert call(ctx, text, 9, 0, FASTQ, 2, pos, 1, None, 1, C.byref(out), None) == BAD_ARG
    assert call(ctx, text, 9, 0, FASTQ, 0, pos, 1, None, 2, C.byref(out), None) == BAD_ARG       # no src_record: n_seqs == n_records
    assert call(ctx, text, 1 << 32, 0, LINES, 0, pos, 1, None, 1, C.byref(out), None) == BAD_ARG  # the format before the size
    assert call(ctx, text, 1 << 32, 0, FASTQ, 0, pos, 1, None, 1, C.byref(out), None) == TOO_LARGE
    assert call(ctx, text, 9, 0, FASTQ, 0, pos, 1 << 32, pos, 1, C.byref(out), None) == TOO_LARGE
    assert call(ctx, text, 9, 0, FASTQ, 0, pos, 1, pos, 1 << 32, C.byref(out), None) == TOO_LARGE
    # take
    take = L.dnagpu_names_take
    assert take(None, obj, pos, 1, 0, C.byref(out)) == BAD_ARG
    assert take(ctx, None, pos, 1, 0, C.byref(out)) == BAD_ARG
    assert take(ctx, obj, None, 1, 0, C.byref(out)) == BAD_ARG
    assert take(ctx, obj, pos, 1, 0, None) == BAD_ARG
    # the named image: the NULLs, then the options
    Opt = pkg.binding._TextOutOptionsC
    good = Opt(format=FASTQ)
    named = L.dnagpu_table_to_text_named
    for args in ((None, obj, obj, C.byref(good)), (ctx, None, obj, C.byref(good)), (ctx, obj, None, C.byref(good)), (ctx, obj, obj, None)):
        assert named(*args, C.byref(out)) == BAD_ARG
    assert named(ctx, obj, obj, C.byref(good), None) == BAD_ARG
    for bad in (Opt(format=0), Opt(format=4), Opt(format=FASTQ, flags=2), Opt(format=FASTQ, line_width=3), Opt(format=LINES)):
        assert named(ctx, obj, obj, C.byref(bad), C.byref(out)) == BAD_ARG
    assert out.value == 77 and text.raw == b"@a\nA\n+\nI\n\0"


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


def check_names(nm, want, what=""):
    assert nm.n_sequences == len(want) and nm.n_bytes == sum(len(x) for x in want), what
    assert [int(x) for x in nm.offsets()] == N.offsets_of(want), what
    got = nm.download()
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{what}: name {at} of {len(want)}: got {got[at][:60]!r} want {want[at][:60]!r}")


def check_from_text(ctx, pkg, text, fmt, pos, rec=None, what="", arena=None, offsets=()):
    """names_from_text with and without FIRST_WORD against the model, from host memory and, with an arena, from device memory
    at every destination offset of `offsets`"""
    for fw in (False, True):
        want = N.names_of(text, fmt, pos, rec, fw)
        with ctx.names_from_text(text, fmt, pos, rec, first_word=fw) as nm:
            check_names(nm, want, f"{what} first_word={fw}")
        for off in offsets:
            arena.reset()
            p = arena.take("text", len(text), off, text)
            dp = arena.take("record_pos", 8 * len(pos), 0, np.array(pos, dtype=np.uint64))
            n_seqs = len(pos) if rec is None else len(rec)
            dr = None if rec is None else arena.take("src_record", 8 * len(rec), 0, np.array(rec, dtype=np.uint64))
            with ctx.names_from_text_device(p, len(text), fmt, dp, len(pos), dr, n_seqs, first_word=fw) as nm:
                check_names(nm, want, f"{what} first_word={fw} device text at offset {off}")
            arena.check(f"{what} text at offset {off}")


@pytest.mark.gpu
@pytest.mark.parametrize("crlf", [False, True], ids=["lf", "crlf"])
def test_names_from_text_edge_lengths_and_alignments(ctx, dbg, pkg, crlf):
    """names of 0, 1, 15, 16, 17, 31, 32, 33 bytes (with and without a blank inside), FASTQ and FASTA, the last line with and
    without its terminator, from host memory and from device memory at every alignment 0 .. 15 (the odd addresses among them)"""
    rng = np.random.default_rng(SEED + 1 + crlf)
    lengths = [int(x) for x in rng.permutation(NAME_LENGTHS * 3)]
    names = [random_name(rng, n, blanks=i % 2 == 1) for i, n in enumerate(lengths)]
    seqs = [random_seq(rng, int(n)) for n in rng.integers(1, 40, size=len(names))]
    quals = [random_qual(rng, len(s)) for s in seqs]
    ar = Arena(ctx, 1 << 16)
    try:
        for last_newline in (True, False):
            text = fastq(names, seqs, quals, crlf, last_newline)
            check_from_text(ctx, pkg, text, FASTQ, positions(text, FASTQ), None, f"fastq crlf={crlf}", ar, range(16))
        text = fasta(names, seqs, 11, crlf)
        check_from_text(ctx, pkg, text, FASTA, positions(text, FASTA), None, f"fasta crlf={crlf}", ar, (0, 1, 7))
        text = fasta(names, seqs, 0, crlf)[:-(2 if crlf else 1) - len(seqs[-1])]       # the last header's '\n' is the text's last byte
        check_from_text(ctx, pkg, text, FASTA, positions(text, FASTA), None, "a header last")
        text = text[:-(2 if crlf else 1)]                                              # ... and the unterminated last line
        check_from_text(ctx, pkg, text, FASTA, positions(text, FASTA), None, "an unterminated header last")
    finally:
        ar.free()


@pytest.mark.gpu
def test_names_from_text_tile_edges(ctx, dbg, pkg):
    """a header whose '\\n' is the last byte of a tile of the sweep and one whose '\\n' is the first byte of the next; a header
    that spans more than two whole tiles (a tile with no line end at all); a FIRST_WORD blank in an earlier tile than the
    '\\n'; a CRLF pair across the boundary; and one text of more tiles than one group of the suffix minimum holds, whose long
    header ends in another group"""
    rng = np.random.default_rng(SEED + 3)
    chunk, G, group = pkg.names_geometry()
    cases = {}
    for end in (G - 1, G, G + 1):                                    # the first header's '\n' at offset `end`
        cases[f"'\\n' at {end}"] = ([end - 1, 5, 20], False)
        cases[f"'\\r\\n' ends at {end}"] = ([end - 2, 5, 20], True)
    cases["a header of more than two tiles"] = ([7, 2 * G + G // 2 + 3, 9], False)
    cases["a header of three tiles, crlf"] = ([3 * G + 1, 4], True)
    for what, (lengths, crlf) in cases.items():
        names = [random_name(rng, n) for n in lengths]
        seqs = [random_seq(rng, 20) for _ in names]
        quals = [random_qual(rng, 20) for _ in names]
        text = fastq(names, seqs, quals, crlf)
        pos = positions(text, FASTQ)
        assert len(pos) == len(names)
        check_from_text(ctx, pkg, text, FASTQ, pos, None, what)
        if "tiles" in what:                                          # the blank in the header's first tile, its '\n' tiles later
            k = max(range(len(names)), key=lambda i: len(names[i]))
            nm = bytearray(names[k])
            nm[5] = 0x20
            nm[G + 17] = 0x09
            names[k] = bytes(nm)
            text = fastq(names, seqs, quals, crlf)
            check_from_text(ctx, pkg, text, FASTQ, positions(text, FASTQ), None, what + ", a blank early")
    # more than one group of tiles: a header that begins in the first group and ends in the second, short ones around it
    long = group * G + 3 * G + 11
    names = [b"first", random_name(rng, long), b"after it", b""]
    seqs = [random_seq(rng, 30) for _ in names]
    text = fasta(names, seqs, 0)
    pos = positions(text, FASTA)
    assert len(text) > (group + 1) * G and pos[1] < G and pos[2] > group * G
    for fw in (False, True):
        with ctx.names_from_text(text, FASTA, pos, [3, 1, 0, 2, 1], first_word=fw) as nm:
            want = [names[3], names[1], b"first", b"after" if fw else b"after it", names[1]]
            assert nm.download() == want


@pytest.mark.gpu
def test_names_under_the_loaders_policies(ctx, dbg, pkg):
    """DROP, SPLIT and min_bases through dnagpu_reads_from_text's own record_pos / src_record: every sequence carries its
    record's name; a chunked load with DNAGPU_READS_MORE where a record is held back"""
    rng = np.random.default_rng(SEED + 5)
    lengths = [int(n) for n in rng.integers(1, 200, size=100)] + EDGE_LENGTHS
    seqs = [random_seq(rng, n, b"ATCG" * 20 + b"N") for n in lengths]
    quals = [random_qual(rng, n) for n in lengths]
    names = [random_name(rng, int(n), blanks=True) for n in rng.integers(0, 50, size=len(seqs))]
    for fmt, text in ((FASTQ, fastq(names, seqs, quals)), (FASTA, fasta(names, seqs, 60))):
        for kw in (dict(ambiguous=pkg.AMBIG_DROP), dict(ambiguous=pkg.AMBIG_SPLIT), dict(ambiguous=pkg.AMBIG_SPLIT, min_bases=12),
                   dict(ambiguous=pkg.AMBIG_DROP, min_bases=20)):
            p = reads_model.parse(text, reads_model.Options(format=fmt, ambiguous=kw["ambiguous"], min_bases=kw.get("min_bases", 0)))
            d, rep = ctx.reads_from_text(text, fmt, record_pos=True, source=True, **kw)
            check_table(d, p.sequences, str(kw))
            assert 0 < d.n_sequences != len(seqs)
            for fw in (False, True):
                want = N.names_of(text, fmt, p.pos, p.src_record, fw)
                assert fw or want == [names[r] for r in p.src_record]
                with ctx.names_from_text(text, fmt, rep.record_pos, rep.src_record, first_word=fw) as nm:
                    check_names(nm, want, f"{fmt} {kw} first_word={fw}")
            d.free()
    # chunks: the unfinished last record of a chunk is held back and named with the next chunk
    text = fastq(names, seqs, quals)
    got, at, step = [], 0, 3000
    while at < len(text):
        chunk = text[at:at + step]
        more = at + step < len(text)
        d, rep = ctx.reads_from_text(chunk, FASTQ, ambiguous=pkg.AMBIG_SPLIT, more=more, record_pos=True, source=True)
        assert rep.consumed > 0
        for data in (chunk[:rep.consumed], chunk):                   # the loader's `consumed`, or the whole chunk
            with ctx.names_from_text(data, FASTQ, rep.record_pos, rep.src_record) as nm:
                part = nm.download()
        got += part
        d.free()
        at += rep.consumed
    p = reads_model.parse(text, reads_model.Options(format=FASTQ, ambiguous=reads_model.SPLIT))
    assert got == [names[r] for r in p.src_record]


@pytest.mark.gpu
def test_names_errors(ctx, dbg, pkg):
    """a '\\r' inside a name: the lowest sequence wins, its text offset and record are reported; a bad marker, a record_pos past
    the text, a src_record out of range; the upload's offset checks and a CR / LF in an upload with its offset.  After each
    error *out is untouched and nothing stays allocated"""
    rng = np.random.default_rng(SEED + 6)
    _, G, _ = pkg.names_geometry()
    names = [random_name(rng, int(n)) for n in rng.integers(4, 60, size=200)]
    seqs = [random_seq(rng, 40) for _ in names]
    quals = [random_qual(rng, 40) for _ in names]
    good = fastq(names, seqs, quals)
    assert len(good) > 2 * G
    pos = positions(good, FASTQ)
    with ctx.names_from_text(good, FASTQ, pos) as nm:                # (warm: the pool holds what the calls below need)
        check_names(nm, names)
    before = ctx.device_bytes()

    def refused(text, p, rec=None, fw=False):
        with pytest.raises(pkg.DnaGpuError) as ei:
            ctx.names_from_text(text, FASTQ, p, rec, first_word=fw)
        assert ei.value.code == BAD_ARG
        return ei.value.report

    def edit(edits):
        t = bytearray(good)
        for at, b in edits:
            t[at:at + len(b)] = b
        return bytes(t)

    for edits, rec in (([(pos[3] + 2, b"\r")], None), ([(pos[150] + 3, b"\r"), (pos[20] + 1, b"\r"), (pos[20] + 3, b"\r")], None),
                       ([(pos[150] + 3, b"\r"), (pos[20] + 1, b"\r")], [150, 20, 3]), ([(pos[199] + 1, b"\r")], None),
                       ([(pos[0] + 1, b"\r")], [5, 6, 0, 0])):
        text = edit(edits)
        with pytest.raises(N.NamesError) as want:
            N.names_of(text, FASTQ, pos, rec)
        rep = refused(text, pos, rec)
        assert (rep.bad_pos, rep.bad_record, rep.bad_char) == (want.value.pos, want.value.record, b"\r"), (edits, rep)
        assert pkg.lib().dnagpu_last_error().decode() == N.MSG_CHAR
    # a lone '\r' that is in no name -- a quality line's, or behind the first word -- is no error of this call
    text = edit([(pos[7] - 3, b"\r")])
    with ctx.names_from_text(text, FASTQ, pos) as nm:
        check_names(nm, names)
    text = edit([(pos[9] + 2, b" "), (pos[9] + 3, b"\r")])
    with ctx.names_from_text(text, FASTQ, pos, first_word=True) as nm:
        assert nm.download()[9] == names[9][:1]
    assert refused(text, pos).bad_pos == pos[9] + 3
    # sources that are no record: no offset
    for p, rec in ((pos[:5] + [pos[5] + 1], None), (pos[:5] + [len(good)], None), (pos[:5] + [U64_MAX], None), (pos, [0, 200]),
                   (pos, [U64_MAX]), (pos[:1], [0, 1])):
        rep = refused(good, p, rec)
        assert rep.bad_pos is None and rep.bad_record is None, (p[-1], rec)
    assert refused(b"", pos[:1]).bad_pos is None
    with pytest.raises(pkg.DnaGpuError) as ei:
        ctx.names_from_text(good, FASTA, pos)                        # '@' is not FASTA's marker
    assert ei.value.code == BAD_ARG
    with pytest.raises(pkg.DnaGpuError) as ei:
        ctx.names_from_text(good, LINES, pos)
    assert ei.value.code == BAD_ARG
    # upload: the offsets, then the bytes
    data = b"".join(names)
    off = N.offsets_of(names)
    for bad in ([1] + off[1:], off[:50] + [off[50] + 100] + off[51:], off[:-1] + [off[-2] - 1], [0, 5, 4] + off[3:]):
        with pytest.raises(pkg.DnaGpuError) as ei:
            ctx.names_upload_raw(data, bad, len(names))
        assert ei.value.code == BAD_ARG and ei.value.report.bad_pos is None, bad[:4]
    with pytest.raises(pkg.DnaGpuError) as ei:
        ctx.names_upload_raw(data, off[:-1] + [1 << 32], len(names))
    assert ei.value.code == TOO_LARGE
    for at, ch in ((0, b"\n"), (15, b"\r"), (16, b"\n"), (len(data) - 1, b"\r"), (500, b"\n")):
        bad = bytearray(data)
        bad[at:at + 1] = ch
        if at < 900:
            bad[at + 37] = 10                                          # a later one does not win
        with pytest.raises(pkg.DnaGpuError) as ei:
            ctx.names_upload_raw(bytes(bad), off, len(names))
        rep = ei.value.report
        assert ei.value.code == BAD_ARG and (rep.bad_pos, rep.bad_record, rep.bad_char) == (at, None, ch), (at, rep)
        assert pkg.lib().dnagpu_last_error().decode() == N.MSG_CHAR
    assert ctx.device_bytes() == before
    # *out untouched by a refused call
    out = C.c_void_p(77)
    p = np.array(pos[:1], dtype=np.uint64)
    assert pkg.lib().dnagpu_names_from_text(ctx.h, b"Xa\n", 3, 0, FASTQ, 0, p.ctypes.data, 1, None, 1, C.byref(out), None) == BAD_ARG
    o = np.array([0, 1], dtype=np.uint64)
    assert pkg.lib().dnagpu_names_upload(ctx.h, b"\n", o.ctypes.data, 1, 0, C.byref(out), None) == BAD_ARG
    assert out.value == 77 and ctx.device_bytes() == before


@pytest.mark.gpu
def test_names_upload_read_and_windows(ctx, dbg, pkg):
    """a column from the caller's arrays in host and in device memory; windows of its bytes and of its offsets; the empty
    column and the column of empty names"""
    rng = np.random.default_rng(SEED + 7)
    names = [random_name(rng, n, blanks=True) for n in NAME_LENGTHS * 2 + [100]]
    data, off = b"".join(names), N.offsets_of(names)
    ar = Arena(ctx, 1 << 15)
    try:
        with ctx.names_upload(names) as nm:
            check_names(nm, names)
            total, n = len(data), len(names)
            for first, count in ((0, 0), (0, 1), (1, 15), (15, 17), (total - 1, 1), (total, 0), (3, total - 3)):
                assert nm.read(first, count) == data[first:first + count]
            for first, count in ((0, 0), (0, 1), (n, 1), (n + 1, 0), (3, 5)):
                assert [int(x) for x in nm.offsets(first, count)] == off[first:first + count]
            for first, count in ((total + 1, 0), (0, total + 1), (total, 1), (U64_MAX, 1), (2, U64_MAX)):
                with pytest.raises(pkg.DnaGpuError) as ei:
                    nm.read_device(first, count, ar.base)
                assert ei.value.code == BAD_ARG
            for first, count in ((n + 2, 0), (0, n + 2), (n + 1, 1), (U64_MAX, 1), (2, U64_MAX)):
                with pytest.raises(pkg.DnaGpuError) as ei:
                    nm.offsets_device(first, count, ar.base)
                assert ei.value.code == BAD_ARG
            p = ar.take("window", 40, 5)
            q = ar.take("offsets", 8 * 4, 0)
            nm.read_device(7, 40, p)
            nm.offsets_device(2, 4, q)
            ar.check("windows into device memory", {p: data[7:47], q: np.array(off[2:6], dtype=np.uint64)})
        for a in (0, 1, 5):
            ar.reset()
            p = ar.take("bytes", len(data), a, data)
            q = ar.take("offsets", 8 * len(off), 0, np.array(off, dtype=np.uint64))
            with ctx.names_upload_device(p, q, len(names)) as nm:
                check_names(nm, names, f"device arrays at offset {a}")
            ar.check("upload from device memory")
        with ctx.names_upload([]) as nm:
            check_names(nm, [])
            assert nm.read() == b"" and [int(x) for x in nm.offsets()] == [0]
        with ctx.names_upload([b"", b"", b""]) as nm:
            check_names(nm, [b"", b"", b""])
    finally:
        ar.free()


@pytest.mark.gpu
def test_names_take(ctx, dbg, pkg):
    """repeated and reversed ids, an empty list, thousands of names of 0 .. 2 bytes (more names under one tile of the copy than
    it stages in LDS), ids in device memory, an id out of range; the result names dnagpu_dna_take's table"""
    rng = np.random.default_rng(SEED + 8)
    _, tile, lds_segs = pkg.quals_copy_geometry()
    names = [random_name(rng, int(n)) for n in rng.integers(0, 70, size=12)]
    ar = Arena(ctx, 1 << 17)
    try:
        with ctx.names_upload(names) as nm:
            for ids in (TAKE_IDS, list(range(11, -1, -1)), [5] * 9, [], [0], list(range(12)) * 3):
                with ctx.names_take(nm, ids) as t:
                    check_names(t, N.take(names, ids), str(ids))
            ar.reset()
            di = ar.take("ids", 8 * len(TAKE_IDS), 0, np.array(TAKE_IDS, dtype=np.uint64))
            with ctx.names_take(nm, (di, len(TAKE_IDS)), on_device=True) as t:
                check_names(t, N.take(names, TAKE_IDS), "ids on the device")
            ar.check("ids on the device")
            before = ctx.device_bytes()
            for bad in ([12], [0, U64_MAX], [3] * 500 + [12]):
                with pytest.raises(pkg.DnaGpuError) as ei:
                    ctx.names_take(nm, bad)
                assert ei.value.code == BAD_ARG
            assert ctx.device_bytes() == before
        with ctx.names_upload([]) as none:
            with ctx.names_take(none, []) as t:
                check_names(t, [])
            with pytest.raises(pkg.DnaGpuError) as ei:
                ctx.names_take(none, [0])
            assert ei.value.code == BAD_ARG
        m = 4 * lds_segs + 77
        small = [random_name(rng, int(n)) for n in rng.integers(0, 3, size=m)]
        assert sum(len(x) for x in small) < 3 * tile and m > lds_segs
        ids = [int(x) for x in rng.integers(0, m, size=2 * m)]
        with ctx.names_upload(small) as nm:
            with ctx.names_take(nm, ids) as t:
                check_names(t, N.take(small, ids), "thousands of short names")
    finally:
        ar.free()


def make_table(ctx, records):
    words, starts = encode_table(records)
    d = ctx.upload(words, int(starts[-1]))
    d.set_sequences(starts)
    return d


IMAGE_SHAPES = [(FASTQ, 0), (FASTA, 0), (FASTA, 1), (FASTA, 60)]


@pytest.mark.gpu
@pytest.mark.parametrize("crlf", [False, True], ids=["lf", "crlf"])
@pytest.mark.parametrize("fmt,width", IMAGE_SHAPES, ids=[f"{'LAQ'[f - 1]}{w}" for f, w in IMAGE_SHAPES])
def test_named_image_formats_and_destination_offsets(ctx, dbg, pkg, fmt, width, crlf):
    """names of 0 .. 33 bytes and one longer than a tile of the image's sweep over sequences of 0 .. 65 bases: size, sequences,
    empties, record offsets, the whole image to host memory and to device memory at every destination offset 0 .. 15, partitions
    that tile, read_quals on it; the numbered image of the same table still equals export_model"""
    rng = np.random.default_rng(SEED + 16 * fmt + width + 1000 * crlf)
    G = pkg.text_out_geometry()
    seq_lengths = [5, 0, 1, 15, 16, 17, 0, 0, 33, 64, 65, 150, 2, 31]
    name_lengths = [3, 0, 1, 15, 16, 17, 31, 32, 33, G + 37, 0, 20, 1, 48]
    records = [random_seq(rng, n).decode() for n in seq_lengths]
    names = [random_name(rng, n, blanks=True) for n in name_lengths]
    quals = [random_qual(rng, n) for n in seq_lengths]
    d = make_table(ctx, records)
    ar = Arena(ctx, 1 << 18)
    opt = export_model.Options(fmt, crlf=crlf, line_width=width, quality=b"#")
    try:
        with ctx.names_upload(names) as nm, ctx.quals_upload(b"".join(quals)) as q:
            want = N.render_named(records, names, None, opt)
            pos = [0]
            for s in range(len(records)):
                pos.append(pos[-1] + len(N.render_named(records[s:s + 1], names[s:s + 1], None, opt)))
            with ctx.table_to_text_named(d, nm, fmt, crlf=crlf, line_width=width, quality=b"#") as img:
                assert (img.bytes, img.sequences, img.empty) == (len(want), len(records), 3)
                assert [int(x) for x in img.record_pos()] == pos
                got = img.read()
                if got != want:
                    at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
                    raise AssertionError(f"the image differs first at byte {at}: got {got[max(at - 8, 0):at + 24]!r} want "
                                         f"{want[max(at - 8, 0):at + 24]!r}")
                for off in range(16):
                    ar.reset()
                    p = ar.take("image", len(want), off)
                    img.read_device(0, len(want), p)
                    ar.check(f"destination offset {off}", {p: want})
                for step in (1000, G + 3):
                    assert b"".join(img.read(a, min(step, len(want) - a)) for a in range(0, len(want), step)) == want, step
                if fmt == FASTQ:
                    wq = N.render_named(records, names, quals, opt)
                    assert img.read_quals(q) == wq
                    assert b"".join(img.read_quals(q, a, min(777, len(wq) - a)) for a in range(0, len(wq), 777)) == wq
            # unchanged ground: the numbered image of the same table
            with ctx.table_to_text(d, fmt, crlf=crlf, line_width=width, prefix=b"r", name_base=9, quality=b"#") as img:
                assert img.read() == export_model.render(records, export_model.Options(fmt, crlf, width, b"r", 9, None, b"#"))
    finally:
        ar.free()
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,width,crlf", [(FASTQ, 0, True), (FASTA, 3, False)], ids=["fastq-crlf", "fasta3-lf"])
def test_named_image_every_window(ctx, dbg, pkg, fmt, width, crlf):
    """every window [a, b) of a small named image into device memory at every destination alignment 0 .. 15: the window's
    bytes are the image's, and no byte outside the window is touched (every window has a slot of its own in a block of
    sentinel bytes, which is read back once per alignment)"""
    rng = np.random.default_rng(SEED + 40 + fmt)
    records = [random_seq(rng, n).decode() for n in (4, 0, 1, 9)]
    names = [random_name(rng, n, blanks=True) for n in (17, 0, 1, 20)]
    opt = export_model.Options(fmt, crlf=crlf, line_width=width)
    want = np.frombuffer(N.render_named(records, names, None, opt), dtype=np.uint8)
    n = len(want)
    assert 60 <= n <= 140
    windows = [(a, b) for a in range(n + 1) for b in range(a, n + 1)]
    slot, lead = 256, 64
    assert lead + 15 + n <= slot
    d = make_table(ctx, records)
    base = ctx.buffer_alloc(slot * len(windows))
    clean = np.full(slot * len(windows), 0xC3, dtype=np.uint8)
    try:
        with ctx.names_upload(names) as nm, ctx.table_to_text_named(d, nm, fmt, crlf=crlf, line_width=width) as img:
            assert img.bytes == n
            for off in range(16):
                ctx.upload_bytes(base, clean)
                expect = clean.copy()
                for i, (a, b) in enumerate(windows):
                    at = i * slot + lead + off
                    img.read_device(a, b - a, base + at)
                    expect[at:at + b - a] = want[a:b]
                got = ctx.download_bytes(base, len(clean))
                bad = np.flatnonzero(got != expect)
                if len(bad):
                    i = int(bad[0]) // slot
                    raise AssertionError(f"alignment {off}, window {windows[i]}: byte {int(bad[0]) - i * slot - lead - off} of the "
                                         f"destination differs")
    finally:
        ctx.buffer_free(base)
        d.free()


@pytest.mark.gpu
def test_named_image_refusals(ctx, dbg, pkg):
    """a column of another sequence count, LINES, a non-empty stream without a set: BAD_ARG, *out untouched, nothing allocated;
    a table of no sequence with the column of no name: an image of 0 bytes"""
    d = make_table(ctx, ["ACGT", "GG"])
    bare = ctx.upload(encode_table(["ACGT"])[0], 4)
    try:
        with ctx.names_upload([b"a", b"b", b"c"]) as three, ctx.names_upload([b"a", b"b"]) as two, ctx.names_upload([]) as none:
            before = ctx.device_bytes()
            for table, nm, fmt in ((d, three, FASTQ), (d, none, FASTA), (d, two, LINES), (bare, two, FASTA)):
                with pytest.raises(pkg.DnaGpuError) as ei:
                    ctx.table_to_text_named(table, nm, fmt)
                assert ei.value.code == BAD_ARG
            assert ctx.device_bytes() == before
            with ctx.table_to_text_named(d, two, FASTA) as img:
                assert img.read() == b">a\nACGT\n>b\nGG\n"
            empty = ctx.dna_take(d, [])
            with ctx.table_to_text_named(empty, none, FASTQ) as img:
                assert img.bytes == 0 and img.read() == b""
            empty.free()
    finally:
        bare.free()
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("crlf", [False, True], ids=["lf", "crlf"])
def test_round_trip_byte_for_byte(ctx, dbg, pkg, crlf):
    """the test that states the feature.  A canonical FASTQ (bare '+', random names without CR / LF, lengths from EDGE_LENGTHS)
    loaded with reads_from_text + names_from_text + quals_from_fastq and written with table_to_text_named + read_quals is EQUAL
    TO THE INPUT BYTES; so is a FASTA at the input's line width.  After quals_trim, with its seg_first / seg_len into
    dna_gather / quals_gather and its seg_seq into names_take, the written file is the model's rendering of the surviving
    reads under their own names; the same ids through dna_take name the same table"""
    rng = np.random.default_rng(SEED + 60 + crlf)
    lengths = [int(x) for x in rng.permutation(EDGE_LENGTHS * 4 + [150] * 6)]
    seqs = [random_seq(rng, n) for n in lengths]
    quals = [bytes(rng.integers(33, 75, size=n, dtype=np.uint8)) for n in lengths]
    names = [random_name(rng, int(n), blanks=True) for n in rng.integers(0, 45, size=len(seqs))]
    text = fastq(names, seqs, quals, crlf)
    d, rep = ctx.reads_from_text(text, FASTQ, record_pos=True, source=True)
    nm = ctx.names_from_text(text, FASTQ, rep.record_pos, rep.src_record)
    q, _ = ctx.quals_from_fastq(text, d, rep.src_record, rep.src_offset)
    try:
        with ctx.table_to_text_named(d, nm, FASTQ, crlf=crlf) as img:
            assert img.read_quals(q) == text
            assert [int(x) for x in img.record_pos()[:-1]] == [int(x) for x in rep.record_pos]
        # FASTA at the input's line width
        ftext = fasta(names, seqs, 60, crlf)
        fd, frep = ctx.reads_from_text(ftext, FASTA, record_pos=True, source=True)
        with ctx.names_from_text(ftext, FASTA, frep.record_pos, frep.src_record) as fnm:
            with ctx.table_to_text_named(fd, fnm, FASTA, crlf=crlf, line_width=60) as img:
                assert img.read() == ftext
        fd.free()
        # trim, then the survivors under their own names
        col, starts = b"".join(quals), [int(x) for x in d.sequence_starts()]
        kw = dict(cut_front=20, cut_tail=20, min_bases=10, min_mean_q=18)
        want = Q.trim(col, starts, **kw)
        tr = ctx.quals_trim(d, q, **kw)
        assert [int(x) for x in tr.seg_seq] == want.seg_seq and 0 < tr.passed < len(seqs)
        t = ctx.dna_gather(d, tr.seg_first, tr.seg_len)
        qt = ctx.quals_gather(q, tr.seg_first, tr.seg_len)
        nt = ctx.names_take(nm, tr.seg_seq)
        cut = [(a - starts[s], n) for s, a, n in zip(want.seg_seq, want.seg_first, want.seg_len)]
        want_s = [seqs[s][a:a + n].decode() for s, (a, n) in zip(want.seg_seq, cut)]
        want_q = [quals[s][a:a + n] for s, (a, n) in zip(want.seg_seq, cut)]
        want_n = N.take(names, want.seg_seq)
        with ctx.table_to_text_named(t, nt, FASTQ, crlf=crlf) as img:
            assert img.read_quals(qt) == N.render_named(want_s, want_n, want_q, export_model.Options(FASTQ, crlf=crlf))
        for o in (t, qt, nt):
            o.free()
        # the same ids through the whole chain of takes: table, qualities, names
        ids = TAKE_IDS + want.seg_seq[::-1]
        t, qt, nt = ctx.dna_take(d, ids), ctx.quals_take(d, q, ids), ctx.names_take(nm, ids)
        check_table(t, [seqs[i].decode() for i in ids])
        with ctx.table_to_text_named(t, nt, FASTQ, crlf=crlf) as img:
            assert img.read_quals(qt) == fastq([names[i] for i in ids], [seqs[i] for i in ids], [quals[i] for i in ids], crlf)
        for o in (t, qt, nt):
            o.free()
    finally:
        for o in (q, nm, d):
            o.free()


# ------------------------------------------------------------------ the glue

@pytest.fixture(scope="module")
def g(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".glue")


def test_glue_names_surface_and_refusals(g):
    """the entry points exist; the host logic that needs no device: copy_reads_keep_names on a format without names and after
    a feed, named and unnamed adds in one handle, each with its message"""
    L = g.lib()
    for name in ("copy_reads_keep_names", "copy_reads_name", "copy_reads_to_add_named", "copy_dna_to_add_named"):
        assert hasattr(L, name)
    with pytest.raises(g.GlueError) as ei:
        g.copy_reads_named([], format=LINES)
    assert "only FASTA and FASTQ" in str(ei.value)
    c = L.copy_dna_begin(FASTA)                                      # a copy_dna handle is no copy_reads handle
    assert not L.copy_reads_keep_names(c, False) and "only FASTA and FASTQ" in str(g._err())
    L.copy_dna_end(c)
    c = L.copy_reads_begin(FASTQ, 0, 0, 0)
    try:
        n = C.c_size_t(7)
        assert L.copy_reads_name(c, C.byref(n)) is None and n.value == 0
        assert L.copy_dna_feed(c, b"@r", 2, False)                   # (two bytes: below every chunk size, nothing is loaded)
        assert not L.copy_reads_keep_names(c, False)
        assert "after the first bytes were fed" in str(g._err())
    finally:
        L.copy_dna_end(c)
    row = g.dna("ACGT")
    for first_named in (True, False):
        c = L.copy_reads_to_begin(False)
        try:
            add = lambda named: (L.copy_reads_to_add_named(c, row.p, b"n", 1, b"IIII", 4) if named else L.copy_reads_to_add(c, row.p, b"IIII", 4))
            assert add(first_named) and add(first_named)
            assert not add(not first_named)
            assert "rows with a name and rows without one" in str(g._err()) and L.copy_reads_to_failed(c)
        finally:
            L.copy_reads_to_end(c)
    c = L.copy_dna_to_begin(FASTA, 0, False)
    try:
        assert L.copy_dna_to_add_named(c, row.p, b"n", 1) and not L.copy_dna_to_add(c, row.p)
        assert "rows with a name and rows without one" in str(g._err())
    finally:
        L.copy_dna_to_end(c)
    c = L.copy_dna_to_begin(LINES, 0, False)
    try:
        assert not L.copy_dna_to_add_named(c, row.p, b"n", 1) and "has no names" in str(g._err())
    finally:
        L.copy_dna_to_end(c)


@pytest.mark.gpu
def test_glue_keeps_names_through_trim_and_write(ctx, dbg, g):
    """FASTQ chunks through trim_reads with copy_reads_keep_names at chunk sizes so small that records straddle chunks, the file
    fed whole and in pieces of 50 bytes: the rows, their qualities and their names equal the models'; written with
    copy_reads_to_add_named the output is the model's rendering and loads again to the same rows and names; copy_reads
    (FASTA, SPLIT) and copy_dna_to_add_named; a CR inside a name is the library's input error with its record"""
    rng = np.random.default_rng(SEED + 70)
    lengths = [60, 1, 33] + [int(n) for n in rng.integers(1, 120, size=25)]
    seqs = [random_seq(rng, n, b"ATCG" * 12 + b"N") for n in lengths]
    quals = [bytes(int(x) for x in np.clip(rng.integers(20, 75, size=n) - 14 * (np.arange(n) % 9 == 0), 33, 126)) for n in lengths]
    names = [random_name(rng, int(n), blanks=True) for n in rng.integers(0, 40, size=len(seqs))]
    text = fastq(names, seqs, quals)
    kw = dict(cut_front=25, cut_tail=25, min_bases=5)

    def model(first_word):
        p = reads_model.parse(text, reads_model.Options(format=FASTQ, ambiguous=2))
        starts = N.offsets_of(p.sequences)
        col = Q.column(text, [len(s) for s in p.sequences], p.src_record, p.src_offset)
        nm = N.names_of(text, FASTQ, p.pos, p.src_record, first_word)
        t = Q.trim(col, starts, **kw)
        return [(p.sequences[s][a - starts[s]:a - starts[s] + n], p.src_record[s], p.src_offset[s] + a - starts[s], col[a:a + n], nm[s])
                for s, a, n in zip(t.seg_seq, t.seg_first, t.seg_len)]

    try:
        for chunk in (16, 97, 64 << 20):
            g.set_copy_chunk_bytes(chunk)
            for pieces in ([text], [text[a:a + 50] for a in range(0, len(text), 50)]):
                for fw in (False, True):
                    want = model(fw)
                    rows, rec, off, qs, nms = g.trim_reads_named(pieces, first_word=fw, ambiguous=2, **kw)
                    assert [(str(r), a, b, q, n) for r, a, b, q, n in zip(rows, rec, off, qs, nms)] == want, (chunk, len(pieces), fw)
                    assert 0 < len(rows) == len(want)
            want = model(False)
            rows, rec, off, qs, nms = g.trim_reads_named([text], ambiguous=2, **kw)
            for crlf in (False, True):
                out = g.copy_reads_to_named(rows, nms, qs, crlf=crlf)
                assert out == N.render_named([w[0] for w in want], [w[4] for w in want], [w[3] for w in want],
                                             export_model.Options(FASTQ, crlf=crlf))
                back = g.trim_reads_named([out])
                assert [str(r) for r in back[0]] == [w[0] for w in want] and back[3] == [w[3] for w in want]
                assert back[4] == [w[4] for w in want]
            # FASTA through copy_reads under SPLIT, and back through copy_dna_to_add_named
            ftext = fasta(names, seqs, 60)
            p = reads_model.parse(ftext, reads_model.Options(format=FASTA, ambiguous=2))
            rows, rec, off, nms = g.copy_reads_named([ftext[a:a + 50] for a in range(0, len(ftext), 50)], format=FASTA, ambiguous=2)
            assert [str(r) for r in rows] == p.sequences and rec == p.src_record and nms == [names[r] for r in p.src_record]
            out = g.copy_dna_to_named(rows, nms, FASTA, 60)
            assert out == N.render_named(p.sequences, nms, None, export_model.Options(FASTA, line_width=60))
        g.set_copy_chunk_bytes(97)
        pos = positions(text, FASTQ)
        assert len(names[8]) >= 2 or len(names[9]) >= 2
        r = 8 if len(names[8]) >= 2 else 9
        bad = bytearray(text)
        bad[pos[r] + 1] = 0x0D
        with pytest.raises(g.GlueError) as ei:
            g.trim_reads_named([bytes(bad)], ambiguous=2)
        assert str(ei.value) == N.MSG_CHAR and ei.value.record == r
        with pytest.raises(g.GlueError) as ei:
            g.copy_reads_to_named([g.dna("ACGT"), g.dna("AC")], [b"fine", b"not\nfine"], [b"IIII", b"II"])
        assert str(ei.value) == N.MSG_CHAR
    finally:
        g.set_copy_chunk_bytes(64 << 20)
