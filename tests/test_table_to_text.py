"""dnagpu_table_to_text: a resident table written out as text, FASTA or FASTQ on the device, read window by window
(COPY dna_sequences (sequence) TO ...).

The reference of every comparison is tests/export_model.py: render() forms the image in a plain Python loop over records and
lines that states the contract of include/dnagpu.h and shares nothing with the C++.  The model itself is guarded by images
written out by hand and by the loaders' models (text_model.parse, reads_model.parse), which must read its images back.  Every
GPU test runs twice: as it is, and with poisoned, guarded pool buffers."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import export_model as M
import reads_model
import text_model
from __graft_entry__ import ROOT, load_package
from test_device_io import Arena
from test_dna_take import check_table, encode_table

BAD_ARG, TOO_LARGE = 5, 6
LINES, FASTA, FASTQ = M.LINES, M.FASTA, M.FASTQ
SEED = 0x7E88
U64_MAX = 2 ** 64 - 1
EDGE_LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65]
NUMBERS = [0, 9, 10, 99, 100, 10 ** 19, U64_MAX]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def g(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


def random_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ATCG", dtype=np.uint8), n)).decode() if n else ""


# ------------------------------------------------------------------ CPU: the reference itself

HAND = [
    # records, options, the image
    (["AT", "", "G"], M.Options(LINES), b"AT\n\nG\n"),
    (["AT", "", "G"], M.Options(LINES, crlf=True, prefix=b"x", name_base=5), b"AT\r\n\r\nG\r\n"),
    (["ATCGA", "", "G"], M.Options(FASTA, numbers=[0, 9, 10]), b">0\nATCGA\n>9\n>10\nG\n"),
    (["ATCGA", "", "G"], M.Options(FASTA, line_width=1, prefix=b"r"), b">r0\nA\nT\nC\nG\nA\n>r1\n>r2\nG\n"),
    (["ATCGA", "GG"], M.Options(FASTA, line_width=3, crlf=True, name_base=9), b">9\r\nATC\r\nGA\r\n>10\r\nGG\r\n"),
    (["ATCGA", "GGG"], M.Options(FASTA, line_width=3, numbers=[U64_MAX, 0]), b">18446744073709551615\nATC\nGA\n>0\nGGG\n"),
    (["ATCGA"], M.Options(FASTA, line_width=5), b">0\nATCGA\n"),
    (["ATCGA"], M.Options(FASTA, line_width=6, prefix=b"seq "), b">seq 0\nATCGA\n"),
    (["AT"], M.Options(FASTA, name_base=U64_MAX), b">18446744073709551615\nAT\n"),
    (["AT", "C"], M.Options(FASTA, name_base=U64_MAX), b">18446744073709551615\nAT\n>0\nC\n"),
    (["AT", "", "G"], M.Options(FASTQ, numbers=[9, 10, U64_MAX]),
     b"@9\nAT\n+\nII\n@10\n\n+\n\n@18446744073709551615\nG\n+\nI\n"),
    (["AT"], M.Options(FASTQ, crlf=True, prefix=b"read/", quality=b"#"), b"@read/0\r\nAT\r\n+\r\n##\r\n"),
]


def test_the_model_on_hand_written_images():
    """a guard on the reference itself, against images written out by hand.  It runs no code of the project."""
    for records, opt, image in HAND:
        assert M.render(records, opt) == image, (records, opt)
        pos = M.record_pos(records, opt)
        assert len(pos) == len(records) + 1 and pos[0] == 0 and pos[-1] == len(image)
        for s, at in enumerate(pos[:-1]):
            assert image[at:pos[s + 1]] == M.render_record(records[s], opt, s)
    assert M.empties(["AT", "", "G", ""]) == 2
    for records, opt, image in HAND:
        if len(records) == 1:
            n = len(records[0])
            assert M.size_of_one(n, opt) == len(image)
            for first in range(len(image)):
                for count in (1, 2, 5, len(image) - first):
                    if first + count <= len(image):
                        got = M.window_of_one(n, opt, first, count, lambda i, m: records[0][i:i + m])
                        assert got == image[first:first + count], (opt, first, count)


def test_the_model_through_the_loaders_models():
    """parse(render(records)) gives back the records and record_pos, for random records without empties.  It runs no code of
    the project."""
    rng = np.random.default_rng(SEED)
    for it in range(60):
        records = [random_seq(rng, int(n)) for n in rng.integers(1, 90, size=int(rng.integers(1, 12)))]
        crlf = bool(it & 1)
        numbers = [int(x) for x in rng.integers(0, 1 << 63, size=len(records), dtype=np.uint64)]
        for opt in (M.Options(LINES, crlf=crlf), M.Options(FASTA, crlf=crlf, line_width=int(rng.integers(0, 70)), prefix=b"r", numbers=numbers),
                    M.Options(FASTQ, crlf=crlf, prefix=b"read ", name_base=it)):
            image = M.render(records, opt)
            if opt.format == FASTQ:
                p = reads_model.parse(image, reads_model.Options(format=reads_model.FASTQ))
                got = p.sequences
            else:
                p = text_model.parse(image, opt.format)
                got = p.records
            assert p.error is None and got == records, opt
            assert p.pos == M.record_pos(records, opt)[:-1], opt


SANITIZERS = ["-g", "-Xarch_host", "-fsanitize=address,undefined"]


@pytest.mark.parametrize("extra", [[], SANITIZERS], ids=["plain", "sanitizers"])
def test_export_math_on_the_host(tmp_path, extra):
    """export_math.hpp, host code of the header the kernels share, as a stand-alone program (the second build with
    AddressSanitizer and UndefinedBehaviorSanitizer on it): hand-written and 50,000 random tables rendered byte by byte
    through the header's map from every offset of every record must agree with a naive writer inside the same program"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "export_math_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", *extra, "-I",
                           os.path.join(ROOT, "dna-sequences-pg-extension_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "export_math_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_export_argument_rules_without_a_device(pkg):
    """the checks that need no device, in their order -- the NULL rules, then the options -- with a context and a table that
    are never dereferenced, so none of them can have touched a device; *out left as it was; the window rules and the
    accessors on a NULL image"""
    L = pkg.lib()
    Opt = pkg.binding._TextOutOptionsC
    out = C.c_void_p(77)
    ctx, table = C.c_void_p(1), C.c_void_p(1)                                  # (never dereferenced below)
    call = L.dnagpu_table_to_text
    good = Opt(format=LINES)
    assert call(None, table, C.byref(good), C.byref(out)) == BAD_ARG
    assert call(ctx, None, C.byref(good), C.byref(out)) == BAD_ARG
    assert call(ctx, table, None, C.byref(out)) == BAD_ARG
    assert call(ctx, table, C.byref(good), None) == BAD_ARG
    bad = [Opt(format=0), Opt(format=4), Opt(format=-1), Opt(format=LINES, flags=2), Opt(format=FASTA, flags=3),
           Opt(format=FASTA, flags=0x80000000), Opt(format=FASTA, reserved=b"\0\0\1"), Opt(format=FASTA, reserved=b"\1"),
           Opt(format=FASTA, prefix_len=65, name_prefix=b"x" * 65), Opt(format=FASTA, prefix_len=1, name_prefix=None),
           Opt(format=FASTA, prefix_len=3, name_prefix=b"a\nb"), Opt(format=FASTQ, prefix_len=3, name_prefix=b"ab\r"),
           Opt(format=FASTQ, quality=b" "), Opt(format=FASTQ, quality=b"\x7f"), Opt(format=FASTQ, quality=b"\xff"),
           Opt(format=LINES, line_width=60), Opt(format=FASTQ, line_width=1)]
    C.memmove(C.addressof(bad[6]) + Opt.reserved.offset + 2, b"\1", 1)         # (a char array is set up to its first NUL)
    for o in bad:
        assert call(ctx, table, C.byref(o), C.byref(out)) == BAD_ARG, [getattr(o, f[0]) for f in Opt._fields_]
        assert call(None, table, C.byref(o), C.byref(out)) == BAD_ARG           # the NULL before the options
    assert out.value == 77
    buf = C.create_string_buffer(8)
    pos = (C.c_uint64 * 1)(9)
    assert L.dnagpu_text_image_bytes(None) == 0 and L.dnagpu_text_image_sequences(None) == 0 and L.dnagpu_text_image_empty(None) == 0
    for count in (0, 1):                                                       # a NULL image has no window
        assert L.dnagpu_text_image_read(ctx, None, 0, count, buf, 0) == BAD_ARG
        assert L.dnagpu_text_image_record_pos(ctx, None, 0, count, pos, 0) == BAD_ARG
    assert pos[0] == 9 and buf.raw == b"\0" * 8
    L.dnagpu_text_image_free(ctx, None)
    L.dnagpu_text_image_free(None, None)
    assert L.dnagpu_text_out_geometry(None) == BAD_ARG


def test_export_binding_surface(pkg):
    assert pkg.abi_version() == 2
    assert pkg.TEXT_OUT_CRLF == 1
    t = pkg.text_out_geometry()
    assert t >= 16 and t % 16 == 0
    assert callable(pkg.Context.table_to_text)
    for name in ("bytes", "sequences", "empty", "read", "read_device", "record_pos", "free"):
        assert hasattr(pkg.TextImage, name)
    assert C.sizeof(pkg.binding._TextOutOptionsC) == 48


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


@pytest.fixture(scope="module")
def G(pkg):
    return pkg.text_out_geometry()


def make_table(ctx, records):
    """the resident table of records (str each; some, not all, may be empty)"""
    words, starts = encode_table(records)
    d = ctx.upload(words, int(starts[-1]))
    d.set_sequences(starts)
    return d


def model_options(fmt, kw):
    numbers = kw.get("numbers")
    return M.Options(fmt, crlf=kw.get("crlf", False), line_width=kw.get("line_width", 0), prefix=kw.get("prefix", b""),
                     name_base=kw.get("name_base", 0), numbers=None if numbers is None else [int(x) for x in numbers],
                     quality=kw.get("quality", b"I"))


def check_image(ctx, d, records, fmt, what="", arena=None, offsets=(), **kw):
    """the image of d under the options against the model's: size, sequences, empties, record offsets and the whole image in
    host memory; arena: also into device memory at every destination offset of `offsets`, nothing written beside it.
    -> the model's image"""
    opt = model_options(fmt, kw)
    want = M.render(records, opt)
    what = f"{what} format={fmt} {kw if len(str(kw)) < 200 else sorted(kw)}"
    with ctx.table_to_text(d, fmt, **kw) as img:
        assert (img.bytes, img.sequences, img.empty) == (len(want), len(records), M.empties(records)), what
        assert np.array_equal(img.record_pos(), np.array(M.record_pos(records, opt), dtype=np.uint64)), what
        got = img.read()
        if got != want:
            at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
            raise AssertionError(f"{what}: the image differs first at byte {at}: got {got[max(at - 8, 0):at + 24]!r} want "
                                 f"{want[max(at - 8, 0):at + 24]!r}")
        for off in offsets:
            arena.reset()
            p = arena.take("image", len(want), off)
            img.read_device(0, len(want), p)
            arena.check(f"{what} destination offset {off}", {p: want})
    return want


def edge_records(rng):
    """sequences of 0 (singly and in runs of three), 1, 15, .. 65 bases, each twice, in random order"""
    groups = [[n] for n in EDGE_LENGTHS * 2] + [[0], [0, 0, 0]]
    order = rng.permutation(len(groups))
    lengths = [5] + [n for i in order for n in groups[i] + [7]][:-1] + [0, 0, 0, 9, 0]     # (the 7s keep the runs apart)
    return [random_seq(rng, n) for n in lengths]


def edge_numbers(rng, n):
    numbers = np.array([NUMBERS[i % len(NUMBERS)] for i in range(n)], dtype=np.uint64)
    return numbers[rng.permutation(n)]


SHAPES = [(LINES, 0), (FASTQ, 0)] + [(FASTA, w) for w in (0, 1, 7, 16, 60, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("crlf", [False, True], ids=["lf", "crlf"])
@pytest.mark.parametrize("fmt,width", SHAPES, ids=[f"{'LAQ'[f - 1]}{w}" for f, w in SHAPES])
def test_formats_widths_and_destination_offsets(ctx, dbg, fmt, width, crlf):
    """every format, terminator and FASTA width over sequences of 0 .. 65 bases with the numbers 0, 9, 10, 99, 100, 10^19 and
    2^64 - 1: the whole image to host memory and to device memory at every destination offset 0 .. 15, where nothing but the
    image's bytes may change"""
    rng = np.random.default_rng(SEED + 16 * fmt + width + 1000 * crlf)
    records = edge_records(rng)
    assert M.empties(records) >= 4
    d = make_table(ctx, records)
    ar = Arena(ctx, 1 << 14)
    try:
        numbers = edge_numbers(rng, len(records))
        want = check_image(ctx, d, records, fmt, arena=ar, offsets=range(16), crlf=crlf, line_width=width, prefix=b"read_",
                           numbers=numbers, quality=b"#")
        assert 0xC3 not in want
        # the numbers from device memory; then no numbers: name_base + s wraps at 2^64; no prefix
        ar.reset()
        nd = ar.take("numbers", 8 * len(numbers), 0, numbers)
        with ctx.table_to_text(d, fmt, crlf=crlf, line_width=width, prefix=b"read_", numbers=int(nd), quality=b"#") as img:
            assert img.read() == want
        ar.check("numbers in device memory")
        check_image(ctx, d, records, fmt, crlf=crlf, line_width=width, name_base=U64_MAX - 3)
    finally:
        ar.free()
        d.free()


@pytest.mark.gpu
def test_windows(ctx, dbg, pkg, G):
    """every first byte 0 .. 40 with counts 0, 1, 15, 16, 17, 33; windows that end 0 .. 17 bytes before the end; partitions
    into windows of 1, 1000 and G + 3 bytes concatenate to the image; the window rules"""
    rng = np.random.default_rng(SEED + 50)
    records = edge_records(rng)
    d = make_table(ctx, records)
    kw = dict(crlf=True, line_width=7, prefix=b"w", name_base=98)
    want = M.render(records, model_options(FASTA, kw))
    ar = Arena(ctx, 1 << 14)
    try:
        with ctx.table_to_text(d, FASTA, **kw) as img:
            n = img.bytes
            assert n == len(want)
            for first in range(41):
                for count in (0, 1, 15, 16, 17, 33):
                    assert img.read(first, count) == want[first:first + count], (first, count)
            for back in range(18):
                assert img.read(5, n - 5 - back) == want[5:n - back], back
                assert img.read(n - back, back) == want[n - back:], back
            for first, count, off in ((3, 1, 15), (3, 2, 15), (17, 14, 1), (1, 31, 1), (6, 40, 9), (n - 3, 3, 13), (n, 0, 5)):
                ar.reset()
                p = ar.take("window", max(count, 1), off)
                img.read_device(first, count, p)
                ar.check(f"window {first}+{count} at destination offset {off}", {p: want[first:first + count]})
            assert b"".join(img.read(i, 1) for i in range(n)) == want
            for first, count in ((n + 1, 0), (0, n + 1), (n, 1), (1, n), (U64_MAX, 1), (2, U64_MAX)):
                with pytest.raises(pkg.DnaGpuError) as ei:             # (refused before anything is written)
                    img.read_device(first, count, ar.base)
                assert ei.value.code == BAD_ARG, (first, count)
            pos = img.record_pos()
            assert np.array_equal(img.record_pos(3, 4), pos[3:7]) and len(img.record_pos(len(pos), 0)) == 0
            for first, count in ((len(pos) + 1, 0), (1, len(pos))):
                with pytest.raises(pkg.DnaGpuError) as ei:
                    img.record_pos(first, count)
                assert ei.value.code == BAD_ARG
    finally:
        ar.free()
        d.free()
    records = [random_seq(rng, n) for n in (50, 3 * G + 5, 1, 700)]
    d = make_table(ctx, records)
    try:
        for fmt, kw in ((FASTA, dict(line_width=60, prefix=b"chr")), (FASTQ, dict(crlf=True)), (LINES, {})):
            want = M.render(records, model_options(fmt, kw))
            with ctx.table_to_text(d, fmt, **kw) as img:
                for step in (1000, G + 3):
                    got = b"".join(img.read(a, min(step, len(want) - a)) for a in range(0, len(want), step))
                    assert got == want, (fmt, step)
    finally:
        d.free()


@pytest.mark.gpu
def test_tile_and_chunk_edges(ctx, dbg, pkg, G):
    """record boundaries, a CRLF pair, a 20-digit number and a 64-byte prefix across the boundaries of the tiles one workgroup
    forms and of the 16-byte chunks one lane forms; a sequence of 3G + 5 bases; records that outnumber the chunks; images of
    exactly G - 1, G and G + 1 bytes, of 0 sequences, and of one base"""
    rng = np.random.default_rng(SEED + 60)
    b = lambda n: random_seq(rng, n)
    prefix = bytes(rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz_/ |", dtype=np.uint8), 64))
    top = np.array([U64_MAX, 10 ** 19, U64_MAX - 1], dtype=np.uint64)
    cases = {
        "a record begins at G - 1": ([b(G - 2), b(40)], LINES, {}),
        "a record begins at G": ([b(G - 1), b(40)], LINES, {}),
        "a record begins at G + 1": ([b(G), b(40)], LINES, {}),
        "crlf across the tile boundary": ([b(G - 1), b(40)], LINES, dict(crlf=True)),
        "crlf last in the tile": ([b(G - 2), b(7)], LINES, dict(crlf=True)),
        "crlf across a chunk": ([b(15), b(14), b(31), b(5)], LINES, dict(crlf=True)),
        # record 0 is '>' + 64 + 20 + T + bases + T: record 1's header lies across the boundary, its prefix or its digits on it
        "a 64-byte prefix across the tile boundary": ([b(G - 40 - 87), b(50), b(3)], FASTA, dict(prefix=prefix, numbers=top)),
        "a 20-digit number across the tile boundary": ([b(G - 75 - 87), b(50), b(3)], FASTA, dict(prefix=prefix, numbers=top)),
        "a header across the tile boundary, FASTQ": ([b((G - 75 - 91) // 2), b(50), b(3)], FASTQ, dict(prefix=prefix, numbers=top, crlf=True)),
        "3G + 5 bases at width 60": ([b(9), b(3 * G + 5), b(33)], FASTA, dict(line_width=60)),
        "3G + 5 bases at width 60, crlf": ([b(9), b(3 * G + 5), b(33)], FASTA, dict(line_width=60, crlf=True)),
        "3G + 5 bases on one line": ([b(9), b(3 * G + 5), b(33)], FASTA, dict(line_width=0)),
        "3G + 5 bases, FASTQ": ([b(3 * G + 5), b(33)], FASTQ, {}),
        "3G + 5 bases, LINES": ([b(3 * G + 5)], LINES, {}),
        "5000 one-base sequences, LINES": ([b(1) for _ in range(5000)], LINES, {}),
        "5000 one-base sequences, FASTA": ([b(1) for _ in range(5000)], FASTA, dict(line_width=60)),
        "5000 one-base sequences, FASTQ": ([b(1) for _ in range(5000)], FASTQ, dict(crlf=True)),
        "20000 one-base sequences, LINES": ([b(1) for _ in range(20000)], LINES, {}),
        "empties that outnumber the chunks": ([b(1)] + [""] * 9000 + [b(2)], LINES, {}),
        "G - 1 bytes": ([b(G - 2)], LINES, {}),
        "G bytes": ([b(G - 1)], LINES, {}),
        "G + 1 bytes": ([b(G)], LINES, {}),
        "one base": ([b(1)], LINES, {}),
        "one base, FASTQ": ([b(1)], FASTQ, {}),
    }
    ar = Arena(ctx, 8 * G)
    try:
        for what, (records, fmt, kw) in cases.items():
            d = make_table(ctx, records)
            try:
                check_image(ctx, d, records, fmt, what, arena=ar, offsets=(0, 5), **kw)
            finally:
                d.free()
        # 0 sequences: an image of 0 bytes that holds no device memory
        d = make_table(ctx, [b(4)])
        none = ctx.dna_take(d, [])
        before = ctx.device_bytes()
        for fmt in (LINES, FASTA, FASTQ):
            with ctx.table_to_text(none, fmt) as img:
                assert (img.bytes, img.sequences, img.empty) == (0, 0, 0)
                assert img.read() == b"" and len(img.record_pos()) == 0
                assert ctx.device_bytes() == before
                with pytest.raises(pkg.DnaGpuError):
                    img.read(0, 1)
        none.free()
        d.free()
    finally:
        ar.free()


@pytest.mark.gpu
def test_round_trip_on_the_device(ctx, dbg, pkg):
    """for tables without empties the image, read into a device buffer and handed to the loaders, gives the table back, and
    the loader's record offsets are the image's; a canonical text loaded and written with the same options is the text"""
    rng = np.random.default_rng(SEED + 70)
    records = [random_seq(rng, int(n)) for n in list(rng.integers(1, 400, size=300)) + EDGE_LENGTHS]
    d = make_table(ctx, records)
    n = len(records)
    try:
        for fmt, kw in ((LINES, {}), (LINES, dict(crlf=True)), (FASTA, dict(line_width=60, prefix=b"r")),
                        (FASTA, dict(line_width=0, crlf=True, numbers=edge_numbers(rng, n))), (FASTA, dict(line_width=1)),
                        (FASTQ, dict(prefix=b"read.")), (FASTQ, dict(crlf=True, quality=b"~"))):
            with ctx.table_to_text(d, fmt, **kw) as img:
                size = img.bytes
                buf = ctx.buffer_alloc(size + 1 + 8 * (n + 1))
                pos_dev = (buf + size + 1 + 7) & ~7
                try:
                    img.read_device(0, size, buf + 1)
                    if fmt == FASTQ:
                        back, rep = ctx.reads_from_text_device(buf + 1, size, pkg.TEXT_FASTQ, dev_record_pos=pos_dev, record_cap=n)
                    else:
                        back, rep = ctx.table_from_text_device(buf + 1, size, fmt, False, pos_dev, n)
                    check_table(back, records, f"round trip {fmt} {sorted(kw)}")
                    assert rep.records == n
                    assert np.array_equal(ctx.download_u64(pos_dev, n), img.record_pos()[:-1]), (fmt, kw)
                    back.free()
                finally:
                    ctx.buffer_free(buf)
    finally:
        d.free()
    # text -> table -> text
    lines = b"".join(r.encode() + b"\n" for r in records)
    fasta = b"".join(b">r%d\n" % s + b"".join(r.encode()[a:a + 60] + b"\n" for a in range(0, len(r), 60)) for s, r in enumerate(records))
    fastq = b"".join(b"@%d\n%s\n+\n%s\n" % (s + 7, r.encode(), b"I" * len(r)) for s, r in enumerate(records))
    for text, fmt, kw in ((lines, LINES, {}), (fasta, FASTA, dict(line_width=60, prefix=b"r")), (fastq, FASTQ, dict(name_base=7))):
        t, _ = ctx.reads_from_text(text, fmt) if fmt == FASTQ else ctx.table_from_text(text, fmt)
        with ctx.table_to_text(t, fmt, **kw) as img:
            assert img.empty == 0 and img.read() == text, fmt
        t.free()


@pytest.mark.gpu
def test_the_tables_edges(ctx, dbg, pkg):
    """a result of dnagpu_dna_take with flips (empties among its sequences); a dnagpu_dna_wrap view in the middle of an arena,
    non-zero bits behind its last base and a sentinel behind its words; a non-empty stream without a set"""
    rng = np.random.default_rng(SEED + 80)
    records = [random_seq(rng, n) for n in (33, 1, 64, 17, 100, 31)]
    d = make_table(ctx, records)
    comp = str.maketrans("ATCG", "TAGC")
    ids = [5, 0, 0, 3, 2, 4, 1, 1]
    flip = [1, 0, 1, 0, 1, 1, 0, 1]
    taken = ctx.dna_take(d, ids, flip)
    want = [records[i][::-1].translate(comp) if f else records[i] for i, f in zip(ids, flip)]
    try:
        for fmt, kw in ((LINES, {}), (FASTA, dict(line_width=16, numbers=np.array(ids, dtype=np.uint64))), (FASTQ, dict(crlf=True))):
            check_image(ctx, taken, want, fmt, "take", **kw)
    finally:
        taken.free()
    bare = ctx.upload(encode_table(records)[0], sum(map(len, records)))
    with pytest.raises(pkg.DnaGpuError) as ei:                   # a non-empty stream without a set
        ctx.table_to_text(bare, LINES)
    assert ei.value.code == BAD_ARG
    bare.free()
    d.free()
    # the view: 3 words of which the last holds 5 bases and, behind them, ones
    records = [random_seq(rng, n) for n in (20, 0, 30, 19)]
    words, starts = encode_table(records)
    words = words[:3].copy()
    words[2] |= np.uint64(U64_MAX) << np.uint64(10)
    ar = Arena(ctx, 1 << 16)
    try:
        w = ar.take("words", 24, 0, words)
        view = ctx.wrap(w, 3, 69)
        view.set_sequences(starts)
        written = {}
        for fmt, kw in ((LINES, {}), (FASTA, dict(line_width=7)), (FASTQ, {})):
            want = M.render(records, model_options(fmt, kw))
            with ctx.table_to_text(view, fmt, **kw) as img:
                assert img.empty == 1 and img.read() == want, fmt
                p = ar.take(f"image {fmt}", len(want), 3)
                img.read_device(0, len(want), p)
                written[p] = want
                ar.check(f"view, format {fmt}", written)         # the words unchanged, nothing written beside the images
        view.free()
    finally:
        ar.free()


@pytest.mark.gpu
def test_offsets_beyond_32_bits_and_the_extras_bound(ctx, dbg, pkg):
    """one sequence of 2^31 bases: as FASTA of width 1 with CRLF its extras are 2^32 + 4 -- DNAGPU_ERR_TOO_LARGE with nothing
    left allocated --; with LF the image has 2^32 + 3 bytes, and windows of 4096 bytes at its start, around 2^32 - 2048 and at
    its very end are the model's.  The model reads its bases through dnagpu_dna_unpack."""
    n = 1 << 31
    d = ctx.synth(0xD1CE, n)
    d.set_sequences(np.array([0, n], dtype=np.uint64))
    try:
        before = ctx.device_bytes()
        with pytest.raises(pkg.DnaGpuError) as ei:
            ctx.table_to_text(d, FASTA, line_width=1, crlf=True)
        assert ei.value.code == TOO_LARGE
        assert ctx.device_bytes() == before
        opt = M.Options(FASTA, line_width=1)
        size = M.size_of_one(n, opt)
        assert size == (1 << 32) + 3
        blocks = {}

        def bases(i, m):                                         # through dnagpu_dna_unpack, 8192 bases at a time
            a = i & ~8191
            if a not in blocks:
                blocks[a] = ctx.unpack(d, a, min(8192, n - a))
            assert i - a + m <= len(blocks[a])
            return blocks[a][i - a:i - a + m]
        with ctx.table_to_text(d, FASTA, line_width=1) as img:
            assert img.bytes == size and img.empty == 0
            assert [int(x) for x in img.record_pos()] == [0, size]
            for first in (0, (1 << 32) - 2048 - 2048, (1 << 32) - 2048 - 4096 - 7, size - 4096):     # (4096 bytes around 2^32 - 2048)
                assert img.read(first, 4096) == M.window_of_one(n, opt, first, 4096, bases), first
        # a wide line pitch, and FASTQ, whose quality line lies beyond 2^31
        for fmt, kw in ((FASTA, dict(line_width=(1 << 30) + 1, crlf=True, prefix=b"chr")), (FASTQ, {}), (LINES, {})):
            opt = model_options(fmt, kw)
            size = M.size_of_one(n, opt)
            with ctx.table_to_text(d, fmt, **kw) as img:
                assert img.bytes == size
                for first in (0, (1 << 30) - 100, min((1 << 31) - 2000, size - 4096 - 5), size - 4096):
                    assert img.read(first, 4096) == M.window_of_one(n, opt, first, 4096, bases), (fmt, first)
    finally:
        d.free()


@pytest.mark.gpu
def test_glue_copy_to(ctx, dbg, g):
    """COPY ... TO through the glue: ~300 rows of mixed lengths in each format, with a chunk size small enough to force
    several flushes and several output chunks, equal the model; COPY ... FROM of that output gives the rows back"""
    rng = np.random.default_rng(SEED + 90)
    texts = [random_seq(rng, int(n)) for n in list(rng.integers(1, 500, size=290)) + EDGE_LENGTHS]
    rows = [g.dna(t) for t in texts]
    g.set_copy_chunk_bytes(4096)
    try:
        for fmt, kw in ((LINES, {}), (FASTA, dict(line_width=60)), (FASTA, dict(line_width=0, crlf=True)), (FASTQ, {}), (LINES, dict(crlf=True))):
            out = g.copy_dna_to(rows, fmt, **kw)
            assert out == M.render(texts, model_options(fmt, kw)), (fmt, kw)
            back = g.copy_reads([out], fmt)[0] if fmt == FASTQ else g.copy_dna([out], fmt)[0]
            assert [str(r) for r in back] == texts, fmt
    finally:
        g.set_copy_chunk_bytes(64 << 20)


def test_glue_copy_to_surface_and_refusals(g):
    """the COPY ... TO entry points exist; a format outside 1 .. 3 is refused with a message, before any device is touched"""
    L = g.lib()
    for name in ("copy_dna_to_begin", "copy_dna_to_add", "copy_dna_to_finish", "copy_dna_to_next", "copy_dna_to_failed", "copy_dna_to_end"):
        assert hasattr(L, name)
    for fmt in (0, 4):
        with pytest.raises(g.GlueError) as ei:
            g.copy_dna_to([], fmt)
        assert "format" in str(ei.value)
    L.copy_dna_to_end(None)
