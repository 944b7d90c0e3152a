"""dnagpu_dna_adapters (include/dnagpu.h) through the C-ABI against the plain-Python model of its contract
(tests/adapters_model.py): every per-segment output, the passing lists and the whole report must be equal.  The hand-written
vectors of the model and the host check of adapters_math.hpp are in tests/test_adapters_model.py."""
import ctypes as C

import numpy as np
import pytest

import adapters_model as am
from __graft_entry__ import load_package
from test_device_io import Arena
from test_dna_take import resident, upload_text

SEED = 20251
TRUSEQ = "GATCGGAAGAGCACACGTCT"           # 20 letters; 'G' at 0, 4, 5, 8, 10 of the first eleven
SECOND = "GTCTCTTATACACATCTGAC"
PER = ("out_len", "out_adapter", "out_mismatch")
PASS = ("pass_seq", "pass_first", "pass_len")
SCALARS = ("segments", "passed", "trimmed", "bases_in", "bases_kept", "bases_cut", "failed_short", "failed_discarded")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["plain", "poison"])
def dbg(request, ctx, pkg):
    """every test once as it is and once with poisoned, guarded pool buffers; the guard bands are checked afterwards"""
    ctx.set_debug(pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL if request.param == "poison" else 0)
    yield request.param
    assert pkg.lib().dnagpu_synchronize(ctx.h) == 0
    ctx.set_debug(0)


def rand_text(rng, n, letters="ATCG"):
    return "".join(letters[i] for i in rng.integers(0, len(letters), size=n))


def starts_of(texts):
    return [int(x) for x in np.cumsum([0] + [len(t) for t in texts])]


def report_of(got):
    return dict({f: getattr(got, f) for f in SCALARS}, per_adapter=got.per_adapter)


def assert_equal(want, got, what):
    for f in PER + PASS:
        w, g = getattr(want, f), [int(x) for x in getattr(got, f)]
        if w != g:
            at = next((i for i in range(min(len(w), len(g))) if w[i] != g[i]), -1)
            raise AssertionError(f"{what}: {f} has {len(g)} entries, want {len(w)}; first difference at {at}: "
                                 f"{g[at] if 0 <= at < len(g) else None}, want {w[at] if 0 <= at < len(w) else None}")
    assert report_of(got) == want.report, what


_MEMO = {}                                # (adapters, err, min_overlap) -> {bases: cut}: the model runs once per distinct segment


def check(ctx, d, stream, first, length, adapters, what="", table=False, **opt):
    """the device over the segments -- table: with both lists NULL, the segments being the table's sequences -- against the
    model; -> the model's result"""
    memo = _MEMO.setdefault((tuple(adapters), opt.get("err", (0, 1)), opt.get("min_overlap", 1)), {})
    want = am.trim(stream, first, length, adapters, memo=memo, **opt)
    got = ctx.dna_adapters(d, adapters, None if table else first, None if table else length, **opt)
    assert_equal(want, got, f"{what} {opt}")
    assert want.report["bases_in"] == want.report["bases_kept"] + want.report["bases_cut"]
    return want


# ------------------------------------------------------------------ no device

def test_symbols_geometry_and_refusals_without_a_device(pkg):
    L = pkg.lib()
    g, w, t = pkg.adapters_geometry()
    assert 0 < g < w < t and g % 16 == 0
    assert L.dnagpu_adapters_geometry(None, None, None) == am.BAD_ARG
    ads = (C.c_char_p * 1)(b"ACGT")
    assert L.dnagpu_dna_adapters(None, None, ads, 1, None, None, None, None, 0, 0, None, None, None, None, None, None, 0, 0, None) == am.BAD_ARG


# ------------------------------------------------------------------ GPU

@pytest.mark.gpu
def test_every_stream_alignment(ctx, dbg, pkg):
    """reads of 0 .. 70 bases back to back, so that the reads start at all 32 base offsets of a word; adapters of 1, 31 and 32
    letters; full and end-clipped adapters planted; the last read ends with a hit at its last position, and the stream ends
    there with no word behind it.  Reads hold no G and every adapter begins with one, so only planted hits are exact."""
    rng = np.random.default_rng(SEED)
    ad1, ad31, ad32 = "G", "G" + rand_text(rng, 30), "G" + rand_text(rng, 31)
    reads = []
    for n in range(71):
        r = rand_text(rng, n, "ATC")
        kind = n % 4
        if kind == 1 and n > 40:                                   # a whole adapter inside
            at = int(rng.integers(0, n - 32))
            r = r[:at] + ad32 + r[at + 32:]
        elif kind == 2 and n > 12:                                 # an end-clipped one
            k = int(rng.integers(2, 12))
            r = r[:n - k] + ad31[:k]
        elif kind == 3 and n > 35:                                 # a whole one with two substitutions
            at = int(rng.integers(0, n - 31))
            bad = list(ad31)
            bad[7], bad[19] = "A" if bad[7] != "A" else "T", "A" if bad[19] != "A" else "T"
            r = r[:at] + "".join(bad) + r[at + 31:]
        reads.append(r)
    reads[70] = rand_text(rng, 69, "ATC") + "G"                   # the stream's last base: the read's only hit, of overlap 1
    starts = starts_of(reads)
    assert {s % 32 for s in starts[:-1]} == set(range(32))
    stream = "".join(reads)
    assert len(stream) % 32 != 0
    first, length = starts[:-1], [len(r) for r in reads]
    d = resident(ctx, reads)
    try:
        for adapters in ([ad31, ad32, ad1], [ad32], [ad31]):
            for err in ((0, 1), (1, 10)):
                for mo in (1, 3):
                    for table in (False, True):
                        w = check(ctx, d, stream, first, length, adapters, "alignments", table=table, err=err, min_overlap=mo)
                    if mo == 1:
                        assert w.out_len[70] == 69 and w.out_mismatch[70] == 0
        w = check(ctx, d, stream, first, length, [ad31, ad32, ad1], "alignments", err=(1, 10), min_overlap=1)
        assert w.out_adapter[70] == 0 and 0 < w.report["trimmed"] < 71 and min(w.report["per_adapter"][:3]) > 0
    finally:
        d.free()


@pytest.mark.gpu
def test_neighbours(ctx, dbg, pkg):
    """a read that ends with the first 5 letters of the adapter while the next read begins with the rest: the cut is the
    partial one, judged on 5 bases alone; the same with one substitution among the 5, which is no hit at 1/10 although the 13
    letters across the boundary would be; then the same boundaries made by segment lists that cut one read inside a planted
    adapter"""
    rng = np.random.default_rng(SEED + 1)
    ad = "GATCGGAAGAGCA"                                          # 13 letters
    sub = "GATAG"                                                 # ad[:5] with letter 3 substituted
    reads = []
    for i in range(40):
        body = rand_text(rng, int(rng.integers(20, 90)), "ATC")
        tail = (ad[:5], sub, "")[i % 3]
        head = ad[5:] if i % 3 != 0 or i % 2 else ""               # the read behind: the rest of the adapter, or its own bases
        reads.append(body + tail)
        reads.append(head + rand_text(rng, int(rng.integers(0, 50)), "ATC"))
    stream, starts = "".join(reads), starts_of(reads)
    first, length = starts[:-1], [len(r) for r in reads]
    d = resident(ctx, reads)
    try:
        for err in ((0, 1), (1, 10), (1, 5)):
            for table in (False, True):
                w = check(ctx, d, stream, first, length, [ad], "neighbours", table=table, err=err, min_overlap=3)
            for i in range(0, 80, 2):
                n = length[i]
                if (i // 2) % 3 == 0:
                    assert (w.out_len[i], w.out_mismatch[i], w.out_adapter[i]) == (n - 5, 0, 0), (err, i)
                elif (i // 2) % 3 == 1 and err != (1, 5):
                    assert w.out_len[i] == n, (err, i)                 # 1 mismatch in 5 bases; in 13 it would have been a hit
                elif (i // 2) % 3 == 1:
                    assert (w.out_len[i], w.out_mismatch[i]) == (n - 5, 1), (err, i)
        # one long read with whole adapters planted, cut by lists inside them: 5 letters before the boundary, 8 behind
        body = list(rand_text(rng, 900, "ATC"))
        at = [60, 200, 333, 471, 640, 801]
        for a in at:
            body[a:a + 13] = ad
        long_read = "".join(body)
        cuts = [0] + [a + 5 for a in at] + [900]
        d2 = upload_text(ctx, long_read)
        try:
            for err in ((0, 1), (1, 10)):
                w = check(ctx, d2, long_read, cuts[:-1], [b - a for a, b in zip(cuts[:-1], cuts[1:])], [ad], "lists", err=err,
                          min_overlap=3)
                assert w.out_len[:6] == [b - a - 5 for a, b in zip(cuts[:6], cuts[1:7])] and w.out_mismatch[:6] == [0] * 6
                assert w.out_len[6] == 900 - cuts[6]                   # the last piece begins with the rest of an adapter: no hit
        finally:
            d2.free()
    finally:
        d.free()


@pytest.mark.gpu
def test_path_edges(ctx, dbg, pkg):
    """segments of group_bases, wave_bases and tile_bases bases and one more, and of 3 tile_bases + 5: the only hit at the last
    position; a hit whose window straddles two lanes' chunks; one whose window straddles two tiles; a hit with one mismatch in
    tile 0 and an exact one in tile 2, where tile 0's wins"""
    rng = np.random.default_rng(SEED + 2)
    g, w, t = pkg.adapters_geometry()
    adapters = [TRUSEQ, SECOND]
    one_off = TRUSEQ[:9] + ("A" if TRUSEQ[9] != "A" else "T") + TRUSEQ[10:]
    reads, expect = [], []

    def add(n, plants, want):
        body = list(rand_text(rng, n, "ATC"))
        for p, text in plants:
            body[p:p + len(text)] = text
        assert len(body) == n
        reads.append("".join(body))
        expect.append(want)

    for n in (g, g + 1, w, w + 1, t, t + 1, 3 * t + 5):
        add(n, [], (n, am.NO_ADAPTER, 0))
        add(n, [(n - 1, "G")], (n - 1, 0, 0))                      # overlap 1 at the last position
        add(n, [(n - 7, SECOND[:7])], (n - 7, 1, 0))               # end-clipped
        for p in (9, (n // 2 // 16) * 16 - 7):                     # the window lies in two lanes' chunks
            add(n, [(p, TRUSEQ)], (p, 0, 0))
        add(n, [(n - 26, one_off)], (n - 26, 0, 1))
        if n > t:
            add(n, [(t - 7, SECOND[:n - (t - 7)])], (t - 7, 1, 0))  # the window lies in tiles 0 and 1 (clipped by the end at t + 1)
            add(n, [(n - 20, TRUSEQ)], (n - 20, 0, 0))             # the last tile's only hit
        if n > 2 * t:
            add(n, [(2 * t - 3, TRUSEQ)], (2 * t - 3, 0, 0))       # tiles 1 and 2
            add(n, [(100, one_off), (2 * t + 50, TRUSEQ)], (100, 0, 1))
            add(n, [(t + 100, one_off), (2 * t + 50, SECOND)], (t + 100, 0, 1))
    stream, starts = "".join(reads), starts_of(reads)
    first, length = starts[:-1], [len(r) for r in reads]
    d = resident(ctx, reads)
    try:
        for table in (False, True):
            got = check(ctx, d, stream, first, length, adapters, "edges", table=table, err=(1, 10), min_overlap=1)
        assert list(zip(got.out_len, got.out_adapter, got.out_mismatch)) == expect
        check(ctx, d, stream, first, length, adapters, "edges", err=(0, 1), min_overlap=8)
    finally:
        d.free()


def raw_call(pkg, ctx_h, dna_h, adapters, n_ad, opt, lists, n_segs, on_device, outs, cap, out_on_device, rep=None):
    arr = (C.c_char_p * max(len(adapters), 1))(*adapters) if adapters is not None else None
    return pkg.lib().dnagpu_dna_adapters(ctx_h, dna_h, arr, n_ad, opt, *lists, n_segs, on_device, *outs, cap, out_on_device, rep)


@pytest.mark.gpu
def test_checks_in_their_order(ctx, pkg):
    """every argument check of the header, each tried with all the later ones failing too; the outputs stay as they were"""
    B = pkg.binding
    opt_c = lambda *a: C.byref(B._AdaptersOptionsC(*a))
    good, none3 = opt_c(1, 10, 3, 0, 0, 0), (None, None, None)
    no_set = upload_text(ctx, "ACGTACGTAC")
    table = resident(ctx, ["ACGTAC", "GTAC"])
    out = [np.full(4, 77, dtype=np.uint64) for _ in range(6)]
    outs = [a.ctypes.data for a in out]
    one = np.array([0, 0, 0, 0], dtype=np.uint64)
    p = one.ctypes.data
    big = 2 ** 32
    try:
        h, ns, tb = ctx.h, no_set.h, table.h
        bad_opt = opt_c(2, 1, 3, 0, 0, 0)
        cases = [
            # 1: a NULL ctx, src, opt or adapters -- with a bad count, a bad letter, one list and too many segments behind
            (am.BAD_ARG, (None, ns, [b"AX"], 0, bad_opt, (None, p, None), big)),
            (am.BAD_ARG, (h, None, [b"AX"], 0, bad_opt, (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"], 0, None, (None, p, None), big)),
            (am.BAD_ARG, (h, ns, None, 1, good, (None, p, None), big)),
            # 2: the count, a length, an option -- with a bad letter behind, whose code is another
            (am.BAD_ARG, (h, ns, [b"AX"], 0, good, (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"] * 33, 33, good, (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX", b""], 2, good, (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX", b"A" * 33], 2, good, (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"], 1, bad_opt, (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"], 1, opt_c(1, 0, 3, 0, 0, 0), (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"], 1, opt_c(1, 10, 0, 0, 0, 0), (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"], 1, opt_c(1, 10, 33, 0, 0, 0), (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"], 1, opt_c(1, 10, 3, 3, 0, 0), (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"], 1, opt_c(1, 10, 3, 4, 0, 0), (None, p, None), big)),
            (am.BAD_ARG, (h, ns, [b"AX"], 1, opt_c(1, 10, 3, 0, 0, 1), (None, p, None), big)),
            # 3: a bad letter -- with one list and too many segments behind
            (am.QKMER_INVALID, (h, ns, [b"ACGT", b"AX"], 2, good, (None, p, None), big)),
            (am.QKMER_INVALID, (h, ns, [b"acgt"], 1, good, (None, None, p), big)),
            # 4: only one of the two lists -- with too many segments behind
            (am.BAD_ARG, (h, ns, [b"ACGU"], 1, good, (None, p, None), big)),
            (am.BAD_ARG, (h, tb, [b"ACGN"], 1, good, (p, None, p), big)),
            # 5: both NULL without a set, or more segments than sequences -- with too many segments behind
            (am.BAD_ARG, (h, ns, [b"ACGT"], 1, good, none3, big)),
            (am.BAD_ARG, (h, tb, [b"ACGT"], 1, good, none3, big)),
            (am.BAD_ARG, (h, tb, [b"ACGT"], 1, good, none3, 3)),
            # 6: too many segments (the lists are never read)
            (am.TOO_LARGE, (h, ns, [b"ACGT"], 1, good, (None, p, p), big)),
        ]
        for want, (ch, dh, ads, n_ad, o, lists, n) in cases:
            rc = raw_call(pkg, ch, dh, ads, n_ad, o, lists, n, 0, outs, 4, 0)
            assert rc == want, (want, ads, n_ad, lists, n)
            assert all((a == 77).all() for a in out)
        # found on the device: a segment that leaves the stream, among good ones; host lists and device lists, host outputs and
        # device outputs, all untouched
        ar = Arena(ctx, 1 << 17)
        try:
            for f, ln in (([0, 4, 11, 2], [4, 4, 0, 3]), ([0, 4, 3, 2], [4, 4, 8, 3]), ([2 ** 63, 0, 0, 0], [2 ** 63, 1, 1, 1])):
                fa, la = np.array(f, dtype=np.uint64), np.array(ln, dtype=np.uint64)
                rep = B._AdaptersReportC()
                rc = raw_call(pkg, h, ns, [b"ACGT"], 1, good, (None, fa.ctypes.data, la.ctypes.data), 4, 0, outs, 4, 0, C.byref(rep))
                assert rc == am.BAD_ARG and "leaves the stream" in pkg.lib().dnagpu_last_error().decode()
                assert all((a == 77).all() for a in out) and rep.segments == 0 and rep.bases_in == 0
                ar.reset()
                dl = [ar.take("seg_first", 32, 0, fa), ar.take("seg_len", 32, 0, la)]
                do = [ar.take(name, 32, 0) for name in PER + PASS]
                rc = raw_call(pkg, h, ns, [b"ACGT"], 1, good, (None, dl[0], dl[1]), 4, 1, do, 4, 1)
                assert rc == am.BAD_ARG
                ar.check("a segment that leaves the stream")
            # the last base of the stream is inside: a segment that ends exactly there, and an empty one behind it
            r = ctx.dna_adapters(no_set, ["AC"], [6, 10], [4, 0], min_overlap=2)
            assert [int(x) for x in r.out_len] == [2, 0] and r.failed_short == 1 and r.passed == 1
        finally:
            ar.free()
    finally:
        no_set.free()
        table.free()


@pytest.mark.gpu
def test_options_outputs_and_memory(ctx, dbg, pkg):
    """pass_cap below the passing count; NULL outputs; host and device lists and outputs in every combination; n_segs == 0;
    segments of 0 bases; a hit at p = 0, which keeps nothing and fails; min_bases; the two discard flags; seg_seq carried through;
    32 adapters with per_adapter checked"""
    rng = np.random.default_rng(SEED + 3)
    many = []
    while len(many) < 32:                                          # 32 adapters, all different in their first six letters
        a = "G" + rand_text(rng, 5 + len(many) % 27, "ATCG")
        if all(a[:6] != b[:6] for b in many):
            many.append(a)
    reads = []
    for i in range(200):
        body = rand_text(rng, int(rng.integers(0, 120)), "ATC")
        kind = i % 5
        if kind == 0:
            reads.append(body)
        elif kind == 1:
            reads.append(many[i % 32] + body)                      # p = 0: nothing is kept
        elif kind == 2:
            reads.append("")
        else:
            reads.append(body + many[(7 * i) % 32] + rand_text(rng, i % 9, "ATC"))
    stream, starts = "".join(reads), starts_of(reads)
    first, length = starts[:-1], [len(r) for r in reads]
    ids = [int(x) for x in rng.integers(0, 10 ** 12, size=len(reads))]
    d = resident(ctx, reads)
    ar = Arena(ctx, 1 << 17)
    try:
        base = dict(err=(1, 10), min_overlap=6)
        w = check(ctx, d, stream, first, length, many, "32 adapters", **base)
        assert all(c > 0 for c in w.report["per_adapter"]) and sum(w.report["per_adapter"]) == w.report["trimmed"]
        assert w.report["failed_short"] >= 80 and w.out_len[1] == 0 and w.out_adapter[1] == 1
        check(ctx, d, stream, first, length, many, "ids", seg_seq=ids, **base)
        passed = w.report["passed"]
        for cap in (0, 1, passed // 2, passed, passed + 1):
            check(ctx, d, stream, first, length, many, f"cap {cap}", cap=cap, seg_seq=ids, **base)
        r = check(ctx, d, stream, first, length, many, "min_bases", min_bases=40, **base)
        assert 0 < r.report["passed"] < passed
        for flags in (pkg.ADAPTERS_DISCARD_UNTRIMMED, pkg.ADAPTERS_DISCARD_TRIMMED):
            r = check(ctx, d, stream, first, length, many, "discard", flags=flags, min_bases=10, **base)
            assert r.report["failed_discarded"] and r.report["failed_short"] and 0 < r.report["passed"] < passed
        # the report only
        only = ctx.dna_adapters(d, many, first, length, want=False, **base)
        assert report_of(only) == w.report and only.out_len is None
        # no segment at all
        r = ctx.dna_adapters(d, many, [], [], **base)
        assert report_of(r) == am.empty_report() and len(r.out_len) == 0 and len(r.pass_seq) == 0
        none = ctx.dna_take(d, [])
        r = ctx.dna_adapters(none, many, **base)
        assert report_of(r) == am.empty_report()
        none.free()
        # device lists and device outputs, in the four combinations; seg_seq given and not
        n, cap = len(reads), 50
        fa, la, sa = (np.array(x, dtype=np.uint64) for x in (first, length, ids))
        for in_dev in (0, 1):
            for out_dev in (0, 1):
                for with_ids in (False, True):
                    want = am.trim(stream, first, length, many, seg_seq=ids if with_ids else None, cap=cap, **base)
                    ar.reset()
                    if in_dev:
                        lists = [ar.take("seg_seq", 8 * n, 0, sa) if with_ids else None, ar.take("seg_first", 8 * n, 8, fa),
                                 ar.take("seg_len", 8 * n, 16, la)]
                    else:
                        lists = [sa.ctypes.data if with_ids else None, fa.ctypes.data, la.ctypes.data]
                    wants = [want.out_len, want.out_adapter, want.out_mismatch, want.pass_seq, want.pass_first, want.pass_len]
                    if out_dev:
                        outs = [ar.take(f, 8 * n, 0) for f in PER] + [ar.take(f, 8 * cap, 8) for f in PASS]
                        host = None
                    else:
                        host = [np.full(n, 77, dtype=np.uint64) for _ in PER] + [np.full(cap + 2, 77, dtype=np.uint64) for _ in PASS]
                        outs = [a.ctypes.data for a in host]
                    got = ctx.dna_adapters_device(d, many, n, lists, in_dev, outs[:3], outs[3:], cap, out_dev, **base)
                    assert report_of(got) == want.report
                    what = f"lists on device {in_dev}, outputs on device {out_dev}, ids {with_ids}"
                    if out_dev:
                        ar.check(what, {p: np.array(x, dtype=np.uint64) for p, x in zip(outs, wants)})
                    else:
                        ar.check(what)
                        for a, x in zip(host, wants):
                            assert [int(v) for v in a[:len(x)]] == x and (a[len(x):] == 77).all(), what
    finally:
        ar.free()
        d.free()


# ------------------------------------------------------------------ the random differential

_RANDOM = {}


def random_table():
    """about 600 reads of 0 .. 300 bases; three adapters of 20, 32 and 13 letters, one with two IUPAC letters; an adapter
    planted into one third of the reads, whole or clipped by the read's end, with 0 .. 3 substituted letters.  Made once."""
    if "reads" not in _RANDOM:
        rng = np.random.default_rng(SEED + 4)
        a32 = list(rand_text(rng, 32))
        a32[5], a32[17] = "R", "N"
        adapters = [rand_text(rng, 20), "".join(a32), rand_text(rng, 13)]
        reads = []
        for i in range(600):
            n = int(rng.integers(0, 301))
            r = rand_text(rng, n)
            if i % 3 == 0 and n > 0:
                ad = list(adapters[int(rng.integers(0, 3))].replace("R", "G").replace("N", "T"))
                for _ in range(int(rng.integers(0, 4))):
                    j = int(rng.integers(0, len(ad)))
                    ad[j] = "ATCG"[("ATCG".index(ad[j]) + int(rng.integers(1, 4))) % 4]
                at = int(rng.integers(0, n))                        # clipped by the end where at + len(ad) > n
                r = (r[:at] + "".join(ad) + r[at + len(ad):])[:n]
            reads.append(r)
        _RANDOM.update(reads=reads, adapters=adapters, stream="".join(reads), starts=starts_of(reads), model={})
    return _RANDOM


@pytest.fixture(scope="module")
def random_dna(ctx):
    d = resident(ctx, random_table()["reads"])
    yield d
    d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("min_overlap", [1, 3, 8])
@pytest.mark.parametrize("err", [(0, 1), (1, 10), (1, 5), (1, 3)], ids=["0", "1/10", "1/5", "1/3"])
def test_random_differential(ctx, pkg, random_dna, err, min_overlap):
    t = random_table()
    reads, stream, starts = t["reads"], t["stream"], t["starts"]
    first, length = starts[:-1], [len(r) for r in reads]
    want = am.trim(stream, first, length, t["adapters"], err=err, min_overlap=min_overlap, min_bases=20)
    hit = want.report["trimmed"]
    # the condition of the test, from the model alone: both kinds of read are at least 5 % of the table
    assert hit >= 0.05 * len(reads) and len(reads) - hit >= 0.05 * len(reads), (err, min_overlap, hit)
    for table in (False, True):
        got = ctx.dna_adapters(random_dna, t["adapters"], None if table else first, None if table else length, err=err,
                               min_overlap=min_overlap, min_bases=20)
        assert_equal(want, got, f"random {err} {min_overlap} table {table}")


@pytest.mark.gpu
def test_scale(ctx, pkg):
    """2^21 + 5 segments of 12 bases drawn from 64 distinct reads: the size at which the scans of the table features change
    shape.  The model runs once per distinct read; the expected arrays are spread over the segments with numpy."""
    rng = np.random.default_rng(SEED + 5)
    ad = ["GATCGGAAGAGCA", "GTCTCTTATA"]
    distinct = []
    for i in range(64):
        r = rand_text(rng, 12, "ATC")
        if i % 2:
            k = int(rng.integers(3, 11))
            a = ad[i % 4 == 1]
            r = r[:12 - k] + a[:k]
        if i % 16 == 3:
            r = ad[0][:12]                                         # p = 0
        distinct.append(r)
    stream = "".join(distinct)
    opt = dict(err=(1, 10), min_overlap=3, min_bases=4)
    one = am.trim(stream, [12 * i for i in range(64)], [12] * 64, ad, **opt)
    assert 10 < one.report["trimmed"] < 54 and one.report["failed_short"] > 0
    n = 2 ** 21 + 5
    pick = rng.integers(0, 64, size=n)
    first, length = (12 * pick).astype(np.uint64), np.full(n, 12, dtype=np.uint64)
    kept, adp, mis = (np.array(x, dtype=np.uint64)[pick] for x in (one.out_len, one.out_adapter, one.out_mismatch))
    passing = kept >= 4
    d = upload_text(ctx, stream)
    try:
        got = ctx.dna_adapters(d, ad, first, length, **opt)
        assert np.array_equal(got.out_len, kept) and np.array_equal(got.out_adapter, adp) and np.array_equal(got.out_mismatch, mis)
        assert got.passed == int(passing.sum()) and got.segments == n and got.failed_short == n - got.passed
        assert np.array_equal(got.pass_seq, np.flatnonzero(passing).astype(np.uint64))
        assert np.array_equal(got.pass_first, first[passing]) and np.array_equal(got.pass_len, kept[passing])
        assert got.bases_in == 12 * n and got.bases_kept == int(kept.sum()) and got.bases_cut == 12 * n - int(kept.sum())
        assert got.trimmed == int((adp != am.NO_ADAPTER).sum())
        assert got.per_adapter[:2] == [int((adp == 0).sum()), int((adp == 1).sum())] and sum(got.per_adapter[2:]) == 0
    finally:
        d.free()
