"""The C-ABI's device-memory face (include/dnagpu.h: out_on_device, text_on_device, wire_on_device, on_device,
dnagpu_dna_wrap, dnagpu_hist_sorted_view) against the CPU oracle, bit for bit.

Every device pointer a test hands to the library is a sub-range of an ARENA: one dnagpu_buffer_alloc block filled with a
sentinel byte, the sub-range at a chosen byte offset with at least 4 KiB of sentinel on either side.  After the call the
whole arena comes back: the sub-range must hold the oracle's bytes exactly, inputs must be unchanged, and every other
byte must still be the sentinel -- so a store a few elements past `count` / `cap`, or before the output, is seen (on the
host face it lands in the slack of a pooled staging buffer).  The context runs with DNAGPU_DEBUG_POISON_POOL |
DNAGPU_DEBUG_GUARD_POOL and is synchronised at the end of every test: the pool's own guard bands are checked as well.

The contract pinned for views and windows: results never depend on the bits behind the last base of a dnagpu_dna_wrap view
or of a window [first, first + count)."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
BAD_ARG, DNA_INVALID_CHAR = 5, 12
GAP = 4096                                        # sentinel bytes on either side of every sub-range
SENTINEL = 0xC3


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def _ctx(pkg):
    c = pkg.Context(0)
    c._base_debug |= pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL
    c.set_debug(0)
    yield c
    c.close()


@pytest.fixture
def ctx(_ctx):
    yield _ctx
    _ctx.set_debug(0)
    _ctx.synchronize()                            # raises if a kernel wrote past the end of a pooled work buffer


# ------------------------------------------------------------------ 1. the arena

class Range:
    def __init__(self, name, start, nbytes, data):
        self.name, self.start, self.nbytes, self.data = name, start, nbytes, data


class Arena:
    """one device block of `nbytes` sentinel bytes; take() hands out sub-ranges, check() proves what a call did to it"""

    def __init__(self, ctx, nbytes, sentinel=SENTINEL):
        self.ctx, self.size = ctx, int(nbytes)
        self.base = ctx.buffer_alloc(self.size)
        assert self.base % 256 == 0, "the arena's offsets are byte offsets from a 256-byte boundary"
        self.dirty = self.size
        self.reset(sentinel)

    def reset(self, sentinel=None):
        """a fresh sentinel under everything handed out so far; forgets the sub-ranges"""
        if sentinel is not None:
            if getattr(self, "sentinel", None) != sentinel:
                self.dirty = self.size
            self.sentinel = sentinel
        self.img = np.full(self.size, self.sentinel, dtype=np.uint8)
        if self.dirty:
            self.ctx.upload_bytes(self.base, self.img[:self.dirty])
        self.ranges, self.cursor, self.dirty = [], 0, 0

    def take(self, name, nbytes, offset=0, data=None):
        """-> device address of a sub-range of nbytes at byte offset `offset` from a 256-byte boundary.  data: the bytes an
        INPUT holds (uploaded here, checked unchanged by check()); None: an output, sentinel until the call"""
        start = ((self.cursor + GAP + 255) & ~255) + int(offset)
        end = start + int(nbytes)
        assert end + GAP <= self.size, f"arena of {self.size} bytes is too small for {name} ({nbytes} bytes)"
        r = Range(name, start, int(nbytes), None)
        if data is not None:
            r.data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else \
                np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert r.data.size == nbytes
            self.img[start:end] = r.data
            if nbytes:
                self.ctx.upload_bytes(self.base + start, r.data)
        self.ranges.append(r)
        self.cursor = end
        self.dirty = max(self.dirty, end + GAP)
        return self.base + start

    def read(self, addr, nbytes):
        return self.ctx.download_bytes(addr, nbytes)

    def check(self, what, outputs=None):
        """outputs: {device address: expected bytes (a prefix of the sub-range; the rest must still be sentinel)}.  Sub-ranges
        not named: inputs must be unchanged, outputs untouched.  Everything else must be sentinel."""
        outputs = {} if outputs is None else dict(outputs)
        hw = min(self.cursor + GAP, self.size)
        got = self.ctx.download_bytes(self.base, hw)
        outside = np.ones(hw, dtype=bool)
        for r in self.ranges:
            want = np.full(r.nbytes, self.sentinel, dtype=np.uint8)
            kind = "untouched output"
            if r.data is not None:
                want, kind = r.data, "input"
            exp = outputs.pop(self.base + r.start, None)
            if exp is not None:
                e = np.frombuffer(bytes(exp), dtype=np.uint8) if isinstance(exp, (bytes, bytearray)) else \
                    np.ascontiguousarray(exp).view(np.uint8).reshape(-1)
                assert e.size <= r.nbytes
                want = want.copy()
                want[:e.size] = e
                kind = f"output ({e.size} bytes expected, sentinel behind)"
            seg = got[r.start:r.start + r.nbytes]
            outside[r.start:r.start + r.nbytes] = False
            if not np.array_equal(seg, want):
                at = int(np.flatnonzero(seg != want)[0])
                raise AssertionError(
                    f"{what}: {r.name} [{kind}, {r.nbytes} bytes at arena offset {r.start} = 256-byte boundary + {r.start % 256}] "
                    f"differs first at byte {at} (element {at // 8} of 8 bytes): got {seg[at:at + 16].tobytes().hex()} "
                    f"want {want[at:at + 16].tobytes().hex()}")
        assert not outputs, "expected bytes for an address that was not handed out"
        bad = np.flatnonzero(outside & (got != self.sentinel))
        if bad.size:
            at = int(bad[0])
            near = min(self.ranges, key=lambda r: min(abs(at - r.start), abs(at - (r.start + r.nbytes)))) if self.ranges else None
            rel = f"byte {at - near.start} relative to {near.name} ({near.nbytes} bytes at boundary + {near.start % 256})" if near \
                else f"arena offset {at}"
            raise AssertionError(f"{what}: {bad.size} sentinel bytes changed outside every sub-range, first at {rel}: "
                                 f"got {got[at:at + 16].tobytes().hex()}")

    def free(self):
        self.ctx.buffer_free(self.base)


@pytest.fixture
def arena(ctx):
    made = []

    def make(nbytes, sentinel=SENTINEL):
        a = Arena(ctx, nbytes, sentinel)
        made.append(a)
        return a
    yield make
    for a in made:
        a.free()


def u64_bytes(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.uint8)


def clean_words(words, n_bases):
    """the first n_bases bases of a packed stream as a sequence of their own: tail bits zero"""
    w = np.array(words[:(n_bases + 31) // 32], dtype=np.uint64)
    if n_bases % 32:
        w[-1] &= np.uint64((1 << (2 * (n_bases % 32))) - 1)
    return w


def sorted_groups(h):
    k, c = h.download()
    if not h.is_sorted:
        o = np.argsort(k, kind="stable")
        k, c = k[o], c[o]
    return k, c


def assert_groups(h, ok, oc, what):
    gk, gc = sorted_groups(h)
    assert h.distinct == len(ok), f"{what}: {h.distinct} groups, oracle {len(ok)}"
    assert np.array_equal(gk, ok), f"{what}: keys differ"
    assert np.array_equal(gc, oc), f"{what}: counts differ"
    assert h.total == int(oc.sum(dtype=np.uint64)), f"{what}: total"


# ------------------------------------------------------------------ 2. every device-memory variant

GEN_COUNTS = (0, 1, 2, 3, 511, 512, 513, 4095, 4096, 4097, 70_001)


@pytest.mark.parametrize("k", [1, 21, 31, 32])
def test_generate_kmers_out_on_device(ctx, arena, k):
    """dnagpu_generate_kmers, out_on_device: out 16-byte aligned and not (the scalar-pair stores of extract_kernel), every
    first x count around 2 keys per store, 512 rows per round and EXTRACT_TILE = 4096 rows per workgroup"""
    n = 70_100
    words = orc.synth_words(0xD10 + k, n)
    d = ctx.upload(words, n)
    ar = arena(max(GEN_COUNTS) * 8 + 4 * GAP)
    for first in (0, 1, 31, 33):
        for count in GEN_COUNTS:
            want = orc.generate_kmers(words, n, k, first, count, faithful=False)
            assert len(want) == count
            for off in (0, 8):
                ar.reset()
                out = ar.take("out_keys", count * 8, off)
                ctx.generate_kmers_device(d, k, first, count, C.c_void_p(out))
                ar.check(f"dnagpu_generate_kmers out_on_device k={k} first={first} count={count} out at +{off}",
                         {out: u64_bytes(want)})
    d.free()


def _filters(pkg, words, n):
    """one filter of each kind with its k and the oracle's (keys, positions)"""
    k = 21
    pat = "NNNNNNNNNNWSNNNNNNNNN"
    ln, bits = orc.kmer_encode("G")
    keys4 = orc.generate_kmers(words, n, 4, faithful=False)
    q = int(keys4[777])
    return [
        ("contains", k, pkg.Filter.contains(pat), orc.generate_kmers_contains(words, n, k, pat)),
        ("starts_with", k, pkg.Filter.starts_with(ln, bits), orc.generate_kmers_starts_with(words, n, k, ln, bits)),
        ("equals", 4, pkg.Filter.equals(4, q), orc.generate_kmers_equals(words, n, 4, 4, q)),
    ]


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["contains", "starts_with", "equals"])
def test_generate_kmers_filtered_out_on_device(ctx, pkg, arena, kind):
    """dnagpu_generate_kmers_filtered, out_on_device: keys / positions at either 16-byte parity, alone and together, every
    cap against a FRESH sentinel: slots >= min(cap, total) untouched, *n_out = the oracle's total whatever cap is"""
    n = 70_000
    words = orc.synth_words(31337, n)
    d = ctx.upload(words, n)
    name, k, flt, (wk, wp) = _filters(pkg, words, n)[kind]
    total = len(wk)
    assert total > 100
    rows = n - k + 1
    ar = arena(2 * (max(total + 7, 1001) + 8) * 8 + 8 * GAP)
    places = [(0, 0), (8, 8), (8, 0), (0, 8), (0, None), (8, None), (None, 0), (None, 8)]
    for cap in (0, 1, 2, 1000, 1001, total - 1, total, total + 7):
        for koff, poff in places:
            ar.reset()
            room = (max(cap, total) + 8) * 8
            dk = ar.take("out_keys", room, koff) if koff is not None else None
            dp = ar.take("out_pos", room, poff) if poff is not None else None
            m = ctx.count_matches_device(d, k, flt, 0, rows, C.c_void_p(dk) if dk else None, C.c_void_p(dp) if dp else None, cap)
            what = f"dnagpu_generate_kmers_filtered out_on_device {name} k={k} cap={cap} total={total} keys at +{koff} pos at +{poff}"
            assert m == total, f"{what}: *n_out = {m}"
            w = min(cap, total)
            exp = {}
            if dk:
                exp[dk] = u64_bytes(wk[:w])
            if dp:
                exp[dp] = u64_bytes(wp[:w])
            ar.check(what, exp)
    # a window that starts and ends inside the sequence
    first, count = 33, rows - 33 - 1000
    sel = (wp >= first) & (wp < first + count)
    for koff, poff in ((8, 8), (0, 8)):
        ar.reset()
        dk, dp = ar.take("out_keys", (total + 8) * 8, koff), ar.take("out_pos", (total + 8) * 8, poff)
        m = ctx.count_matches_device(d, k, flt, first, count, C.c_void_p(dk), C.c_void_p(dp), total)
        assert m == int(sel.sum())
        ar.check(f"dnagpu_generate_kmers_filtered out_on_device {name} window [{first}, +{count}) keys at +{koff} pos at +{poff}",
                 {dk: u64_bytes(wk[sel]), dp: u64_bytes(wp[sel])})
    d.free()


PACK_SIZES = (1, 31, 32, 33, 63, 64, 65, 1000, 100_003)
PACK_OFFSETS = (0, 1, 3, 4, 8, 15, 16)


@pytest.mark.parametrize("behind", ["G", "#"])
def test_dna_pack_text_on_device(ctx, arena, behind):
    """dnagpu_dna_pack, text_on_device: text at every alignment (pack_kernel's byte-wise path for full words), every size
    around 32 bases per word.  The bytes around the text are 'G' (a read past n_bases leaves non-zero tail bits) or '#'
    (a read past n_bases is DNAGPU_ERR_DNA_INVALID_CHAR)"""
    text = orc.dna_decode(orc.synth_words(0xD20, max(PACK_SIZES)), max(PACK_SIZES)).encode()
    ar = arena(max(PACK_SIZES) + 4 * GAP, ord(behind))
    for n in PACK_SIZES:
        want, _ = orc.dna_encode(text[:n].decode())
        for off in PACK_OFFSETS:
            ar.reset()
            t = ar.take("text", n, off, text[:n])
            what = f"dnagpu_dna_pack text_on_device n={n} text at +{off} behind={behind!r}"
            d = ctx.pack_device(t, n)
            assert d.n_bases == n, what
            got = d.download()
            assert np.array_equal(got, want), f"{what}: words differ, last word {int(got[-1]):#x} want {int(want[-1]):#x}"
            d.free()
            ar.check(what)


def test_dna_pack_text_on_device_invalid_characters(ctx, pkg, arena):
    """the FIRST invalid character is reported (bad_pos, bad_char): in the first word, in the last partial word, several in
    different words and workgroups (256 words = 8192 characters per workgroup); lower case is invalid, as the oracle says"""
    n = 100_003
    good = orc.dna_decode(orc.synth_words(0xD21, n), n)
    ar = arena(n + 4 * GAP, ord("G"))
    cases = [([(5, "N")], n), ([(n - 2, "x")], n), ([(70_000, "a"), (9_000, "t"), (40_001, "N"), (8_191, "c")], n),
             ([(31, "g")], 64), ([(32, "U")], 33), ([(0, " ")], 1), ([(99_999, "\0"), (99_998, "@")], n)]
    for bad, m in cases:
        t = bytearray(good[:m].encode())
        for pos, ch in bad:
            t[pos] = ord(ch)
        first = min(pos for pos, _ in bad)
        with pytest.raises(orc.OracleError):
            orc.dna_encode(t[:first + 1].decode())
        if first:
            orc.dna_encode(t[:first].decode())    # (valid up to there: the oracle's first offender is at `first`)
        for off in (0, 1, 3, 16):
            ar.reset()
            dt = ar.take("text", m, off, bytes(t))
            what = f"dnagpu_dna_pack text_on_device invalid at {sorted(bad)} n={m} text at +{off}"
            with pytest.raises(pkg.DnaGpuError) as ei:
                ctx.pack_device(dt, m)
            assert ei.value.code == DNA_INVALID_CHAR, what
            assert ei.value.bad_pos == first and ei.value.bad_char == bytes([t[first]]), \
                f"{what}: reported {ei.value.bad_pos} {ei.value.bad_char!r}, first is {first} {bytes([t[first]])!r}"
            ar.check(what)


UNPACK_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 100_003)


@pytest.mark.parametrize("off", range(18))
def test_dna_unpack_out_on_device(ctx, arena, off):
    """dnagpu_dna_unpack, out_on_device: out at every byte alignment (unpack_kernel's byte-wise path for whole lanes), every
    first x count around 16 characters per lane; and the windows that end at the last base of a sequence whose length is
    not a multiple of 32"""
    n = 100_100
    words = orc.synth_words(0xD30, n)
    text = orc.dna_decode(words, n).encode()
    d = ctx.upload(words, n)
    ar = arena(max(UNPACK_COUNTS) + 4 * GAP)
    windows = [(first, count) for first in (0, 1, 31, 32, 33) for count in UNPACK_COUNTS]
    windows += [(n - count, count) for count in (1, 4, 5, 16, 17, 33, 4097)]
    for first, count in windows:
        ar.reset()
        out = ar.take("out_text", count, off)
        ctx.unpack_device(d, first, count, C.c_void_p(out))
        ar.check(f"dnagpu_dna_unpack out_on_device first={first} count={count} (n={n}) out at +{off}",
                 {out: text[first:first + count]})
    d.free()


WIRE_WORDS = (1, 2, 3, 4, 255, 256, 257)


def test_dna_wire_on_device(ctx, pkg, arena):
    """dnagpu_dna_to_wire / _from_wire, wire_on_device: images of 1 .. 257 words with and without a partial last word, at
    byte offset 0 and 8; a wire_cap larger than the image: nothing written behind it; offsets 1 and 4: BAD_ARG and nothing
    written; bits behind the last base of a device image are cleared by from_wire; the round trip on the device"""
    ar = arena(2 * (8 + 8 * max(WIRE_WORDS)) + 6 * GAP)
    for nw in WIRE_WORDS:
        for n in (32 * nw, 32 * nw - 5):
            words = orc.synth_words(0xD40 + nw, n)
            image = orc.dna_to_wire(words, n)
            size = pkg.lib().dnagpu_dna_wire_size(n)
            assert size == len(image) == 8 + 8 * nw
            d = ctx.upload(words, n)
            for off in (0, 8):
                for extra in (0, 64):
                    ar.reset()
                    w = ar.take("wire", size + extra, off)
                    ctx.to_wire_device(d, C.c_void_p(w), size + extra)
                    what = f"dnagpu_dna_to_wire wire_on_device n={n} ({nw} words) wire at +{off} wire_cap={size + extra}"
                    ar.check(what, {w: image})
                    # ... and back from where it lies: the round trip on the device
                    d2 = ctx.from_wire_device(C.c_void_p(w), size)
                    assert d2.n_bases == n and np.array_equal(d2.download(), words), what + " -> from_wire"
                    d2.free()
                    ar.check(what + " -> from_wire", {w: image})
                # a device image with bits set behind the last base
                dirty = words.copy()
                if n % 32:
                    dirty[-1] |= ~np.uint64((1 << (2 * (n % 32))) - 1)
                img = image[:8] + dirty.byteswap().tobytes()
                ow, on = orc.dna_from_wire(img)
                assert on == n and np.array_equal(ow, words)
                ar.reset()
                w = ar.take("wire", size, off, img)
                d2 = ctx.from_wire_device(C.c_void_p(w), size)
                what = f"dnagpu_dna_from_wire wire_on_device n={n} ({nw} words) wire at +{off}, dirty tail"
                got = d2.download()
                assert d2.n_bases == n and np.array_equal(got, ow), f"{what}: last word {int(got[-1]):#x} want {int(ow[-1]):#x}"
                d2.free()
                ar.check(what)
            for off in (1, 4):
                ar.reset()
                w = ar.take("wire", size + 8, off)
                what = f"wire_on_device at +{off} (not 8-byte aligned) n={n}"
                assert pkg.lib().dnagpu_dna_to_wire(ctx.h, d.h, C.c_void_p(w), size + 8, 1) == BAD_ARG, what
                out = C.c_void_p()
                assert pkg.lib().dnagpu_dna_from_wire(ctx.h, C.c_void_p(w), size, 1, C.byref(out)) == BAD_ARG, what
                ar.check(what)
            d.free()


TEXT_SIZES = (1, 255, 256, 257, 10_001)


@pytest.mark.parametrize("k", [1, 7, 31, 32])
def test_kmers_to_text_on_device(ctx, arena, k):
    """dnagpu_kmers_to_text, on_device: records of k characters + NUL (stride k + 1), text at any alignment"""
    rng = np.random.default_rng(0xD50 + k)
    keys = rng.integers(0, 1 << 63, max(TEXT_SIZES), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, max(TEXT_SIZES)).astype(np.uint64)
    keys[0], keys[1 % len(keys)] = 0, ONES
    if k < 32:
        keys &= np.uint64((1 << (2 * k)) - 1)
    want = b"".join(orc.kmer_decode(int(x), k).encode() + b"\0" for x in keys)
    ar = arena(max(TEXT_SIZES) * (8 + k + 1) + 6 * GAP)
    for n in TEXT_SIZES:
        for toff in (0, 1, 7, 16):
            for koff in (0, 8):
                ar.reset()
                dk = ar.take("keys", n * 8, koff, u64_bytes(keys[:n]))
                dt = ar.take("out_text", n * (k + 1), toff)
                ctx.kmers_to_text_device(C.c_void_p(dk), n, k, C.c_void_p(dt))
                ar.check(f"dnagpu_kmers_to_text on_device k={k} n={n} keys at +{koff} text at +{toff}", {dt: want[:n * (k + 1)]})


BATCH_SIZES = (1, 255, 256, 257, 100_003)


def _random_keys(seed, n):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64)
    keys[0] = 0
    keys[n // 2] = ONES
    keys[n - 1] = ONES
    return keys


def test_kmer_hash_on_device(ctx, arena):
    """dnagpu_kmer_hash, on_device: keys at either 16-byte parity, 32-bit results at every 4-byte alignment class"""
    keys = _random_keys(0xD60, max(BATCH_SIZES))
    keys[1] = ONES
    want = np.array([orc.kmer_hash(int(x)) & 0xFFFFFFFF for x in keys], dtype=np.uint32)
    ar = arena(max(BATCH_SIZES) * 12 + 6 * GAP)
    for n in BATCH_SIZES:
        for koff in (0, 8):
            for ooff in (0, 4, 8, 12):
                ar.reset()
                dk = ar.take("keys", n * 8, koff, u64_bytes(keys[:n]))
                do = ar.take("out", n * 4, ooff)
                ctx.kmer_hash_device(C.c_void_p(dk), n, C.c_void_p(do))
                ar.check(f"dnagpu_kmer_hash on_device n={n} keys at +{koff} out at +{ooff}", {do: want[:n].view(np.uint8)})


@pytest.mark.parametrize("kind", ["contains", "starts_with", "equals"])
def test_kmer_match_on_device(ctx, pkg, arena, kind):
    """dnagpu_kmer_match, on_device: one flag byte per key at any alignment; the oracle's operator on every key"""
    rng = np.random.default_rng(sum(kind.encode()))
    nmax = max(BATCH_SIZES)
    for k in sorted({int(x) for x in rng.integers(3, 33, 2)} | {32}):
        keys = _random_keys(0xD70 + k, nmax)
        if k < 32:
            keys &= np.uint64((1 << (2 * k)) - 1)
        if kind == "contains":
            pat = ["N"] * k
            pat[int(rng.integers(0, k))] = "W"
            pat[int(rng.integers(0, k))] = "B"
            pat = "".join(pat)
            flt = pkg.Filter.contains(pat)
            want = np.array([orc.contains(pat, k, int(x)) for x in keys], dtype=np.uint8)
        elif kind == "starts_with":
            ln, bits = orc.kmer_encode("CA"[:min(2, k)])
            flt = pkg.Filter.starts_with(ln, bits)
            want = np.array([orc.starts_with(k, int(x), ln, bits) for x in keys], dtype=np.uint8)
        else:
            q = keys[12345]
            keys[rng.integers(0, nmax, 500)] = q
            keys[0] = q
            flt = pkg.Filter.equals(k, int(q))
            want = np.array([bool(orc.lib().orc_kmer_eq(k, int(x), k, int(q))) for x in keys], dtype=np.uint8)
        assert 0 < int(want.sum()) < nmax
        ar = arena(nmax * 9 + 6 * GAP)
        for n in BATCH_SIZES:
            for foff in (0, 1, 3, 16):
                for koff in ((0, 8) if foff in (0, 3) else (0,)):
                    ar.reset()
                    dk = ar.take("keys", n * 8, koff, u64_bytes(keys[:n]))
                    df = ar.take("flags", n, foff)
                    ctx.kmer_match_device(C.c_void_p(dk), n, k, flt, C.c_void_p(df))
                    ar.check(f"dnagpu_kmer_match on_device {kind} k={k} n={n} keys at +{koff} flags at +{foff}", {df: want[:n]})


# ------------------------------------------------------------------ 3. dnagpu_dna_wrap: views into live data

SEQ_BASES = 3_000_000
VIEWS = [(0, 1_000_000 - 64), (0, 1_000_003), (1001, 32 * 31_000), (1001, 999_979)]     # (first word, n_bases)
SK_KS = (20, 21, 27, 31, 32)


@pytest.fixture
def live(ctx, arena):
    """a random sequence of SEQ_BASES bases inside an arena -> (arena, device address of word 0, host words)"""
    words = orc.synth_words(0xD80, SEQ_BASES)
    assert SEQ_BASES % 32 == 0 and not np.any(words == 0)
    ar = arena(words.size * 8 + 4 * GAP)
    base = ar.take("sequence", words.size * 8, 0, u64_bytes(words))
    return ar, base, words


def _windows(rows):
    """whole, and a window with first > 0 whose end is short of the last row (it ends inside live data)"""
    return [(0, rows), (12_345, rows - 12_345 - 54_321)]


@pytest.mark.parametrize("view", range(len(VIEWS)))
def test_wrap_views_generate_filter_unpack_wire(ctx, pkg, live, view):
    """a view into the middle of live data == the same bases uploaded on their own: dnagpu_generate_kmers, one filter of
    each kind, dnagpu_dna_unpack, dnagpu_dna_to_wire (the neighbour's bases in the view's last word do not leak into the
    image); the wrapped words are unchanged and dnagpu_dna_free leaves them alone"""
    ar, base, words = live
    w0, n = VIEWS[view]
    nw = (n + 31) // 32
    clean = clean_words(words[w0:], n)
    if n % 32:
        assert words[w0 + nw - 1] != clean[-1], "the view's last word carries the neighbour's bases"
    held = ctx.device_bytes()
    v = ctx.wrap(C.c_void_p(base + 8 * w0), nw, n)
    what = f"dnagpu_dna_wrap view at word {w0}, n_bases={n}, n_words={nw}"
    assert v.n_bases == n and v.device_words == base + 8 * w0
    for k in (1, 21, 32):
        for first, count in _windows(n - k + 1):
            got = ctx.generate_kmers(v, k, first, count)
            assert np.array_equal(got, orc.generate_kmers(clean, n, k, first, count, faithful=False)), \
                f"{what}: dnagpu_generate_kmers k={k} rows [{first}, +{count})"
    for name, k, flt, (wk, wp) in _filters(pkg, clean, n):
        for first, count in _windows(n - k + 1):
            sel = (wp >= first) & (wp < first + count)
            gk, gp, tot = ctx.generate_kmers_filtered(v, k, flt, first=first, count=count)
            assert tot == int(sel.sum()) and np.array_equal(gk, wk[sel]) and np.array_equal(gp, wp[sel]), \
                f"{what}: dnagpu_generate_kmers_filtered {name} k={k} rows [{first}, +{count})"
    text = orc.dna_decode(clean, n)
    assert ctx.unpack(v) == text, f"{what}: dnagpu_dna_unpack"
    assert ctx.unpack(v, n - 17, 17) == text[-17:], f"{what}: dnagpu_dna_unpack of the last 17 bases"
    assert ctx.to_wire(v) == orc.dna_to_wire(clean, n), f"{what}: dnagpu_dna_to_wire (the image of the clean sequence)"
    v.free()
    assert ctx.device_bytes() >= held, f"{what}: dnagpu_dna_free released memory that is the caller's"
    ar.check(what)


@pytest.mark.parametrize("view", range(len(VIEWS)))
def test_wrap_views_counts(ctx, pkg, live, view):
    """dnagpu_count_kmers (k = 5 dense, 12, 31 tree) and the forced super-k-mer engine (k = 20 .. 32) on a view, whole and
    over a window that ends inside live data; dnagpu_dna_set_sequences + dnagpu_count_kmers_table on the view"""
    ar, base, words = live
    w0, n = VIEWS[view]
    nw = (n + 31) // 32
    clean = clean_words(words[w0:], n)
    v = ctx.wrap(C.c_void_p(base + 8 * w0), nw, n)
    what = f"dnagpu_dna_wrap view at word {w0}, n_bases={n}"
    for k in (5, 12, 31):
        for first, count in _windows(n - k + 1):
            ok, oc = orc.count_keys(orc.generate_kmers(clean, n, k, first, count, faithful=False))
            h = ctx.count_kmers(v, k, first, count)
            assert_groups(h, ok, oc, f"{what}: dnagpu_count_kmers k={k} rows [{first}, +{count})")
            h.free()
    for k in SK_KS:
        for first, count in _windows(n - k + 1):
            ok, oc = orc.count_keys(orc.generate_kmers(clean, n, k, first, count, faithful=False))
            ctx.set_debug(pkg.DEBUG_FORCE_SUPERKMER)
            try:
                h = ctx.count_kmers_unordered(v, k, first, count)
            finally:
                ctx.set_debug(0)
            assert not h.is_sorted
            assert_groups(h, ok, oc, f"{what}: dnagpu_count_kmers_unordered (super-k-mers) k={k} rows [{first}, +{count})")
            h.free()
    # the view as a table of sequences
    rng = np.random.default_rng(view)
    cuts = np.unique(np.concatenate([[0, n], rng.integers(0, n, 5000)])).astype(np.uint64)
    v.set_sequences(cuts)
    assert v.n_sequences == len(cuts) - 1
    for k in (12, 31):
        ok, oc = orc.count_keys(orc.generate_kmers_table(clean, cuts, k))
        for force in (0, pkg.DEBUG_FORCE_SUPERKMER):
            ctx.set_debug(force)
            try:
                h = ctx.count_kmers_table(v, k)
            finally:
                ctx.set_debug(0)
            assert_groups(h, ok, oc, f"{what}: dnagpu_count_kmers_table k={k} forced={force}")
            h.free()
    v.free()
    ar.check(what)


@pytest.mark.parametrize("k", SK_KS)
def test_superkmer_window_ends_inside_live_data_uploaded(ctx, pkg, k):
    """the same windows on an UPLOADED sequence: first > 0 and first + count short of the end, so the bits behind the
    window's last base are other rows' bases (independent of dnagpu_dna_wrap)"""
    n = 1_500_007
    words = orc.synth_words(0xD90 + k, n)
    d = ctx.upload(words, n)
    rows = n - k + 1
    for first, count in [(12_345, rows - 12_345 - 54_321), (31, 1_000_000), (0, rows - 1), (64, 999_936 - k + 1)]:
        ok, oc = orc.count_keys(orc.generate_kmers(words, n, k, first, count, faithful=False))
        ctx.set_debug(pkg.DEBUG_FORCE_SUPERKMER)
        try:
            h = ctx.count_kmers_unordered(d, k, first, count)
        finally:
            ctx.set_debug(0)
        assert_groups(h, ok, oc, f"dnagpu_count_kmers_unordered (super-k-mers) k={k} rows [{first}, +{count}) of {rows}")
        h.free()
    d.free()


def test_wrap_argument_rules(ctx, pkg, live):
    ar, base, words = live
    L, out = pkg.lib(), C.c_void_p()
    assert L.dnagpu_dna_wrap(ctx.h, C.c_void_p(base), 3, 97, C.byref(out)) == BAD_ARG          # n_words too small
    assert L.dnagpu_dna_wrap(ctx.h, C.c_void_p(base), 0, 1, C.byref(out)) == BAD_ARG
    assert L.dnagpu_dna_wrap(ctx.h, None, 4, 97, C.byref(out)) == BAD_ARG                       # NULL words with bases
    assert L.dnagpu_dna_wrap(ctx.h, C.c_void_p(base), 4, 97, None) == BAD_ARG
    assert L.dnagpu_dna_wrap(None, C.c_void_p(base), 4, 97, C.byref(out)) == BAD_ARG
    # more words than the bases need: what lies behind the bases is not part of the sequence
    v = ctx.wrap(C.c_void_p(base + 8), 10, 97)
    clean = clean_words(words[1:], 97)
    assert np.array_equal(ctx.generate_kmers(v, 32), orc.generate_kmers(clean, 97, 32, faithful=False))
    assert ctx.to_wire(v) == orc.dna_to_wire(clean, 97)
    h = ctx.count_kmers(v, 5)
    assert_groups(h, *orc.count_kmers(clean, 97, 5), "dnagpu_count_kmers on a view of 97 bases in 10 words")
    h.free()
    v.free()
    held = ctx.device_bytes()
    v = ctx.wrap(C.c_void_p(base), words.size, SEQ_BASES)
    v.free()
    assert ctx.device_bytes() == held
    assert np.array_equal(ctx.download_u64(base, words.size), words)      # still readable, still the caller's
    ar.check("dnagpu_dna_wrap argument rules")


# ------------------------------------------------------------------ 4. reading histograms

def tiling(distinct):
    """windows of odd sizes that tile [0, distinct) exactly, + the empty window at the end"""
    big = distinct // 2 + 1                        # (larger than any segment of a histogram of more than one segment)
    step = max(99_991, (distinct // 8) | 1)
    sizes = [1, 2, 255, 256, 257, 3, 1001, big]
    out, first, i = [], 0, 0
    while first < distinct:
        w = min(sizes[i] if i < len(sizes) else step, distinct - first)
        out.append((first, w))
        first += w
        i += 1
    return out + [(distinct, 0)]


def check_hist_reads(ctx, pkg, arena, h, ok, oc, what):
    """h against the oracle's groups (ok ascending, oc), then every way of reading it"""
    D = h.distinct
    assert D == len(ok) and h.total == int(oc.sum(dtype=np.uint64)), f"{what}: {D} groups / {h.total} rows"
    fk, fc = h.download()
    if h.is_sorted:
        assert np.array_equal(fk, ok) and np.array_equal(fc, oc), f"{what}: the full read is not the oracle's ascending groups"
    else:
        o = np.argsort(fk, kind="stable")
        assert np.array_equal(fk[o], ok) and np.array_equal(fc[o], oc), f"{what}: the full read is not the oracle's groups"
    assert h.summary() == orc.hist_summary(ok, oc), f"{what}: summary"
    wins = tiling(D)
    assert sum(w for _, w in wins) == D
    # (room for the whole histogram twice: a view that runs past its window must still land inside the arena)
    ar = arena(2 * (D + 2) * 8 + 6 * GAP)
    modes = [(0, True, True), (8, True, True), (0, True, False), (8, True, False), (0, False, True), (8, False, True),
             (8, True, True, 0), (0, True, True, 8)]
    L = pkg.lib()
    # dnagpu_hist_sorted_view into the arena: every placement for small windows, the placements in turn for large ones
    for wi, (first, count) in enumerate(wins):
        w = f"{what}: groups [{first}, +{count}) of {D}"
        k2, c2 = fk[first:first + count], fc[first:first + count]
        use = modes if count <= 4096 else [modes[(wi + j) % len(modes)] for j in range(3)]
        for m in use:
            koff, wk_, wc_ = m[0], m[1], m[2]
            coff = m[3] if len(m) > 3 else koff
            ar.reset()
            dk = ar.take("dev_keys", count * 8, koff) if wk_ else None
            dc = ar.take("dev_counts", count * 8, coff) if wc_ else None
            h.sorted_view_device(C.c_void_p(dk) if dk else None, C.c_void_p(dc) if dc else None, first, count)
            exp = {}
            if dk:
                exp[dk] = u64_bytes(k2)
            if dc:
                exp[dc] = u64_bytes(c2)
            ar.check(f"dnagpu_hist_sorted_view {w} keys at +{koff if wk_ else None} counts at +{coff if wc_ else None}", exp)
    # dnagpu_hist_download of the same windows (so the views above equal the downloads of their windows)
    for first, count in wins:
        w = f"{what}: groups [{first}, +{count}) of {D}"
        k2, c2 = h.download(first, count)
        assert np.array_equal(k2, fk[first:first + count]) and np.array_equal(c2, fc[first:first + count]), \
            f"{w}: dnagpu_hist_download is not the slice of the full download"
        k1, _ = h.download(first, count, want_counts=False)
        _, c1 = h.download(first, count, want_keys=False)
        assert np.array_equal(k1, k2) and np.array_equal(c1, c2), f"{w}: dnagpu_hist_download keys only / counts only"
    # out of range: BAD_ARG and nothing written
    for first, count in ((D, 1), (0, D + 1), (D + 1, 0), (D // 2 + 1, D - D // 2)):
        ar.reset()
        dk, dc = ar.take("dev_keys", 64, 0), ar.take("dev_counts", 64, 8)
        assert L.dnagpu_hist_sorted_view(ctx.h, h.h, first, count, C.c_void_p(dk), C.c_void_p(dc)) == BAD_ARG, f"{what}: [{first}, +{count})"
        assert L.dnagpu_hist_download(ctx.h, h.h, first, count, None, None) == BAD_ARG
        ar.check(f"dnagpu_hist_sorted_view {what}: [{first}, +{count}) out of range")
    # the device arrays part by part (count-0 padding slots skipped) hold the same groups
    pk, pc = [], []
    for i in range(h.n_parts):
        kp, cp, ext = h.part_arrays(i)
        if ext == 0:
            continue
        keys = ctx.download_u64(kp, ext)
        cnt = ctx.download_bytes(cp, ext * 4).view(np.uint32)
        pk.append(keys[cnt != 0])
        pc.append(cnt[cnt != 0].astype(np.uint64))
    pk = np.concatenate(pk) if pk else np.zeros(0, np.uint64)
    pc = np.concatenate(pc) if pc else np.zeros(0, np.uint64)
    o = np.argsort(pk, kind="stable")
    assert np.array_equal(pk[o], ok) and np.array_equal(pc[o], oc), f"{what}: the parts' device arrays hold other groups"
    if h.n_parts == 1:
        assert h.device_keys is not None or D == 0
    else:
        assert h.device_keys is None and h.device_counts is None


def test_hist_reads_ordered_tree(ctx, pkg, arena):
    n, k = 2_000_000, 31
    words = orc.synth_words(0xDA0, n)
    d = ctx.upload(words, n)
    h = ctx.count_kmers(d, k)
    assert h.is_sorted and h.distinct > 1_900_000
    check_hist_reads(ctx, pkg, arena, h, *orc.count_kmers(words, n, k), "ordered tree k=31")
    h.free()
    d.free()


def test_hist_reads_dense_short_k(ctx, pkg, arena):
    n, k = 200_000, 5
    words = orc.synth_words(0xDA1, n)
    d = ctx.upload(words, n)
    h = ctx.count_kmers(d, k)
    assert h.is_sorted and h.distinct == 1024
    check_hist_reads(ctx, pkg, arena, h, *orc.count_kmers(words, n, k), "dense k=5")
    h.free()
    d.free()


def test_hist_reads_ordered_heavy_hitters(ctx, pkg, arena):
    n, k = 1_000_000, 31
    words = orc.synth_words(0xDA2, n).copy()
    words[:len(words) // 2] = 0                    # half poly-A: one group of half the rows
    d = ctx.upload(words, n)
    h = ctx.count_kmers(d, k)
    ok, oc = orc.count_kmers(words, n, k)
    assert h.is_sorted and int(oc.max()) > n // 2 - 100
    check_hist_reads(ctx, pkg, arena, h, ok, oc, "ordered, half poly-A k=31")
    h.free()
    d.free()


def test_hist_reads_unordered_with_padding(ctx, pkg, arena):
    n, k = 400_000, 31
    words = orc.synth_words_repeat(0xDA3, n, 1000)
    d = ctx.upload(words, n)
    ctx.set_debug(pkg.DEBUG_FORCE_SUPERKMER)
    h = ctx.count_kmers_unordered(d, k)
    ctx.set_debug(0)
    assert not h.is_sorted and h.extent > h.distinct, f"extent {h.extent} distinct {h.distinct}: no padding slots"
    check_hist_reads(ctx, pkg, arena, h, *orc.count_kmers(words, n, k), "unordered super-k-mer, motif 1000, k=31")
    h.free()
    d.free()


def test_hist_reads_merge_result(ctx, pkg, arena):
    k = 21
    parts, keys = [], []
    for seed, n in ((0xDA4, 150_000), (0xDA5 << 20, 90_001)):
        words = orc.synth_words_repeat(seed, n, 5000)
        d = ctx.upload(words, n)
        parts.append(ctx.count_kmers_unordered(d, k))
        keys.append(orc.generate_kmers(words, n, k, faithful=False))
        d.free()
    keys.append(keys[0][:1000])                    # (groups the two share)
    wx, nx = orc.synth_words_repeat(0xDA4, 150_000, 5000), 1000 + k - 1
    d = ctx.upload(clean_words(wx, nx), nx)
    hx = ctx.count_kmers(d, k)
    d.free()
    m1 = parts[0].merge(parts[1])
    h = m1.merge(hx)
    assert not h.is_sorted
    check_hist_reads(ctx, pkg, arena, h, *orc.count_keys(np.concatenate(keys)), "dnagpu_hist_merge result k=21")
    for x in parts + [hx, m1, h]:
        x.free()


def test_hist_reads_table_of_sequences(ctx, pkg, arena):
    k = 21
    rng = np.random.default_rng(0xDA6)
    lens = rng.integers(0, 300, 3000)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(starts[-1])
    words = orc.synth_words(0xDA6, n)
    d = ctx.upload(words, n)
    h = ctx.count_kmers_batch(d, starts, k)
    check_hist_reads(ctx, pkg, arena, h, *orc.count_keys(orc.generate_kmers_table(words, starts, k)), "table of sequences k=21")
    h.free()
    d.free()


def test_hist_reads_several_parts(pkg):
    """histograms of several parts (the one-process multi-rank count, ranks sharing the device): the windows run across the
    parts' boundaries"""
    seed, k, n = 0xDA7, 31, 64_000_000            # (>= 4 coarse buckets: an owner cuts its range into groups)
    with pkg.Multi([0, 0], pkg.MULTI_COPY) as m:
        for r in m.ranks:
            r._base_debug |= pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL
            r.set_debug(0)
        m.set_parts(3)
        d = m.synth(seed, n)
        hs = m.count_unordered(d, k)
        m.dna_free(d)
        assert any(h.n_parts > 1 for h in hs), [h.n_parts for h in hs]
        ok, oc = orc.count_kmers(orc.synth_words(seed, n), n, k)
        got = [sorted_groups(h) for h in hs]
        allk = np.concatenate([g[0] for g in got])
        o = np.argsort(allk, kind="stable")
        assert np.array_equal(allk[o], ok) and np.array_equal(np.concatenate([g[1] for g in got])[o], oc)
        made = []
        for r, h in enumerate(hs):
            if h.n_parts < 2:
                continue

            def make(nbytes, sentinel=SENTINEL, ctx=m.ranks[r]):
                a = Arena(ctx, nbytes, sentinel)
                made.append(a)
                return a
            check_hist_reads(m.ranks[r], pkg, make, h, *got[r], f"rank {r}: {h.n_parts} parts k=31")
        for a in made:
            a.free()
        for r, h in enumerate(hs):
            h.free()
            m.ranks[r].synchronize()


def test_acc_download_windows_small(ctx, pkg):
    """dnagpu_acc_download over an accumulator of a few thousand groups: several windows inside one partition"""
    k, n = 31, 5_000
    acc = ctx.accumulator(k)
    words = orc.synth_words(0xDB0, n)
    d = ctx.upload(words, n)
    h = ctx.count_kmers(d, k)
    acc.add(h)
    acc.add(h)
    h.free()
    d.free()
    ok, oc = orc.count_kmers(words, n, k)
    D = acc.distinct
    assert D == len(ok)
    fk, fc = acc.download()
    got_k, got_c = [], []
    for first, count in tiling(D):
        a, b = acc.download(first, count)
        assert np.array_equal(a, fk[first:first + count]) and np.array_equal(b, fc[first:first + count]), \
            f"dnagpu_acc_download groups [{first}, +{count}) of {D}: not the slice of the full download"
        got_k.append(a)
        got_c.append(b)
    gk, gc = np.concatenate(got_k), np.concatenate(got_c)
    o = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[o], ok) and np.array_equal(gc[o], oc * np.uint64(2))
    L = pkg.lib()
    assert L.dnagpu_acc_download(ctx.h, acc.h, D, 1, None, None) == BAD_ARG
    assert L.dnagpu_acc_download(ctx.h, acc.h, 0, D + 1, None, None) == BAD_ARG
    acc.free()
