"""`=`, `^@` and `@>` at every pattern position and IUPAC set, on every path that evaluates them:

  1  the bit-sliced sweep over one sequence     Context.generate_kmers_filtered / count_matches_device  (filter_kernels.hip)
  2  the same sweep over a table of sequences   Context.generate_kmers_table                            (+ stream_rows.hpp)
  3  deny planes per key                        Context.kmer_match                                      (filter_match)
  4  the index scan: ranges, then deny planes   KmerIndex.scan                                          (index_math.hpp)
  5  the scalar operators of the glue, on host  glue.starts_with / glue.contains / kmer ==              (glue_types.c)

The reference is tests/operator_model.py (numpy, one base at a time), pinned against the CPU oracle by the tests of this file
that are not marked gpu.  Every comparison is exact equality of integer arrays.

Coverage of the fused single-sequence path by the sweep (a) below: all 448 (constraining IUPAC set, pattern position) pairs --
14 letters x 32 positions -- and 'U' at every position, each at every one of a thread's 32 row slots (stream_r asserts that
the input puts every code under every position at every slot); k = 1, 8, 9, 16, 17, 24, 25, 32 are the first and last shift of
every match_word<W>."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import operator_model as M
import oracle as orc
from __graft_entry__ import load_package
from test_kmer_index import expected_visited, index_order, mask_of, prune_depth
from test_table_kmers import Table, assert_rows

TILE = 8192                                       # rows of a workgroup tile (FB_TILE)
ROWS_R = 3 * TILE + 17                            # rows of R at k = 32: just over three tiles
N_R = ROWS_R + 31
SEED_R = 0x0FE2A
SENTINEL = np.uint64(0xC3C3C3C3C3C3C3C3)
LEN_MISMATCH_TEXT = "Qkmer pattern and kmer lengths do not match"        # dna.c:1107
PREFIX_TOO_LONG_TEXT = "Prefix length cannot exceed kmer length"         # dna.c:855
EDGE_ROWS = [0, 31, 32, 63, 64, 2047, 2048, 8191, 8192]                  # thread, wave and tile edges

KS_SWEEP = [1, 8, 9, 16, 17, 24, 25, 32]          # (a): every match_word<W> at its first and last shift
KS_TABLE = [1, 9, 32]
KS_LENGTHS = [1, 16, 17, 31, 32]                  # (c)
CONSTRAINING = [c for c in M.LETTERS if c not in "NU"]
SWEEP_LETTERS = CONSTRAINING + ["U"]              # every letter but N
SEAM_PAIRS = [(7, 8), (15, 16), (23, 24), (0, 31), (16, 31)]             # (b): across the word and dword seams


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def glue(pkg):
    return importlib.import_module(pkg.__name__ + ".glue")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ inputs, each built once

class Stream:
    """a packed stream with its codes and, per k, the model's key column"""

    def __init__(self, words, n):
        self.words, self.n = words, int(n)
        self.codes = M.codes_of(words, n)
        self._keys = {}

    @classmethod
    def of_codes(cls, codes):
        return cls(M.words_of(codes), len(codes))

    def keys(self, k):
        if k not in self._keys:
            self._keys[k] = M.keys_of(self.codes, k)
        return self._keys[k]


@functools.lru_cache(maxsize=None)
def stream_r():
    """R: every code under every pattern position at every one of a thread's 32 row slots, so that no sweep passes vacuously"""
    s = Stream(orc.synth_words(SEED_R, N_R), N_R)
    slot = np.arange(ROWS_R) % 32
    for i in range(32):
        under = s.codes[i:i + ROWS_R]
        for c in range(4):
            assert len(np.unique(slot[under == c])) == 32, (i, c)
    return s


@functools.lru_cache(maxsize=None)
def table_r(k):
    """R cut into sequences of 0, 1, k - 1, k, k + 1, 33 and 150 bases (21 times over) and two longer than a tile"""
    s = stream_r()
    base = [0, 1, k - 1, k, k + 1, 33, 150]
    lengths = base + [TILE + 77] + base * 20
    lengths.append(s.n - sum(lengths))
    assert lengths[-1] > TILE
    return Table(s.words, s.n, lengths)


@pytest.fixture(scope="module")
def r_dev(ctx):
    s = stream_r()
    d = ctx.upload(s.words, s.n)
    yield d
    d.free()


@pytest.fixture(scope="module")
def r_tables(ctx):
    """R resident as table_r(k), uploaded on first use"""
    held = {}

    def get(k):
        if k not in held:
            held[k] = table_r(k).upload(ctx)
        return held[k]
    yield get
    for d in held.values():
        d.free()


class Indexed:
    """an index over the key column of a stream, with the whole index order worked out once"""

    def __init__(self, ctx, s, k):
        self.col, self.k = s.keys(k), k
        self.idx = ctx.kmer_index(self.col, k)
        rows, self.order_keys = index_order(self.col, k)
        self.order_rows = rows
        self.order_at = rows.astype(np.int64)

    def free(self):
        self.idx.free()


@pytest.fixture(scope="module")
def r_indexes(ctx):
    held = {}

    def get(k):
        if k not in held:
            held[k] = Indexed(ctx, stream_r(), k)
        return held[k]
    yield get
    for x in held.values():
        x.free()


# ------------------------------------------------------------------ the cases

def single_patterns(k):
    """(a): N..X..N for every position and every letter but N"""
    for i in range(k):
        for x in SWEEP_LETTERS:
            yield i, x, "N" * i + x + "N" * (k - 1 - i)


def seam_patterns():
    """(b): a two-letter and a three-letter set, in both orders, at two positions on either side of a seam; k = 32"""
    for p, q in SEAM_PAIRS:
        for two in "WSMKRY":
            for three in "BDHV":
                for x, y in ((two, three), (three, two)):
                    pat = ["N"] * 32
                    pat[p], pat[q] = x, y
                    yield "".join(pat)


def headed_patterns(s, k):
    """(a) on the index: the single constraint behind a head of L singleton bases of a present key -> (L, i, pattern)"""
    key = int(s.keys(k)[ROWS_R // 3])
    for L in sorted({L for L in (0, 5, 8, k - 1) if L < k}):
        head = [1 << ((key >> (2 * j)) & 3) for j in range(L)]
        for i in range(L, k):
            for x in SWEEP_LETTERS:
                sets = head + [15] * (k - L)
                sets[i] = M.IUPAC[x]
                yield L, i, M.pattern_of(sets)


def length_cases(pkg, s, k):
    """(c): -> (name, filter, the model's sets).  `^@` at every length 0..k of a prefix of a present row, clean and with a stray
    bit behind the prefix; `=` of a present key, an absent key, key 0, the all-ones key, and of k - 1 and k + 1 bases"""
    col = s.keys(k)
    present = int(col[ROWS_R // 2])
    full = int(mask_of(k))
    for plen in range(k + 1):
        bits = present & int(mask_of(plen))
        yield f"^@ {plen} bases", pkg.Filter.starts_with(plen, bits), M.sets_of_prefix(k, plen, bits)
        for stray in {2 * plen, 2 * plen + 1, 63}:
            if plen < 32:
                dirty = bits | (1 << stray)
                assert M.sets_of_prefix(k, plen, dirty) is None
                yield f"^@ {plen} bases, stray bit {stray}", pkg.Filter.starts_with(plen, dirty), None
    have = set(col.tolist())
    rng = np.random.default_rng(k)
    absent = next((x for x in (int(v) & full for v in rng.integers(0, 1 << 63, 64, dtype=np.uint64) * 2 + 1) if x not in have), None)
    assert (absent is None) == (k == 1)              # (k = 1: all four keys occur)
    for name, q in (("present", present), ("absent", absent), ("key 0", 0), ("all ones", full)):
        if q is not None:
            sets = M.sets_of_equals(k, k, q)
            assert sets is not None and M.rows_matching(s.codes, k, sets).any() == (q in have)
            yield f"= {name}", pkg.Filter.equals(k, q), sets
    if k < 32:
        yield "= stray bit", pkg.Filter.equals(k, present | (1 << (2 * k))), M.sets_of_equals(k, k, present | (1 << (2 * k)))
    for qlen in (k - 1, k + 1):
        q = present & int(mask_of(min(qlen, 32)))
        assert M.sets_of_equals(k, qlen, q) is None
        yield f"= of {qlen} bases", pkg.Filter.equals(qlen, q), None


def random_patterns(n, seed):
    """(e): random k, 1 - 6 constrained positions, all sixteen letters"""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        k = int(rng.integers(1, 33))
        pat = ["N"] * k
        for _ in range(int(rng.integers(1, 7))):
            pat[int(rng.integers(0, k))] = M.LETTERS[int(rng.integers(0, 16))]
        yield k, "".join(pat)


def planted_patterns(s):
    """P: 64 rows of R at the thread, wave and tile edges and elsewhere; for each a 32-position pattern with no N, every position
    a random two- or three-letter set that holds the row's base -> (row, pattern)"""
    rng = np.random.default_rng(0x9A77)
    rows = sorted({t * TILE + e for t in range(3) for e in EDGE_ROWS if e < TILE} | {3 * TILE, ROWS_R - 1})
    rows += [int(x) for x in rng.choice(np.setdiff1d(np.arange(ROWS_R), rows), 64 - len(rows), replace=False)]
    assert len(set(rows)) == 64
    for row in rows:
        sets = []
        for i in range(32):
            code = int(s.codes[row + i])
            holding = [t for t in range(16) if bin(t).count("1") in (2, 3) and (t >> code) & 1]
            sets.append(holding[int(rng.integers(0, len(holding)))])
        yield row, M.pattern_of(sets)


# ------------------------------------------------------------------ one check per evaluator

def window_of(mask, first, count):
    sel = mask.copy()
    sel[:first] = False
    sel[first + count:] = False
    return np.flatnonzero(sel)


def check_fused(ctx, d, s, k, flt, sets, what, first=0, count=None):
    """evaluator 1: positions, keys and n_out of window [first, first + count); -> the expected positions"""
    mask = M.rows_matching(s.codes, k, sets)
    if count is None:
        count = len(mask) - first
    pos = window_of(mask, first, count)
    gk, gp, n = ctx.generate_kmers_filtered(d, k, flt, first=first, count=count)
    assert n == len(pos), f"{what}: n_out = {n}, the model has {len(pos)} rows"
    assert np.array_equal(gp, pos.astype(np.uint64)), f"{what}: positions"
    assert np.array_equal(gk, s.keys(k)[pos]), f"{what}: keys"
    return pos


def check_match(ctx, s, k, flt, sets, what):
    """evaluator 3: the flags over the key column"""
    got = ctx.kmer_match(s.keys(k), k, flt)
    assert np.array_equal(got, M.rows_matching(s.codes, k, sets)), f"{what}: flags"


def check_index(x, s, flt, sets, what):
    """evaluator 4: rows and keys in index order, n_out, and visited = the rows under the pruned prefix"""
    mask = M.rows_matching(s.codes, x.k, sets)
    keep = mask[x.order_at]
    rows, keys, n_out, visited = x.idx.scan(flt, cap=len(x.col))
    assert n_out == int(mask.sum()), f"{what}: n_out = {n_out}, the model has {int(mask.sum())} rows"
    assert np.array_equal(rows, x.order_rows[keep]), f"{what}: rows"
    assert np.array_equal(keys, x.order_keys[keep]), f"{what}: keys"
    want = expected_visited(x.col, sets) if sets is not None else 0
    assert visited == want, f"{what}: visited {visited}, the pruned ranges hold {want}"


def check_table(ctx, d, t, s, k, flt, sets, what):
    """evaluator 2: model rows AND table rows, with the sequence and ordinal of each"""
    got = ctx.generate_kmers_table(d, k, flt)
    assert_rows(got, t.expected(k, match=M.rows_matching(s.codes, k, sets)), what)
    return got


def glue_kmer(glue, length, bits):
    return glue.kmer(c=glue._Kmer(length, bits))


# ================================================================== CPU: the model, the oracle and the glue

def test_sweep_covers_every_set_at_every_position():
    """what the parametrisation of (a) feeds the fused path: 448 of 448 (set, position) pairs, 'U' at all 32 positions"""
    fed = {(x, i) for k in KS_SWEEP for i, x, _ in single_patterns(k)}
    assert sum(k for k in KS_SWEEP) == 132 and len(CONSTRAINING) == 14
    assert len({(x, i) for x, i in fed if x != "U"}) == 448 == 14 * 32
    assert {i for x, i in fed if x == "U"} == set(range(32))
    assert {(x, i) for i, x, _ in single_patterns(32)} == fed
    assert len(list(seam_patterns())) == 5 * 6 * 4 * 2
    stream_r()                                       # the code-under-every-slot assertion


def test_model_letters_are_the_oracles():
    """nucleotide_matches (dna.c:1064-1086) for all 16 x 4 pairs"""
    for letter in M.LETTERS:
        for code in range(4):
            assert orc.contains(letter, 1, code) == bool((M.IUPAC[letter] >> code) & 1), (letter, code)
    assert M.IUPAC["U"] == 0 and M.IUPAC["N"] == 15 and sorted(M.IUPAC.values()) == list(range(16))


def test_model_keys_and_table_rows():
    s = stream_r()
    for k in (1, 9, 31, 32):
        assert np.array_equal(s.keys(k), orc.generate_kmers(s.words, s.n, k, faithful=False))
    assert np.array_equal(M.words_of(s.codes), s.words)
    for k in KS_TABLE:
        t = table_r(k)
        assert np.array_equal(M.table_rows(t.starts, t.n, k), t.rows(k)[2])


@pytest.mark.parametrize("k", KS_TABLE)
def test_model_contains_is_the_oracles(k):
    """every position x every letter but N over R: rows_matching == orc.generate_kmers_contains"""
    s = stream_r()
    for i, x, pat in single_patterns(k):
        mask = M.rows_matching(s.codes, k, M.sets_of_pattern(pat))
        wk, wp = orc.generate_kmers_contains(s.words, s.n, k, pat)
        assert np.array_equal(np.flatnonzero(mask).astype(np.uint64), wp), pat
        assert np.array_equal(s.keys(k)[mask], wk), pat


@pytest.mark.parametrize("k", KS_TABLE)
def test_model_equals_and_prefix_are_the_oracles(pkg, k):
    s = stream_r()
    for name, flt, sets in length_cases(pkg, s, k):
        fn = orc.generate_kmers_equals if name[0] == "=" else orc.generate_kmers_starts_with
        wk, wp = fn(s.words, s.n, k, int(flt.c.length), int(flt.c.bits))
        mask = M.rows_matching(s.codes, k, sets)
        assert np.array_equal(np.flatnonzero(mask).astype(np.uint64), wp), name
        assert np.array_equal(s.keys(k)[mask], wk), name
        if name == "^@ 0 bases":
            assert mask.all()


def test_glue_contains_truth_table(glue):
    """evaluator 5, (a): letter x position x code on single values at k = 32"""
    rng = np.random.default_rng(32)
    for i in range(32):
        noise = int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))
        for x in M.LETTERS:
            pat = "N" * i + x + "N" * (31 - i)
            q = glue.qkmer(pat)
            for code in range(4):
                value = (noise & ~(3 << (2 * i))) | (code << (2 * i))
                want = bool((M.IUPAC[x] >> code) & 1)
                assert M.key_matches(value, 32, M.sets_of_pattern(pat)) == want
                assert glue.contains(q, glue_kmer(glue, 32, value)) == want, (pat, code)


@pytest.mark.parametrize("k", KS_LENGTHS)
def test_glue_equals_and_prefix_at_every_length(pkg, glue, k):
    """evaluator 5, (c): the scalar `=` and `^@` on rows of R"""
    s = stream_r()
    col = s.keys(k)
    sample = [int(v) for v in col[:150]] + [int(col[ROWS_R // 2]), 0, int(mask_of(k))]
    for name, flt, sets in length_cases(pkg, s, k):
        rhs = glue_kmer(glue, int(flt.c.length), int(flt.c.bits))
        hits = 0
        for key in sample:
            lhs = glue_kmer(glue, k, key)
            got = (lhs == rhs) if name[0] == "=" else glue.starts_with(lhs, rhs)
            assert got == M.key_matches(key, k, sets), (name, key)
            hits += got
        assert hits >= 1 or sets is None or name in ("= absent", "= key 0", "= all ones"), name
    with pytest.raises(glue.GlueError) as ei:
        glue.starts_with(glue_kmer(glue, k, sample[0]), glue_kmer(glue, k + 1, 0))
    assert str(ei.value) == PREFIX_TOO_LONG_TEXT
    for other in (k - 1, k + 1):
        if 1 <= other <= 32:
            with pytest.raises(glue.GlueError) as ei:
                glue.contains(glue.qkmer("N" * other), glue_kmer(glue, k, sample[0]))
            assert str(ei.value) == LEN_MISMATCH_TEXT


# ================================================================== GPU (a): every set at every position

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS_SWEEP)
def test_every_set_at_every_position_fused(ctx, pkg, r_dev, k):
    """evaluator 1: k positions x 15 letters ('U': zero rows, no ERROR), positions, keys and n_out"""
    s = stream_r()
    for i, x, pat in single_patterns(k):
        pos = check_fused(ctx, r_dev, s, k, pkg.Filter.contains(pat), M.sets_of_pattern(pat), f"k={k} {pat}")
        assert (len(pos) == 0) == (x == "U"), pat


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS_SWEEP)
def test_every_set_at_every_position_match(ctx, pkg, k):
    """evaluator 3: the flags over R's key column"""
    s = stream_r()
    for i, x, pat in single_patterns(k):
        check_match(ctx, s, k, pkg.Filter.contains(pat), M.sets_of_pattern(pat), f"k={k} {pat}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS_SWEEP)
def test_every_set_at_every_position_index(ctx, pkg, r_indexes, k):
    """evaluator 4: the constraint alone and behind heads of 5, 8 and k - 1 singleton bases of a present key, so that it falls
    inside the pruned prefix (index_prefix_at's mixed-radix enumeration) for some (i, L) and into the residual for others"""
    s = stream_r()
    x = r_indexes(k)
    pruned, residual = 0, 0
    for L, i, pat in headed_patterns(s, k):
        sets = M.sets_of_pattern(pat)
        check_index(x, s, pkg.Filter.contains(pat), sets, f"k={k} L={L} {pat}")
        if sets is not None and sets[i] != 15:
            inside = i < prune_depth(sets)
            pruned += inside
            residual += not inside
    assert pruned > 0 and (residual > 0 or k <= 5), (k, pruned, residual)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS_TABLE)
def test_every_set_at_every_position_table(ctx, pkg, r_tables, k):
    """evaluator 2: the same patterns over R cut into sequences of every length around k"""
    s, t, d = stream_r(), table_r(k), r_tables(k)
    for i, x, pat in single_patterns(k):
        got = check_table(ctx, d, t, s, k, pkg.Filter.contains(pat), M.sets_of_pattern(pat), f"table k={k} {pat}")
        assert (got[3] == 0) == (x == "U"), pat


# ================================================================== GPU (b): pairs across the seams

@pytest.mark.gpu
def test_seam_pairs_fused(ctx, pkg, r_dev):
    s = stream_r()
    for pat in seam_patterns():
        pos = check_fused(ctx, r_dev, s, 32, pkg.Filter.contains(pat), M.sets_of_pattern(pat), pat)
        assert len(pos) > 0, pat


@pytest.mark.gpu
def test_seam_pairs_match(ctx, pkg):
    s = stream_r()
    for pat in seam_patterns():
        check_match(ctx, s, 32, pkg.Filter.contains(pat), M.sets_of_pattern(pat), pat)


@pytest.mark.gpu
def test_seam_pairs_index(ctx, pkg, r_indexes):
    s = stream_r()
    for pat in seam_patterns():
        check_index(r_indexes(32), s, pkg.Filter.contains(pat), M.sets_of_pattern(pat), pat)


# ================================================================== GPU (c): `=` and `^@` at every length

@pytest.mark.gpu
@pytest.mark.parametrize("k", KS_LENGTHS)
def test_equals_and_prefix_at_every_length(ctx, pkg, r_dev, r_tables, r_indexes, k):
    """evaluators 1 - 4.  Length 0 matches every row; stray bits match nothing and raise nothing; a prefix longer than k and a
    pattern of another length are the reference's ERRORs everywhere (the table: with a table row in the window)"""
    s, t, d_table = stream_r(), table_r(k), r_tables(k)
    x = r_indexes(k)
    for name, flt, sets in length_cases(pkg, s, k):
        what = f"k={k} {name}"
        pos = check_fused(ctx, r_dev, s, k, flt, sets, what)
        if name == "^@ 0 bases":
            assert len(pos) == s.n - k + 1
        if sets is None:
            assert len(pos) == 0
        check_table(ctx, d_table, t, s, k, flt, sets, what)
        check_match(ctx, s, k, flt, sets, what)
        check_index(x, s, flt, sets, what)
    bad = [(pkg.Filter.starts_with(k + 1, 0), PREFIX_TOO_LONG_TEXT)]
    bad += [(pkg.Filter.contains("N" * other), LEN_MISMATCH_TEXT) for other in (k - 1, k + 1) if 1 <= other <= 32]
    for flt, text in bad:
        for call in (lambda: ctx.generate_kmers_filtered(r_dev, k, flt), lambda: ctx.generate_kmers_table(d_table, k, flt),
                     lambda: ctx.kmer_match(s.keys(k), k, flt), lambda: x.idx.scan(flt)):
            with pytest.raises(pkg.DnaGpuError) as ei:
                call()
            assert ei.value.message == text


# ================================================================== GPU (d): G1, AA and P

G1_COUNT = TILE + 100                             # rows of G1's window: its last row is in the second tile


def g1_base(k, seed):
    """a stream over {A, T, C} with room for a window of G1_COUNT rows from first = 31 on and rows behind it"""
    n = 31 + G1_COUNT + k - 1 + 40
    return np.random.default_rng(seed).integers(0, 3, n).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 17, 32])
def test_single_g_fused(ctx, pkg, k):
    """G1 on evaluator 1: a single G in the stream; G N.. matches exactly its row and N.. G exactly the row k - 1 before it,
    at the thread, wave and tile edges of windows that start 0, 1 and 31 bases into a word"""
    base = g1_base(k, 0x61 + k)
    for first in (0, 1, 31):
        for rel in EDGE_ROWS + [G1_COUNT - 1]:
            row = first + rel
            for lead in (True, False):
                codes = base.copy()
                codes[row if lead else row + k - 1] = 3
                pat = "G" + "N" * (k - 1) if lead else "N" * (k - 1) + "G"
                s = Stream.of_codes(codes)
                d = ctx.upload(s.words, s.n)
                what = f"k={k} first={first} row {rel} of the window, {pat[:2]}..{pat[-1]}"
                pos = check_fused(ctx, d, s, k, pkg.Filter.contains(pat), M.sets_of_pattern(pat), what, first, G1_COUNT)
                assert pos.tolist() == [row], what
                d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 32])
def test_single_g_table(ctx, pkg, k):
    """G1 on evaluator 2: the G as the last base of one sequence and as the first base of the next; the row that would span
    the boundary is absent"""
    bounds = [40, 96, 2053, TILE, TILE + 33]        # (every sequence has at least 33 bases)
    n = TILE + 33 + 200
    base = np.random.default_rng(0x62 + k).integers(0, 3, n).astype(np.uint8)
    lengths = list(np.diff([0] + bounds + [n]))
    for b in bounds:
        for at in (b - 1, b):
            for lead in (True, False):
                codes = base.copy()
                codes[at] = 3
                pat = "G" + "N" * (k - 1) if lead else "N" * (k - 1) + "G"
                s = Stream.of_codes(codes)
                t = Table(s.words, s.n, lengths)
                d = t.upload(ctx)
                what = f"k={k} boundary {b}, G at {at}, {pat[:2]}..{pat[-1]}"
                gk, gs, gp, n_out = check_table(ctx, d, t, s, k, pkg.Filter.contains(pat), M.sets_of_pattern(pat), what)
                d.free()
                stream_row = at if lead else at - k + 1
                spans = stream_row < b < stream_row + k
                assert spans == ((at == b - 1) == lead), what
                if spans:
                    assert n_out == 0, f"{what}: the row across the boundary came back"
                elif at == b:
                    assert (n_out, int(gs[0]), int(gp[0])) == (1, bounds.index(b) + 1, 0), what


AA_ROWS = [1, 31, 32, 33, 8191, 8192, 8193]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 30])
def test_poly_a_counts_and_caps_fused(ctx, pkg, k):
    """AA on evaluator 1: A x n under A x k.  The stream ends inside its last word and the zero fill behind it decodes as A, so
    a row past `count` would match too: n_out == count exactly, for windows that end 0, 1 and 31 rows before the end.  Device
    outputs at both 16-byte parities, caps around 0 and around count, a sentinel behind each array"""
    flt = pkg.Filter.contains("A" * k)
    room = max(AA_ROWS) + 4
    kb, pb = ctx.buffer_alloc(8 * (room + 1)), ctx.buffer_alloc(8 * (room + 1))
    assert kb % 16 == 0 and pb % 16 == 0
    clean = np.full(room + 1, SENTINEL)
    for rows in AA_ROWS:
        n = rows + k - 1
        assert n % 32 != 0
        words = np.zeros((n + 31) // 32, dtype=np.uint64)
        d = ctx.upload(words, n)
        for short in (0, 1, 31):
            count = rows - short
            if count < 1:
                continue
            gk, gp, n_out = ctx.generate_kmers_filtered(d, k, flt, first=0, count=count)
            assert n_out == count, f"k={k} {rows} rows, window of {count}: n_out = {n_out}"
            assert not gk.any() and np.array_equal(gp, np.arange(count, dtype=np.uint64))
            for par in (0, 1):
                for cap in sorted({0, 1, 2, count - 1, count, count + 1}):
                    what = f"k={k} {rows} rows, window of {count}, parity {par}, cap {cap}"
                    ctx.upload_u64(kb, clean)
                    ctx.upload_u64(pb, clean)
                    n_out = ctx.count_matches_device(d, k, flt, 0, count, C.c_void_p(kb + 8 * par), C.c_void_p(pb + 8 * par), cap)
                    assert n_out == count, f"{what}: n_out = {n_out}"
                    w = min(cap, count)
                    gk, gp = ctx.download_u64(kb, room + 1), ctx.download_u64(pb, room + 1)
                    want_k, want_p = clean.copy(), clean.copy()
                    want_k[par:par + w] = 0
                    want_p[par:par + w] = np.arange(w, dtype=np.uint64)
                    assert np.array_equal(gk, want_k), f"{what}: keys / the words around them"
                    assert np.array_equal(gp, want_p), f"{what}: positions / the words around them"
        d.free()
    ctx.buffer_free(kb)
    ctx.buffer_free(pb)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 30])
def test_poly_a_table(ctx, pkg, k):
    """AA on evaluator 2: sequences of exactly k bases have one row each, sequences of k - 1 bases none at all"""
    flt = pkg.Filter.contains("A" * k)
    for length in (k, k - 1):
        m = TILE // length + 40                      # the stream reaches into a second tile
        t = Table(np.zeros((m * length + 31) // 32, dtype=np.uint64), m * length, [length] * m)
        s = Stream(t.words, t.n)
        d = t.upload(ctx)
        gk, gs, gp, n_out = check_table(ctx, d, t, s, k, flt, M.sets_of_pattern("A" * k), f"k={k} sequences of {length}")
        d.free()
        if length == k:
            assert n_out == m and np.array_equal(gs, np.arange(m, dtype=np.uint64)) and not gp.any()
        else:
            assert n_out == 0


@pytest.mark.gpu
def test_planted_full_width_patterns(ctx, pkg, r_dev, r_tables):
    """P on evaluators 1 and 2: no N anywhere, so all four match_word instantiations are ANDed at once"""
    s, t, d = stream_r(), table_r(32), r_tables(32)
    for row, pat in planted_patterns(s):
        assert "N" not in pat
        sets = M.sets_of_pattern(pat)
        pos = check_fused(ctx, r_dev, s, 32, pkg.Filter.contains(pat), sets, f"planted at row {row}")
        assert row in pos
        check_table(ctx, d, t, s, 32, pkg.Filter.contains(pat), sets, f"planted at row {row}, table")


# ================================================================== GPU (e): all paths agree

@pytest.mark.gpu
def test_all_paths_agree_on_random_patterns(ctx, pkg, r_dev, r_indexes):
    """200 random patterns: evaluators 1, 3 and 4 return one row set, evaluator 2 over a one-sequence table evaluator 1's rows"""
    s = stream_r()
    one = Table(s.words, s.n, [s.n]).upload(ctx)
    some = 0
    for k, pat in random_patterns(200, 20261021):
        flt, sets = pkg.Filter.contains(pat), M.sets_of_pattern(pat)
        pos = check_fused(ctx, r_dev, s, k, flt, sets, f"k={k} {pat}")
        some += len(pos) > 0
        flags = ctx.kmer_match(s.keys(k), k, flt)
        assert np.array_equal(np.flatnonzero(flags), pos), f"k={k} {pat}: kmer_match"
        x = r_indexes(k)
        rows, keys, n_out, _ = x.idx.scan(flt, cap=len(x.col))
        assert n_out == len(pos) and np.array_equal(np.sort(rows), pos.astype(np.uint64)), f"k={k} {pat}: index scan"
        check_index(x, s, flt, sets, f"k={k} {pat}")
        gk, gs, gp, n_out = ctx.generate_kmers_table(one, k, flt)
        assert n_out == len(pos) and np.array_equal(gp, pos.astype(np.uint64)) and not gs.any(), f"k={k} {pat}: one-sequence table"
        assert np.array_equal(gk, s.keys(k)[pos])
    assert some > 100
    one.free()
