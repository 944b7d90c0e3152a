"""The three WHERE operators over k-mers -- `=` (kmer_eq, dna.c:655-668), `^@` (starts_with, dna.c:842-866) and `@>` (contains +
nucleotide_matches, dna.c:1064-1135) -- as the plain reference of tests/test_operator_semantics.py: numpy only, no device, no
product code, one base at a time.  Every operator is a list of k per-position SETS of allowed codes (4 bits: bit0 A, bit1 T,
bit2 C, bit3 G; the codes are A=0 T=1 C=2 G=3, dna.c:120-123), or None where the reference's operator can match nothing; a row
matches when every one of its k bases lies in its position's set."""
import numpy as np

# The IUPAC letters as the comment block of nucleotide_matches lists them (dna.c:1064-1086): the set of bases a letter stands
# for.  'U' is compared with the decoded base, which is never 'U': the empty set.
IUPAC_BASES = {"A": "A", "T": "T", "C": "C", "G": "G", "U": "",
               "W": "AT", "S": "CG", "M": "AC", "K": "GT", "R": "AG", "Y": "CT",
               "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
CODE = {"A": 0, "T": 1, "C": 2, "G": 3}
IUPAC = {letter: sum(1 << CODE[b] for b in bases) for letter, bases in IUPAC_BASES.items()}
LETTERS = "ATCGUWSMKRYBDHVN"
LETTER_OF_SET = {s: c for c, s in IUPAC.items()}
assert len(LETTER_OF_SET) == 16

# ALLOWED[set][code]
ALLOWED = np.array([[bool((s >> c) & 1) for c in range(4)] for s in range(16)])


def codes_of(words, n):
    """the packed stream (32 bases per uint64, base j of a word at bits 2j, dna.c:178-202) as n 2-bit codes"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    out = np.empty((len(w), 32), dtype=np.uint8)
    for j in range(32):
        out[:, j] = (w >> np.uint64(2 * j)) & np.uint64(3)
    return out.reshape(-1)[:n].copy()


def words_of(codes):
    """the inverse of codes_of: the bits behind the last base are 0 (dna.c:186)"""
    n = len(codes)
    c = np.zeros((n + 31) // 32 * 32, dtype=np.uint64)
    c[:n] = codes
    c = c.reshape(-1, 32)
    w = np.zeros(len(c), dtype=np.uint64)
    for j in range(32):
        w |= c[:, j] << np.uint64(2 * j)
    return w


def keys_of(codes, k):
    """the key of every row: base i of the k-mer at bits 2i (generate_kmers, dna.c:760-815)"""
    rows = max(len(codes) - k + 1, 0)
    keys = np.zeros(rows, dtype=np.uint64)
    for i in range(k):
        keys |= codes[i:i + rows].astype(np.uint64) << np.uint64(2 * i)
    return keys


def rows_matching(codes, k, sets):
    """bool per row of generate_kmers(codes, k): AND over the k positions of `base i of the row is in sets[i]`"""
    rows = max(len(codes) - k + 1, 0)
    if sets is None:
        return np.zeros(rows, dtype=bool)
    assert len(sets) == k
    m = np.ones(rows, dtype=bool)
    for i in range(k):
        if sets[i] != 15:                            # (N allows every code: nothing to AND)
            m &= ALLOWED[sets[i]][codes[i:i + rows]]
    return m


def key_matches(key, k, sets):
    """the same for one value"""
    return sets is not None and all(ALLOWED[sets[i]][(int(key) >> (2 * i)) & 3] for i in range(k))


def _stray_bits(length, bits):
    return length < 32 and (int(bits) >> (2 * length)) != 0


def sets_of_equals(k, qlen, qbits):
    """kmer = q: lengths, then bits (dna.c:658-667).  None: a q of another length, or bits behind q's own length"""
    if qlen != k or _stray_bits(qlen, qbits):
        return None
    return [1 << ((int(qbits) >> (2 * i)) & 3) for i in range(k)]


def sets_of_prefix(k, plen, pbits):
    """kmer ^@ prefix: the first plen bases (dna.c:862-863; a prefix longer than k is the reference's ERROR, dna.c:854-856, and
    not this function's business).  None: bits behind the prefix's own length.  A 32-base prefix compares all 64 bits."""
    assert 0 <= plen <= k
    if _stray_bits(plen, pbits):
        return None
    return [1 << ((int(pbits) >> (2 * i)) & 3) for i in range(plen)] + [15] * (k - plen)


def sets_of_pattern(text):
    """pattern @> kmer: the IUPAC text itself (a pattern of another length is the reference's ERROR, dna.c:1106-1108).  None: a
    'U' anywhere"""
    sets = [IUPAC[c] for c in text]
    return None if 0 in sets else sets


def pattern_of(sets):
    return "".join(LETTER_OF_SET[s] for s in sets)


def table_rows(starts, n, k):
    """bool per stream row: the row is a table row iff no sequence starts among the k - 1 bases behind its first base"""
    rows = max(n - k + 1, 0)
    mark = np.zeros(n + 1, dtype=bool)
    mark[np.asarray(starts, dtype=np.int64)] = True
    ok = np.ones(rows, dtype=bool)
    for j in range(1, k):
        ok &= ~mark[j:j + rows]
    return ok
