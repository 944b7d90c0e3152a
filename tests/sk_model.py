"""A plain numpy restatement of the super-k-mer record contract -- what sk_device.hpp documents as shared between the
ranks of a sharded count.  No GPU, no package import: tests/test_sk_records.py holds the engine's records against it.

Written from the header's comments, not from the kernels:

record      16 bytes = two 64-bit words.  First word: bases 0..31 of the run, two bits each, base 0 lowest.  Second word:
            bases 32..53 in bits 0..43, len - 1 in bits 44..48 (len = the record's k-mers), d1 in bits 49..57, d2 in bits
            59..62, NULL in bit 63.  Bit 58 is SK_REC_MULTI.  Bit 58 clear: all k-mers of the record have their leftmost
            minimum m-mer at ONE place, and bits 39..43 hold that place's offset `a` from the record's first base (such a
            record has at most 2k - m <= 49 bases, so its payload ends below bit 34 of the second word).  Bit 58 set:
            nothing is known about the place; bits 39..43 are payload.
            k-mer j of a record = bits [2j, 2j + 2k) of the 108 payload bits.
minimizer   m = 15 for k >= 23, 13 for k = 21 and 22, 12 for k = 20; a k-mer's window holds w = k - m + 1 m-mers; a record
            holds at most lmax = min(32, 54 - k + 1) k-mers.
hash        of an m-mer value v, in 32-bit arithmetic: (v & 0xFFFFFF) * 0x9E3779 + ((v >> 24) & (2^(2m-24) - 1)) * 0x85EBCB.
            The m-mers are ordered by the hash's bits 7..31; ties go to the leftmost position.  The minimum m-mer of a
            k-mer is therefore a function of the k-mer's content: kmer_minimum() computes it from the k-mer's bits alone,
            sequence_minima() by sliding a window over a sequence, and the two must agree.
digits      d0 = ((g >> 16) * c0) >> 16 with g = (hash bits 7..30) * 0x9E3779 in 32 bits, c0 = dnagpu_sk_buckets(...)
            (sk_digit_word multiplies with the 24-bit multiply: of the 25 ordering bits the top one does not enter d0);
            f = v * 0x9E3779B1 in 32 bits, d2 = (f >> 19) & 15, d1 = (f >> 23) & (2^b1 - 1).
            b1 is not exposed by the C-ABI and the geometry that chooses it is not restated here.  d1 is checked as "a function
            of v, equal to f >> 23 masked to ONE width b1 <= 9 common to all records of a call": infer_b1() takes the
            smallest width that holds every d1 seen, and the caller compares every record's d1 with d1_of(v, that width).
"""
import numpy as np

U64 = np.uint64
MASK32 = 0xFFFFFFFF

REC_MULTI_BIT = 58
REC_NULL_BIT = 63
POS_SHIFT = 39
POS_MASK = 31
LEN_SHIFT = 44
D1_SHIFT = 49
D1_MASK = 0x1FF
D2_SHIFT = 59
D2_MASK = 15
PAYLOAD_HI_BITS = 44                   # bases 32..53
MAX_BASES = 54


def mlen(k):
    return 15 if k >= 23 else (13 if k >= 21 else 12)


def window(k):
    return k - mlen(k) + 1


def lmax(k):
    return min(32, MAX_BASES - k + 1)


# ------------------------------------------------------------------ hash, order, digits

def mmer_hash(v, m):
    """the 32-bit hash of m-mer values v (any integer array; the bits above 2m must be clear)"""
    v = np.asarray(v).astype(np.uint64)
    lo = v & U64(0xFFFFFF)
    hi = (v >> U64(24)) & U64((1 << (2 * m - 24)) - 1)
    return ((lo * U64(0x9E3779) + hi * U64(0x85EBCB)) & U64(MASK32)).astype(np.uint32)


def mmer_order(v, m):
    """what the m-mers are ordered by: the hash's bits 7..31"""
    return mmer_hash(v, m) >> np.uint32(7)


def d0_of(v, m, c0):
    h = mmer_hash(v, m).astype(np.uint64)
    g = (((h >> U64(7)) & U64(0xFFFFFF)) * U64(0x9E3779)) & U64(MASK32)
    return ((((g >> U64(16)) * U64(c0)) & U64(MASK32)) >> U64(16)).astype(np.uint32)


def fine_word(v):
    return ((np.asarray(v).astype(np.uint64) * U64(0x9E3779B1)) & U64(MASK32)).astype(np.uint32)


def d2_of(v):
    return (fine_word(v) >> np.uint32(19)) & np.uint32(15)


def d1_of(v, b1):
    return (fine_word(v) >> np.uint32(23)) & np.uint32((1 << b1) - 1)


def infer_b1(d1):
    """the smallest width that holds every d1 seen (0 for no records or all-zero digits)"""
    d1 = np.asarray(d1)
    return int(d1.max()).bit_length() if d1.size else 0


# ------------------------------------------------------------------ minimum m-mers

def kmer_minimum(kmers, k):
    """-> (v, off): value and in-k-mer offset of the leftmost minimum m-mer of every k-mer, from the k-mer's bits alone"""
    kmers = np.asarray(kmers, dtype=np.uint64)
    m, w = mlen(k), window(k)
    mmask = U64((1 << (2 * m)) - 1)
    vals = np.stack([(kmers >> U64(2 * i)) & mmask for i in range(w)], axis=1)      # (n, w)
    off = np.argmin(mmer_order(vals, m), axis=1)                                       # (argmin: the first of equal minima)
    v = np.take_along_axis(vals, off[:, None], axis=1)[:, 0]
    return v.astype(np.uint32), off.astype(np.int64)


def mmer_values(codes, m):
    """the value of the m-mer at every base position of a sequence of 2-bit codes (n - m + 1 of them)"""
    c = np.asarray(codes).astype(np.uint64)
    n = len(c) - m + 1
    v = np.zeros(max(n, 0), dtype=np.uint64)
    for j in range(m):
        v |= c[j:j + n] << U64(2 * j)
    return v


def sequence_minima(codes, k, chunk=1 << 18):
    """-> (pos, v): for every k-mer (row) of the sequence, the base position and the value of its leftmost minimum m-mer"""
    m, w = mlen(k), window(k)
    v = mmer_values(codes, m)
    order = mmer_order(v, m)
    rows = len(v) - w + 1
    pos = np.empty(max(rows, 0), dtype=np.int64)
    for r0 in range(0, rows, chunk):
        r1 = min(r0 + chunk, rows)
        win = np.lib.stride_tricks.sliding_window_view(order[r0:r1 + w - 1], w)
        pos[r0:r1] = np.argmin(win, axis=1) + np.arange(r0, r1)
    return pos, v[pos].astype(np.uint32)


def mean_run_length(codes, k):
    """rows per run of one (hash, position) minimum: what a record of a plain tile is (no tile cuts here)"""
    pos, _ = sequence_minima(codes, k)
    return len(pos) / (1 + int(np.count_nonzero(np.diff(pos))))


# ------------------------------------------------------------------ records

def kmers_of_codes(codes, k):
    """the k-mer at every position of a sequence of 2-bit codes, as the engine's keys (base 0 in the lowest bits)"""
    return mmer_values(codes, k)


def encode(codes, k, d1=0, d2=0, a=None, multi=False, null=False):
    """One record over the bases `codes` (k .. 54 of them: len = len(codes) - k + 1 k-mers) -> (lo, hi) as Python ints.
    a = the minimum m-mer's offset for a record without SK_REC_MULTI; multi=True sets bit 58 instead."""
    nb = len(codes)
    length = nb - k + 1
    if not (1 <= length <= lmax(k) and nb <= MAX_BASES):
        raise ValueError(f"a record of {nb} bases at k = {k}")
    if multi == (a is not None):
        raise ValueError("a record either carries its m-mer's offset or has SK_REC_MULTI set")
    pay = 0
    for i, c in enumerate(codes):
        pay |= (int(c) & 3) << (2 * i)
    lo, hi = pay & 0xFFFFFFFFFFFFFFFF, pay >> 64
    if a is not None:
        if not 0 <= a <= POS_MASK or nb > 2 * k - mlen(k):
            raise ValueError(f"offset {a} / {nb} bases in a record without SK_REC_MULTI")
        hi |= a << POS_SHIFT
    else:
        hi |= 1 << REC_MULTI_BIT
    if not (0 <= d1 <= D1_MASK and 0 <= d2 <= D2_MASK):
        raise ValueError("digits out of range")
    hi |= ((length - 1) << LEN_SHIFT) | (d1 << D1_SHIFT) | (d2 << D2_SHIFT) | ((1 << REC_NULL_BIT) if null else 0)
    return lo, hi


def encode_many(recs):
    """[(lo, hi)] -> the flat uint64 array a device buffer takes"""
    out = np.empty(2 * len(recs), dtype=np.uint64)
    out[0::2] = np.array([r[0] for r in recs], dtype=np.uint64)
    out[1::2] = np.array([r[1] for r in recs], dtype=np.uint64)
    return out


class Decoded:
    """the fields of n records and their k-mers (see decode)"""


def decode(records, k):
    """records: 2n uint64 words (or an (n, 2) array).  -> Decoded with, per record: lo, hi, length, d1, d2, null, multi,
    a (the offset field; meaningful where multi is False), pay_hi (the payload bits of the second word: the offset field
    is no payload where multi is False), and the k-mers of all records flattened in record order: kmers, kmer_rec (the
    record's index) and kmer_j (the k-mer's index in it); first[r] = index of record r's first k-mer."""
    w = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 2)
    d = Decoded()
    d.k = k
    d.lo, d.hi = w[:, 0].copy(), w[:, 1].copy()
    d.n = len(d.lo)
    d.length = ((d.hi >> U64(LEN_SHIFT)) & U64(31)).astype(np.int64) + 1
    d.d1 = ((d.hi >> U64(D1_SHIFT)) & U64(D1_MASK)).astype(np.uint32)
    d.d2 = ((d.hi >> U64(D2_SHIFT)) & U64(D2_MASK)).astype(np.uint32)
    d.null = (d.hi >> U64(REC_NULL_BIT)) != 0
    d.multi = ((d.hi >> U64(REC_MULTI_BIT)) & U64(1)) != 0
    d.a = ((d.hi >> U64(POS_SHIFT)) & U64(POS_MASK)).astype(np.int64)
    d.pay_hi = d.hi & np.where(d.multi, U64((1 << PAYLOAD_HI_BITS) - 1), U64((1 << POS_SHIFT) - 1))
    d.n_bases = d.length + k - 1
    d.first = np.concatenate([[0], np.cumsum(d.length)]).astype(np.int64)
    total = int(d.first[-1])
    d.kmer_rec = np.repeat(np.arange(d.n, dtype=np.int64), d.length)
    d.kmer_j = np.arange(total, dtype=np.int64) - d.first[:-1][d.kmer_rec]
    sh = (2 * d.kmer_j).astype(np.uint64)
    lo, ph = d.lo[d.kmer_rec], d.pay_hi[d.kmer_rec]
    up = np.where(sh > 0, ph << ((U64(64) - sh) & U64(63)), U64(0))                  # (a shift by 64 is no shift in numpy)
    kmask = U64((1 << (2 * k)) - 1)
    d.kmers = ((lo >> sh) | up) & kmask
    return d


def payload_above(d):
    """per record: the payload bits at and above 2 * n_bases (the contract wants none set)"""
    nb2 = 2 * d.n_bases
    lo_keep = np.where(nb2 >= 64, U64(0), ~((U64(1) << np.minimum(nb2, 63).astype(np.uint64)) - U64(1)))
    hi_sh = np.clip(nb2 - 64, 0, 63).astype(np.uint64)
    hi_keep = ~((U64(1) << hi_sh) - U64(1))
    return (d.lo & lo_keep) | (d.pay_hi & hi_keep)


def mmer_at(d, off):
    """per record: the m-mer value at base offset off[r] of the payload (off + m <= 54)"""
    m = mlen(d.k)
    sh = (2 * np.asarray(off, dtype=np.int64))
    out = np.zeros(d.n, dtype=np.uint64)
    lo_part = sh < 64
    s = np.where(lo_part, sh, 0).astype(np.uint64)
    up = np.where(s > 0, d.pay_hi << ((U64(64) - s) & U64(63)), U64(0))
    out = np.where(lo_part, (d.lo >> s) | up, d.pay_hi >> np.where(lo_part, 0, sh - 64).astype(np.uint64))
    return (out & U64((1 << (2 * m)) - 1)).astype(np.uint32)
