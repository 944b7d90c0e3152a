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
            b1 is not exposed by the C-ABI.  d1 is checked as "a function of v, equal to f >> 23 masked to ONE width
            b1 <= 9 common to all records of a call": infer_b1() takes the smallest width that holds every d1 seen, and the
            caller compares every record's d1 with d1_of(v, that width).

The second half restates the HOST's rules of levels 1 and 2 (sk_host.hip, sk_level1_kernels.hip) -- geometry(), spec_cap(),
chunk_len(), even(), received_cap(), route(), heavy() -- and crafted_stream() makes record streams that put a chosen number
of records into a chosen (coarse bucket, d1, d2): tests/test_sk_levels12.py feeds them to dnagpu_count_records.  These ARE
written from the host code, one function per rule, each with the values worked out by hand that its test asserts.
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


# ------------------------------------------------------------------ the host's rules of levels 1 and 2

SK_LEAF_MEAN = 2500                    # planned k-mers per final bucket (sk_host.hip)
SK_B1_MAX = 9                          # level 1 splits a coarse bucket at most 512 ways
SK_MAX_C0 = 256                        # most coarse buckets (sk_device.hpp)
SK_MID_LIMIT = 1 << 27                 # k-mers beyond which a mid bucket is heavy (unforced)
SK_MID_RECORDS = 1 << 16               # records beyond which a mid bucket is heavy (unforced)
SK1_TILE = 8192                        # records of a tile of sk_scatter1
SK1_STAGE = SK1_TILE // 2 + 64         # records its stage holds: the half split of a full tile
SKR_TILE = 8192                        # records of a tile of sk_regroup: longer mid buckets take the LONG kernel
# dnagpu_set_debug flags that the rules below read (dnagpu.h; the GPU tie test compares them with the binding's)
DEBUG_FORCE_SUPERKMER, DEBUG_HEAVY_EXPAND, DEBUG_NO_SPEC1, DEBUG_SPEC1_OVERFLOW, DEBUG_SAMPLE1 = 2, 4, 16, 32, 512


class Geometry:
    """b1, c0n, r0bits, mid_limit of one (global_rows, k, forced); n_coarse = 2^r0bits, R = 2^b1"""

    def __repr__(self):
        return f"Geometry(b1={self.b1}, c0n={self.c0n}, r0bits={self.r0bits}, mid_limit={self.mid_limit})"


def geometry(global_rows, k, forced=False):
    """restates sk_geometry (sk_host.hip).  By hand, k = 31 (leaf mean 2500): 40 000 rows -> 16 final, 1 mid bucket, b1 = 1,
    c0n = 1; 160 000 -> 64, 4, b1 = 2, c0n = 1; 10 300 000 -> 4120, 258, b1 = 9, c0n = 1; 21 000 000 -> 8400, 525, b1 = 9,
    c0n = 2.  r0bits = 1 in all four (never 0: one coarse bucket still has two coarse nodes, the second empty).
    forced (DNAGPU_DEBUG_FORCE_SUPERKMER): mid_limit = 3 (rows / (c0n 2^b1) + 1); k = 23, 40 000 rows: leaf mean 225 * 10,
    17 final, 2 mid buckets, b1 = 1, c0n = 1, mid_limit = 3 * 20 001 = 60 003."""
    g = Geometry()
    leaf_mean = min(SK_LEAF_MEAN, 225 * (k - mlen(k) + 2))
    n_final = max(global_rows // leaf_mean, 16)
    n_mid = (n_final + 15) // 16
    g.b1 = 1
    while g.b1 < SK_B1_MAX and (1 << g.b1) < n_mid:
        g.b1 += 1
    g.c0n = min((n_mid + (1 << g.b1) - 1) >> g.b1, SK_MAX_C0)
    g.r0bits = 1
    while (1 << g.r0bits) < g.c0n:
        g.r0bits += 1
    g.mid_limit = 3 * (global_rows // (g.c0n << g.b1) + 1) if forced else SK_MID_LIMIT
    g.n_coarse, g.R = 1 << g.r0bits, 1 << g.b1
    return g


def spec_cap(length, R):
    """restates sk_spec_cap (sk_level1_kernels.hip): the slots of one region of a speculative level 1.  By hand:
    (8192, 2): 9216 / 2 + 79 = 4687 -> 4680; (40000, 4): 45000 / 4 + 79 = 11329 -> 11328; (60000, 512): 67500 / 512 = 131,
    + 79 = 210 -> 208."""
    return (((length + (length >> 3)) // R) + 72 + 7) & ~7


def spec_span(length, bits):
    """restates sk_spec_span: the slots of all 2^bits regions of a coarse bucket of `length` records (none for none)"""
    return spec_cap(length, 1 << bits) << bits if length else 0


def chunk_len(n_recs, target=4096, tile=SK1_TILE):
    """restates sk_chunk_len (sk_host.hip): ~target chunks of whole tiles, four tiles at least.  By hand: up to
    4096 * 32768 = 134 217 728 records the quotient is at most 32768 = four tiles, one more record gives five tiles."""
    length = max(4 * tile, (n_recs + target - 1) // target)
    return (length + tile - 1) // tile * tile


def even(lens, tol=1.02):
    """restates sk_even (sk_host.hip), in double precision as there: big * used <= tol * total + 64 * used.  By hand:
    [20946, 20000]: 41892 <= 1.02 * 40946 + 128 = 41892.92 holds; [20947, 20000]: 41894 <= 41893.94 does not."""
    lens = [int(x) for x in lens]
    tot, big, used = sum(lens), max(lens, default=0), sum(1 for x in lens if x)
    return float(big) * float(used) <= tol * float(tot) + 64.0 * float(used)


def received_cap(blen, b1):
    """restates sk_received_cap (sk_host.hip): the records the landing buffer of dnagpu_count_records has room for -- the
    records or, where they stay below 2^32, the regions of a speculative level 1, whichever is more"""
    n = sum(int(x) for x in blen)
    span = sum(spec_span(min(int(x), 0xFFFFFFFF), b1) for x in blen)
    return max(n, span) if span <= 0xFFFFFFFF else n


def route(lens, flags, b1=SK_B1_MAX):
    """restates sk_l1_route_plain (sk_host.hip) as dnagpu_count_records meets it (the coarse buckets' lengths are known and
    the landing buffer is received_cap): "Exact" under DNAGPU_DEBUG_NO_SPEC1 or without records (no chunk), "Speculative" for
    even buckets whose regions fit, "Sampled" for uneven ones or under DNAGPU_DEBUG_SAMPLE1 (the regions then come from
    sk_sample1; whether the sweep is speculative after it is decided by their total)."""
    lens = [int(x) for x in lens]
    if (flags & DEBUG_NO_SPEC1) or not any(lens):
        return "Exact"
    if even(lens, 1.02) and not (flags & DEBUG_SAMPLE1):
        span = sum(spec_span(x, b1) for x in lens)
        return "Speculative" if span <= received_cap(lens, b1) and span <= 0xFFFFFFFF else "Exact"
    return "Sampled"


def heavy(kmers, records, mid_limit, forced):
    """restates is_heavy of sk_l1_census (sk_host.hip): a mid bucket of more than mid_limit k-mers or -- unforced -- more than
    SK_MID_RECORDS records"""
    return kmers > mid_limit or (not forced and records > SK_MID_RECORDS)


# ------------------------------------------------------------------ crafted record streams

def record_fields(records):
    """-> (d1, d2, length, null) per record, without cutting the k-mers (decode does that)"""
    hi = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 2)[:, 1]
    return (((hi >> U64(D1_SHIFT)) & U64(D1_MASK)).astype(np.int64), ((hi >> U64(D2_SHIFT)) & U64(D2_MASK)).astype(np.int64),
            ((hi >> U64(LEN_SHIFT)) & U64(31)).astype(np.int64) + 1, (hi >> U64(REC_NULL_BIT)) != 0)


def _pack_payload(codes):
    """(n, nb) 2-bit codes -> the two payload words of n records over all nb bases"""
    c = np.asarray(codes).astype(np.uint64) & U64(3)
    lo = np.zeros(len(c), dtype=np.uint64)
    hi = np.zeros(len(c), dtype=np.uint64)
    for i in range(c.shape[1]):
        if i < 32:
            lo |= c[:, i] << U64(2 * i)
        else:
            hi |= c[:, i] << U64(2 * (i - 32))
    return lo, hi


def encode_windows(lo, hi, length, k, d1, d2, null=False):
    """encode(codes[:length + k - 1], k, d1, d2, multi=True, null=null) for many records at once: lo / hi = the payload words
    of the whole strings (_pack_payload), cut to the record's bases here.  -> the flat uint64 array of the records.
    (crafted_stream holds a sample of every stream against encode itself.)"""
    length = np.asarray(length, dtype=np.int64)
    if len(length) and not (1 <= length.min() and length.max() <= lmax(k)):
        raise ValueError(f"records of {int(length.min())} .. {int(length.max())} k-mers at k = {k}")
    nb2 = 2 * (length + k - 1)
    lo_m = np.where(nb2 >= 64, ~U64(0), (U64(1) << np.minimum(nb2, 63).astype(np.uint64)) - U64(1))
    hi_m = (U64(1) << np.clip(nb2 - 64, 0, 63).astype(np.uint64)) - U64(1)
    out = np.empty((len(length), 2), dtype=np.uint64)
    out[:, 0] = lo & lo_m
    out[:, 1] = (hi & hi_m) | U64(1 << REC_MULTI_BIT) | ((length - 1).astype(np.uint64) << U64(LEN_SHIFT)) | \
        (np.asarray(d1).astype(np.uint64) << U64(D1_SHIFT)) | (np.asarray(d2).astype(np.uint64) << U64(D2_SHIFT)) | \
        (U64(1 << REC_NULL_BIT) if null else U64(0))
    return out.reshape(-1)


def _clashing(kmers, triple, owner):
    """the owners (an id per k-mer) of k-mers whose value also occurs under another triple"""
    order = np.argsort(kmers, kind="stable")
    ks, ts = kmers[order], triple[order]
    clash = (ks[1:] == ks[:-1]) & (ts[1:] != ts[:-1])
    return np.unique(owner[order][1:][clash])


def check_contract(records, bucket_of_record, k):
    """The engine's contract on a stream: no k-mer value occurs under two different (coarse bucket, d1, d2) -- equal k-mers
    must meet in ONE final bucket.  NULL records do not count.  Raises ValueError naming the first offending record."""
    w = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 2)
    live = np.flatnonzero((w[:, 1] >> U64(REC_NULL_BIT)) == 0)
    dec = decode(w[live], k)
    triple = (np.asarray(bucket_of_record, dtype=np.int64)[live] << 13) | (dec.d1.astype(np.int64) << 4) | dec.d2.astype(np.int64)
    bad = _clashing(dec.kmers, triple[dec.kmer_rec], dec.kmer_rec)
    if len(bad):
        raise ValueError(f"{len(bad)} records hold a k-mer that also occurs under another (bucket, d1, d2); first: record {int(live[bad[0]])}")


def _lengths(want, n, lm, rng):
    if want is None:
        want = (1, lm)
    if isinstance(want, tuple):
        return rng.integers(want[0], want[1] + 1, n).astype(np.int64)
    if np.ndim(want) == 0:
        return np.full(n, int(want), dtype=np.int64)
    out = np.asarray(want, dtype=np.int64)
    if len(out) != n:
        raise ValueError(f"{len(out)} lengths for {n} records")
    return out


def _interleaved(bucket, cls, run):
    """the order that deals every bucket's records out class by class, `run` records at a time (a class that has run out is
    passed over): run = 8192 over d1 gives tiles of one digit each, run = 1 over d2 gives every lane another d2"""
    n = len(bucket)
    by = np.lexsort((np.arange(n), cls, bucket))
    b, c = bucket[by], cls[by]
    new = np.ones(n, dtype=bool)
    new[1:] = (b[1:] != b[:-1]) | (c[1:] != c[:-1])
    first = np.flatnonzero(new)
    r = np.arange(n) - np.repeat(first, np.diff(np.append(first, n)))
    return by[np.lexsort((r, c, r // run, b))]


def crafted_stream(k, spec, rng):
    """A record stream with a chosen number of records in chosen (coarse bucket, d1, d2) -> (records: uint64[2n],
    bucket_of_record: int64[n], truth_kmers: uint64[...]).  The records of a coarse bucket lie together, the buckets in
    ascending order (one piece per bucket for dnagpu_count_records).  spec is a dict:
      "groups"  [(bucket, d1, d2, n, lengths)]: n records for that final bucket; lengths = their k-mers: one number, (lo, hi)
                for uniform draws, an array of n, or None for 1 .. lmax(k)
      "copies"  (default 8) a group of n records draws its payload from a pool of ceil(n / copies) random "reads" of its own,
                record i from read i mod pool: every read is used `copies` times (windows from its first base, so copies of
                different lengths share their common k-mers)
      "order"   of the real records inside every bucket: "shuffled" (default), "digit" (sorted by d1, then d2), "tiles"
                (SK1_TILE records of one d1, then of the next: tile-interleaved), "lanes" (record i has the i-th d2 in turn),
                "runs64" (64 records of one d2, 64 of the next), or a function (bucket, d1, d2, rng) -> permutation of the
                records (given per record, grouped as listed) that keeps the buckets together and ascending
      "nulls"   {bucket: positions}: NULL records (bit 63; random payload, digits and length) at these positions of the
                bucket's final layout, the real records filling the others in their order
    All records have SK_REC_MULTI set (nothing is claimed about their minimum m-mers: d1 and d2 are free).
    The engine's contract -- no k-mer value under two different (bucket, d1, d2) -- is established here: the k-mers of all
    reads (decode of the reads as records of lmax k-mers) are compared, and every read that holds a k-mer of another group
    is drawn again, until none does (at k = 20 random reads do collide).  crafted_stream.redrawn counts the reads redrawn
    by the last call.  A few records of every stream are held against encode()."""
    groups = spec["groups"]
    copies, order = int(spec.get("copies", 8)), spec.get("order", "shuffled")
    lm = lmax(k)
    nb_full = lm + k - 1
    G = len(groups)
    g_bucket = np.array([g[0] for g in groups], dtype=np.int64).reshape(G)
    g_d1 = np.array([g[1] for g in groups], dtype=np.int64).reshape(G)
    g_d2 = np.array([g[2] for g in groups], dtype=np.int64).reshape(G)
    g_n = np.array([g[3] for g in groups], dtype=np.int64).reshape(G)
    if G and (g_d1.min() < 0 or g_d1.max() > D1_MASK or g_d2.min() < 0 or g_d2.max() > D2_MASK or g_n.min() < 0):
        raise ValueError("digits or counts out of range")
    if len(set(zip(g_bucket.tolist(), g_d1.tolist(), g_d2.tolist()))) != G:
        raise ValueError("a (bucket, d1, d2) listed twice")
    n_real = int(g_n.sum())
    grp = np.repeat(np.arange(G), g_n)
    if G and all(g[4] is groups[0][4] for g in groups) and (groups[0][4] is None or np.ndim(groups[0][4]) == 0 or
                                                               isinstance(groups[0][4], tuple)):
        length = _lengths(groups[0][4], n_real, lm, rng)       # (one rule for all groups: one draw)
    else:
        length = np.concatenate([_lengths(g[4], int(g[3]), lm, rng) for g in groups]) if G else np.zeros(0, dtype=np.int64)
    # ---- the pool of reads, group by group, free of k-mers shared between groups
    g_pool = (g_n + copies - 1) // copies
    pool_first = np.concatenate([[0], np.cumsum(g_pool)])
    pool_grp = np.repeat(np.arange(G), g_pool)
    codes = rng.integers(0, 4, (int(pool_first[-1]), nb_full), dtype=np.uint8)
    pool_triple = (g_bucket << 13 | g_d1 << 4 | g_d2)[pool_grp]
    crafted_stream.redrawn = 0
    while True:
        plo, phi = _pack_payload(codes)
        dec = decode(encode_windows(plo, phi, np.full(len(codes), lm), k, g_d1[pool_grp], g_d2[pool_grp]), k)
        bad = _clashing(dec.kmers, pool_triple[dec.kmer_rec], dec.kmer_rec)
        if not len(bad):
            break
        codes[bad] = rng.integers(0, 4, (len(bad), nb_full), dtype=np.uint8)
        crafted_stream.redrawn += len(bad)
    rank = np.arange(n_real) - np.repeat(np.concatenate([[0], np.cumsum(g_n)])[:-1], g_n)
    read = pool_first[grp] + rank % np.maximum(g_pool[grp], 1)
    # ---- the order of the real records
    bucket, d1, d2 = g_bucket[grp], g_d1[grp], g_d2[grp]
    if callable(order):
        perm = np.asarray(order(bucket, d1, d2, rng), dtype=np.int64)
        if not np.array_equal(np.sort(perm), np.arange(n_real)) or np.any(np.diff(bucket[perm]) < 0):
            raise ValueError("order: not a permutation that keeps the buckets together and ascending")
    elif order == "shuffled":
        perm = np.lexsort((rng.random(n_real), bucket))
    elif order == "digit":
        perm = np.lexsort((np.arange(n_real), d2, d1, bucket))
    elif order == "tiles":
        perm = _interleaved(bucket, d1, SK1_TILE)
    elif order == "lanes":
        perm = _interleaved(bucket, d2, 1)
    elif order == "runs64":
        perm = _interleaved(bucket, d2, 64)
    else:
        raise ValueError(f"order {order!r}")
    real = encode_windows(plo[read[perm]], phi[read[perm]], length[perm], k, d1[perm], d2[perm]).reshape(-1, 2)
    for i in rng.integers(0, max(n_real, 1), min(n_real, 4)):
        j = perm[i]
        want = encode(codes[read[j]][:length[j] + k - 1], k, d1=int(d1[j]), d2=int(d2[j]), multi=True)
        if (int(real[i, 0]), int(real[i, 1])) != want:
            raise AssertionError(f"record {int(i)} differs from encode()")
    real_bucket = bucket[perm]
    # ---- NULL records
    nulls = {int(b): np.unique(np.asarray(p, dtype=np.int64)) for b, p in spec.get("nulls", {}).items() if len(p)}
    if not nulls:
        records, bucket_of_record = real, real_bucket
    else:
        parts, bparts = [], []
        for b in sorted(set(real_bucket.tolist()) | set(nulls)):
            mine = real[real_bucket == b]
            pos = nulls.get(b, np.zeros(0, dtype=np.int64))
            total = len(mine) + len(pos)
            if len(pos) and (pos[0] < 0 or pos[-1] >= total):
                raise ValueError(f"NULL positions outside bucket {b}'s {total} records")
            nlo, nhi = _pack_payload(rng.integers(0, 4, (len(pos), nb_full), dtype=np.uint8))
            out = np.empty((total, 2), dtype=np.uint64)
            is_null = np.zeros(total, dtype=bool)
            is_null[pos] = True
            out[is_null] = encode_windows(nlo, nhi, rng.integers(1, lm + 1, len(pos)), k, rng.integers(0, D1_MASK + 1, len(pos)),
                                          rng.integers(0, D2_MASK + 1, len(pos)), null=True).reshape(-1, 2)
            out[~is_null] = mine
            parts.append(out)
            bparts.append(np.full(total, b, dtype=np.int64))
        records, bucket_of_record = np.concatenate(parts), np.concatenate(bparts)
    live = (records[:, 1] >> U64(REC_NULL_BIT)) == 0
    truth = decode(records[live], k).kmers
    return np.ascontiguousarray(records).reshape(-1), bucket_of_record, truth


crafted_stream.redrawn = 0
