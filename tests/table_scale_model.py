"""A table of sequences large enough to pass the third level of the shared u32 scan (more than 1024 x 2048 = 2^21 entries), and
its exact answers, in plain numpy.  It runs no code of the project.

Every sequence of the table is a whole copy of one entry of a small POOL of pairwise distinct contents, so every per-sequence
answer is per_pool_answer[p[i]] and every per-table answer is a sum over pool entries weighted by their multiplicity: the
references cost what the pool costs, whatever the table's size.  tests/test_table_scale.py shows the references right against
independent per-sequence answers at 5,000 sequences, and then uses them as the judge at 2^21 + 4096 + 5.

Codes: A 0, T 1, C 2, G 3; base i of a stream sits at bits [2i mod 64, +2) of word i / 32; base i of a k-mer key at bits
[2i, 2i + 2); the complement of a code is code ^ 1; text order is A < T < C < G with base 0 most significant."""
import numpy as np

CARRY = 1 << 21                       # entries the scan's block-sum sweep covers before it carries: 1024 sums of 2048 values
SCAN_TILE = 2048
N_FULL = CARRY + 2 * SCAN_TILE + 5    # four scan blocks past the first sweep, the last one partial
POOL_SHORT = 4096
EDGE_LENGTHS = (31, 32, 33, 63, 64, 65)
LONG_LENGTHS = (2_100, 66_000, 70_000)
LETTERS = np.frombuffer(b"ATCG", dtype=np.uint8)
U64_MAX = 2 ** 64 - 1


# ------------------------------------------------------------------ codes, words, keys

def pack_codes(codes):
    """uint8 codes -> packed uint64 words (tail bits zero)"""
    n = len(codes)
    buf = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    buf[:n] = codes
    q = buf.reshape(-1, 4)
    by = q[:, 0] | (q[:, 1] << np.uint8(2)) | (q[:, 2] << np.uint8(4)) | (q[:, 3] << np.uint8(6))
    return np.ascontiguousarray(by, dtype=np.uint8).view("<u8").astype(np.uint64, copy=False)


def unpack_words(words, n):
    """packed words -> uint8 codes of the first n bases"""
    by = np.ascontiguousarray(words, dtype="<u8").view(np.uint8)
    codes = np.empty((len(by), 4), dtype=np.uint8)
    for j in range(4):
        codes[:, j] = (by >> np.uint8(2 * j)) & np.uint8(3)
    return codes.reshape(-1)[:n]


def text_of(codes):
    return LETTERS[codes].tobytes().decode()


def mask_of(k):
    return np.uint64((1 << (2 * k)) - 1 if k < 32 else U64_MAX)


def rc_keys(keys, k):
    keys = np.asarray(keys, dtype=np.uint64) & mask_of(k)
    out = np.zeros_like(keys)
    for i in range(k):
        out |= (((keys >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)) ^ np.uint64(1)) << np.uint64(2 * i)
    return out


def rank_keys(keys, k):
    """the number whose order is the keys' text order"""
    keys = np.asarray(keys, dtype=np.uint64)
    out = np.zeros_like(keys)
    for i in range(k):
        out |= ((keys >> np.uint64(2 * i)) & np.uint64(3)) << np.uint64(2 * (k - 1 - i))
    return out


def canonical_keys(keys, k):
    keys = np.asarray(keys, dtype=np.uint64) & mask_of(k)
    rc = rc_keys(keys, k)
    return np.where(rank_keys(keys, k) <= rank_keys(rc, k), keys, rc)


def ragged(src_off, counts):
    """indices src_off[i], src_off[i] + 1, ... (counts[i] of them) for every i, back to back -> (int64 index, int64 starts)"""
    counts = np.asarray(counts, dtype=np.int64)
    starts = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=starts[1:])
    idx = np.repeat(np.asarray(src_off, dtype=np.int64) - starts[:-1], counts)
    idx += np.arange(int(starts[-1]), dtype=np.int64)
    return idx, starts


def sum_by_key(keys, weights):
    """equal keys added up -> (keys ascending, uint64 sums)"""
    keys = np.asarray(keys, dtype=np.uint64)
    weights = np.asarray(weights, dtype=np.uint64)
    if not len(keys):
        return keys, weights
    order = np.argsort(keys, kind="stable")
    keys, weights = keys[order], weights[order]
    at = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return keys[at], np.add.reduceat(weights, at)


# ------------------------------------------------------------------ the pool

class Pool:
    """pairwise distinct byte strings (codes, or any bytes: the lines of a text), with their flat concatenation"""

    def __init__(self, entries, distinct=True):
        self.entries = [np.ascontiguousarray(e, dtype=np.uint8) for e in entries]
        if distinct:
            assert len({e.tobytes() for e in self.entries}) == len(self.entries), "pool entries are not pairwise distinct"
        self.len = np.array([len(e) for e in self.entries], dtype=np.int64)
        self.off = np.zeros(len(self.entries) + 1, dtype=np.int64)
        np.cumsum(self.len, out=self.off[1:])
        self.flat = np.concatenate(self.entries) if self.entries else np.zeros(0, dtype=np.uint8)
        self._keys = {}

    def __len__(self):
        return len(self.entries)

    def expand(self, choice):
        """the entries choice[0], choice[1], ... back to back -> (uint8 stream, uint64 starts[n + 1])"""
        choice = np.asarray(choice, dtype=np.int64)
        idx, starts = ragged(self.off[choice], self.len[choice])
        return self.flat[idx], starts.astype(np.uint64)

    def table(self, choice):
        """the same as a packed table -> (words, starts, n_bases)"""
        stream, starts = self.expand(choice)
        return pack_codes(stream), starts, int(starts[-1])

    def with_revcomp(self):
        """entries 0 .. n - 1 as they are and n .. 2n - 1 reverse-complemented (they may repeat earlier contents)"""
        return Pool(self.entries + [(e[::-1] ^ np.uint8(1)) for e in self.entries], distinct=False)

    def content_ids(self):
        """for every entry the smallest index of an entry of the same content"""
        seen, out = {}, np.empty(len(self.entries), dtype=np.int64)
        for i, e in enumerate(self.entries):
            out[i] = seen.setdefault(e.tobytes(), i)
        return out

    def keys(self, k):
        """the k-mer rows of every entry -> (keys uint64 flat, rows int64 per entry, entry int64 per row, pos int64 per row)"""
        if k not in self._keys:
            rows = np.maximum(self.len - k + 1, 0)
            n = len(self.flat)
            allk = np.zeros(max(n - k + 1, 0), dtype=np.uint64)
            for i in range(k):
                if len(allk):
                    allk |= self.flat[i:i + len(allk)].astype(np.uint64) << np.uint64(2 * i)
            idx, row_starts = ragged(self.off[:-1], rows)
            entry = np.repeat(np.arange(len(self.entries), dtype=np.int64), rows)
            out = (allk[idx], rows, entry, idx - self.off[entry], row_starts)
            for a in out:
                a.setflags(write=False)
            self._keys[k] = out
        return self._keys[k]

    def profile(self, k, canonical=False):
        """dense counts uint32[n, 4^k] and rows uint64[n] per entry"""
        keys, rows, entry, _, _ = self.keys(k)
        if canonical:
            keys = canonical_keys(keys, k)
        width = 4 ** k
        counts = np.bincount(entry * width + keys.astype(np.int64), minlength=len(self.entries) * width)
        return counts.reshape(len(self.entries), width).astype(np.uint32), rows.astype(np.uint64)

    def hits(self, k, set_keys, set_counts, lo=1, hi=U64_MAX, canonical=False):
        """per entry (rows, hits): its rows, and how many of them are keys of the set with lo <= count <= hi (a lower bound of
        0 counts as 1: a key the set does not hold is no hit)"""
        keys, rows, entry, _, _ = self.keys(k)
        if canonical:
            keys = canonical_keys(keys, k)
        set_keys, set_counts = np.asarray(set_keys, dtype=np.uint64), np.asarray(set_counts, dtype=np.uint64)
        lo = max(int(lo), 1)
        keep = (set_counts >= np.uint64(lo)) & (set_counts <= np.uint64(hi)) if lo <= hi else np.zeros(len(set_keys), dtype=bool)
        sel = np.sort(set_keys[keep])
        hit = np.zeros(len(keys), dtype=bool)
        if len(sel) and len(keys):
            hit = sel[np.minimum(np.searchsorted(sel, keys), len(sel) - 1)] == keys
        return rows.astype(np.uint64), np.bincount(entry[hit], minlength=len(self.entries)).astype(np.uint64)


def make_pool(seed, long=True):
    """-> (Pool, n_short, long ids): the empty sequence, the four of one base, the lengths around the 32-base word and the
    64-base read, random ones of 2 .. 40 bases up to POOL_SHORT short entries; then the long ones and, last, a copy of the
    longest with its last base changed"""
    rng = np.random.default_rng(seed)
    entries, seen = [], set()

    def add(e):
        e = np.asarray(e, dtype=np.uint8)
        if e.tobytes() in seen:
            return False
        seen.add(e.tobytes())
        entries.append(e)
        return True

    add(np.zeros(0, dtype=np.uint8))
    for c in range(4):
        add([c])
    for n in EDGE_LENGTHS:
        add(rng.integers(0, 4, n, dtype=np.uint8))
    while len(entries) < POOL_SHORT:
        add(rng.integers(0, 4, int(rng.integers(2, 41)), dtype=np.uint8))
    n_short, long_ids = len(entries), []
    if long:
        for n in LONG_LENGTHS:
            assert add(rng.integers(0, 4, n, dtype=np.uint8))
            long_ids.append(len(entries) - 1)
        twin = entries[-1].copy()
        twin[-1] ^= np.uint8(2)
        assert add(twin)
        long_ids.append(len(entries) - 1)
    return Pool(entries), n_short, long_ids


# ------------------------------------------------------------------ the table

class ScaleTable:
    def __init__(self, seed, n_seqs, long=True):
        self.pool, self.n_short, self.long_ids = make_pool(seed, long)
        rng = np.random.default_rng(seed + 1)
        n = self.n = int(n_seqs)
        # where the scan carries: at full size the real place, in a small table (the CPU tests of this model) its middle
        self.carry = CARRY if n > CARRY + SCAN_TILE else n // 2
        zone = min(SCAN_TILE, self.carry // 2)
        assert n >= 64 and self.carry + zone + 1 + 4 * len(self.long_ids) < n - 1
        self.hot = 5 + len(EDGE_LENGTHS) + 7                       # a random entry of 2 .. 40 bases
        p = rng.integers(0, self.n_short, n, dtype=np.int64)       # uniform, the empty sequence among them
        p[rng.random(n) < 0.01] = self.hot                         # and one entry about 1% of the table
        nonempty = lambda: int(rng.integers(1, self.n_short))      # noqa: E731
        # every long entry three times: below the first scan block's end, just below the carry, and past the block behind it
        zones = [(1, zone), (self.carry - zone, self.carry), (self.carry + zone + 1, n - 1)]
        self.placed = {}
        for lo, hi in zones:
            at = lo + rng.permutation(hi - lo)[:len(self.long_ids)]
            for e, i in zip(self.long_ids, at):
                p[i] = e
                self.placed.setdefault(e, []).append(int(i))
        for i in (0, self.carry, n - 1):
            if p[i] == 0 or p[i] >= self.n_short:
                p[i] = nonempty()
        p.setflags(write=False)
        self.p = p
        self.words, self.starts, self.n_bases = self.pool.table(p)
        self.words.setflags(write=False)
        self.starts.setflags(write=False)

    # ---- classes of equal sequences
    def classes(self, ids=None):
        """(rep, copies, distinct) of the table whose sequence i holds the content ids[i] (default: this table's p)"""
        ids = self.p if ids is None else np.asarray(ids, dtype=np.int64)
        n, width = len(ids), int(ids.max()) + 1 if len(ids) else 0
        first = np.full(width, n, dtype=np.int64)
        first[ids[::-1]] = np.arange(n - 1, -1, -1, dtype=np.int64)             # the last write wins: the smallest index
        mult = np.bincount(ids, minlength=width)
        return first[ids].astype(np.uint64), mult[ids].astype(np.uint64), int(np.count_nonzero(mult))

    def multiplicity(self):
        return np.bincount(self.p, minlength=len(self.pool)).astype(np.int64)

    def first_index(self):
        """the first sequence of every pool entry (n for one the table does not hold)"""
        first = np.full(len(self.pool), self.n, dtype=np.int64)
        first[self.p[::-1]] = np.arange(self.n - 1, -1, -1, dtype=np.int64)
        return first

    # ---- k-mers
    def groups(self, k):
        """GROUP BY kmer, count(*) over the table -> (keys ascending, counts uint64)"""
        keys, rows, _, _, _ = self.pool.keys(k)
        weights = np.repeat(self.multiplicity(), rows)
        if k <= 6:
            counts = np.bincount(keys.astype(np.int64), weights=weights.astype(np.float64), minlength=4 ** k)   # exact below 2^53
            at = np.flatnonzero(counts)
            return at.astype(np.uint64), counts[at].astype(np.uint64)
        ks, cs = sum_by_key(keys, weights)
        return ks[cs != 0], cs[cs != 0]

    def row_list(self, k):
        """the table's rows in table order -> (keys, seq, pos in the sequence, stream row), uint64 each"""
        keys, rows, _, _, row_starts = self.pool.keys(k)
        idx, _ = ragged(row_starts[:-1][self.p], rows[self.p])
        seq = np.repeat(np.arange(self.n, dtype=np.int64), rows[self.p])
        pos = idx - row_starts[:-1][self.p][seq]
        return keys[idx], seq.astype(np.uint64), pos.astype(np.uint64), self.starts[seq] + pos.astype(np.uint64)

    # ---- text
    def text_ids(self):
        """the sequences a text file can hold with plain readers: neither empty nor long (a long line is fine, but the text
        of the long ones would only add bytes)"""
        return np.flatnonzero((self.p != 0) & (self.p < self.n_short))


def lines_pool(pool, n_short):
    """one line of text per short pool entry"""
    return Pool([np.concatenate([LETTERS[e], np.frombuffer(b"\n", dtype=np.uint8)]) for e in pool.entries[:n_short]])


def n_position(e, length):
    """where the N of entry e's ambiguous variant stands"""
    return (7 * e + 3) % length


def fastq_pool(pool, n_short):
    """-> Pool of 2 * n_short FASTQ records: entry e's read as it is, and at n_short + e with one N in it.  Entry 0 (the empty
    sequence) has no valid record: do not choose it."""
    plain, amb = [], []
    for e, codes in enumerate(pool.entries[:n_short]):
        s = LETTERS[codes].tobytes()
        plain.append(b"@r\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
        if len(s):
            at = n_position(e, len(s))
            s = s[:at] + b"N" + s[at + 1:]
        amb.append(b"@r\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    return Pool([np.frombuffer(r, dtype=np.uint8) for r in plain + amb], distinct=False)


def expand_pieces(pieces, offsets, choice):
    """pieces[e]: the sequences (uint8 code arrays) record e turns into, offsets[e]: where in the record's sequence text each
    began; the records choice[0], choice[1], ... -> (words, starts, n_bases, src_record, src_offset) of the resulting table"""
    choice = np.asarray(choice, dtype=np.int64)
    flat_pool = Pool([x for ps in pieces for x in ps], distinct=False)
    per = np.array([len(ps) for ps in pieces], dtype=np.int64)
    first_piece = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum(per, out=first_piece[1:])
    which, _ = ragged(first_piece[:-1][choice], per[choice])
    words, starts, n_bases = flat_pool.table(which)
    src_record = np.repeat(np.arange(len(choice), dtype=np.uint64), per[choice])
    flat_off = np.array([o for os_ in offsets for o in os_], dtype=np.uint64)
    return words, starts, n_bases, src_record, flat_off[which] if len(flat_off) else flat_off


_TABLES = {}


def scale_table(seed, n_seqs, long=True):
    """the table, built once per argument list and never modified"""
    key = (seed, n_seqs, long)
    if key not in _TABLES:
        _TABLES[key] = ScaleTable(seed, n_seqs, long)
    return _TABLES[key]
