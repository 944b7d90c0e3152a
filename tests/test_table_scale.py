"""The table features on a table of more than 2^21 sequences: past the third level of the shared u32 scan (launch_scan_u32's
scan_sums_kernel carries a running total from one sweep of 1024 block sums to the next only above 1024 x 2048 entries), past
every per-sequence grid, binary search and u32 offset array of sequence 2^21; and the k-mer index past 2^24 keys, where its
sort's scan of 256 x tiles words takes the same carry.

The judge is tests/table_scale_model.py: a table whose sequences are whole copies of the entries of a small pool, so that
every answer is a per-pool-entry answer looked up through p.  The CPU tests here show that model right at 5,000 sequences
against independent per-sequence answers (the oracle, Counter over the texts, the references of test_table_profile.py,
test_table_hits.py, reads_model.py and text_model.py) and assert the structure the GPU tests rely on at full size.  The GPU
tests compare the device with the model at N = 2^21 + 4096 + 5, row for row; every comparison is integer equality, and each
test asserts the size that makes it meaningful."""
import collections

import numpy as np
import pytest

import oracle as orc
import reads_model
import table_scale_model as tsm
import text_model
from __graft_entry__ import load_package
from table_scale_model import CARRY, N_FULL, SCAN_TILE
from test_kmer_index import r_of
from test_table_hits import canonical_np, ref_hits, revcomp_text
from test_table_profile import ref_profile

SEED = 0x5CA1E
SMALL = 5000
U64_MAX = 2 ** 64 - 1
SENTINEL = 0xC3C3C3C3C3C3C3C3
SENTINEL32 = 0xC3C3C3C3
HITS_K = 11
INDEX_K = 12
INDEX_CARRY = 1 << 24                 # keys above which the index sort's 256 x tiles histogram words pass 2^21


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def same(got, want, what):
    """exact equality of two integer arrays, with the first difference and its side of the carry in the message"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if not np.array_equal(got, want):
        at = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        i = int(at[0])
        raise AssertionError(f"{what}: {len(at)} of {len(got)} entries differ, the first at {i} ({i - CARRY:+d} from 2^21): "
                             f"{got[i]} instead of {want[i]}")


def hits_set(pool, n_short, k):
    """the counted set of the hits tests: the first quarter of the pool counted twice, the second quarter once
    -> (keys ascending, counts)"""
    keys, rows, entry, _, _ = pool.keys(k)
    weight = np.where(entry < n_short // 4, 2, np.where(entry < n_short // 2, 1, 0))
    ks, cs = tsm.sum_by_key(keys, weight)
    return ks[cs != 0], cs[cs != 0]


def absent_contents(pool, n, seed):
    """n code arrays no pool entry equals: pool entries with the last base changed (checked), and the longest one with a base
    changed in its middle"""
    rng = np.random.default_rng(seed)
    have = {e.tobytes() for e in pool.entries}
    out = []
    while len(out) < n - 1:
        e = pool.entries[int(rng.integers(5, len(pool.entries)))].copy()
        e[-1] ^= np.uint8(1 + int(rng.integers(0, 3)))
        if e.tobytes() not in have:
            have.add(e.tobytes())
            out.append(e)
    mid = max(pool.entries, key=len).copy()
    mid[len(mid) // 2] ^= np.uint8(1)
    assert mid.tobytes() not in have
    return out + [mid]


def fastq_answers(fq_pool, ambiguous):
    """reads_model's answer for every record of the FASTQ pool on its own -> (pieces as code arrays, offsets, dropped flag)"""
    code_of = np.zeros(256, dtype=np.uint8)
    code_of[list(b"ATCG")] = [0, 1, 2, 3]
    pieces, offsets, dropped = [], [], []
    opt = reads_model.Options(format=reads_model.FASTQ, ambiguous=ambiguous)
    for e in fq_pool.entries:
        if len(e) == len(b"@r\n\n+\n\n"):                  # the empty sequence: no valid record, never chosen
            pieces.append([]), offsets.append([]), dropped.append(0)
            continue
        p = reads_model.parse(e.tobytes(), opt)
        assert p.error is None and p.records == 1
        pieces.append([code_of[np.frombuffer(s.encode(), dtype=np.uint8)] for s in p.sequences])
        offsets.append(list(p.src_offset))
        dropped.append(p.dropped)
    return pieces, offsets, np.array(dropped, dtype=np.int64)


def fastq_choice(t):
    """the FASTQ records of the text table: the reads of text_ids(), every seventh with one N"""
    ids = t.text_ids()
    amb = (np.arange(len(ids)) % 7 == 3)
    return ids, t.p[ids] + amb * t.n_short, amb


# ------------------------------------------------------------------ CPU: the model against per-sequence answers

@pytest.fixture(scope="module")
def small():
    t = tsm.scale_table(SEED, SMALL)
    texts = [tsm.text_of(t.pool.entries[e]) for e in t.p]
    return t, texts


def test_model_pool_and_draw():
    """the pool: pairwise distinct, about 4096 short entries with the listed lengths, the long ones and the one-base twin;
    the draw at 5,000: a hot entry, every long entry three times and around the middle"""
    t = tsm.scale_table(SEED, SMALL)
    texts = [tsm.text_of(e) for e in t.pool.entries]
    assert len(set(texts)) == len(texts) == tsm.POOL_SHORT + 4 and t.n_short == tsm.POOL_SHORT
    assert texts[0] == "" and sorted(texts[1:5]) == ["A", "C", "G", "T"]
    assert [len(x) for x in texts[5:11]] == [31, 32, 33, 63, 64, 65]
    assert all(2 <= len(x) <= 40 for x in texts[11:t.n_short])
    assert [len(texts[e]) for e in t.long_ids] == [2_100, 66_000, 70_000, 70_000]
    a, b = texts[t.long_ids[2]], texts[t.long_ids[3]]
    assert a[:-1] == b[:-1] and a[-1] != b[-1]
    for e in t.long_ids:
        lo, mid, hi = t.placed[e]
        assert lo < t.carry // 2 <= mid < t.carry < hi and list(np.flatnonzero(t.p == e)) == [lo, mid, hi]
    assert 0.005 < np.mean(t.p == t.hot) < 0.02


def test_model_stream_and_starts(small):
    t, texts = small
    words, n = orc.dna_encode("".join(texts))
    assert n == t.n_bases and np.array_equal(words, t.words)
    assert np.array_equal(t.starts, np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.uint64))
    assert np.array_equal(tsm.unpack_words(t.words, n), np.concatenate([t.pool.entries[e] for e in t.p]))


def test_model_classes(small):
    t, texts = small
    count = collections.Counter(texts)
    first = {}
    for i, x in enumerate(texts):
        first.setdefault(x, i)
    rep, copies, distinct = t.classes()
    assert rep.tolist() == [first[x] for x in texts] and copies.tolist() == [count[x] for x in texts]
    assert distinct == len(count)
    assert np.array_equal(t.first_index()[t.p], rep.astype(np.int64)) and np.array_equal(t.multiplicity()[t.p], copies.astype(np.int64))


@pytest.mark.parametrize("k", [1, 5, 6, 7, 21, 31, 32])
def test_model_rows_and_groups(small, k):
    """the row list against generate_kmers of every sequence on its own, the groups against count_kmers of the rows"""
    t, texts = small
    keys, seq, pos, stream_row = t.row_list(k)
    want_keys, want_seq, want_pos = [], [], []
    for i, x in enumerate(texts):
        if len(x) >= k:
            own = orc.generate_kmers(*orc.dna_encode(x), k, faithful=False)
            want_keys.append(own)
            want_seq.append(np.full(len(own), i, dtype=np.uint64))
            want_pos.append(np.arange(len(own), dtype=np.uint64))
    assert np.array_equal(keys, np.concatenate(want_keys)) and np.array_equal(seq, np.concatenate(want_seq))
    assert np.array_equal(pos, np.concatenate(want_pos)) and np.array_equal(stream_row, t.starts[seq.astype(np.int64)] + pos)
    assert np.array_equal(keys, orc.generate_kmers_table(t.words, t.starts, k))
    gk, gc = t.groups(k)
    ok, oc = orc.count_keys(keys)
    assert np.array_equal(gk, ok) and np.array_equal(gc, oc)


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", [1, 2])
def test_model_profiles(small, k, canonical):
    t, texts = small
    counts, rows = t.pool.profile(k, canonical)
    want_counts, want_rows = ref_profile(texts, k, canonical)
    assert np.array_equal(counts[t.p], want_counts) and np.array_equal(rows[t.p], want_rows)


def test_model_hits(small):
    t, texts = small
    sk, sc = hits_set(t.pool, t.n_short, HITS_K)
    quarter = [tsm.text_of(e) for e in t.pool.entries[:t.n_short // 2]]
    want = collections.Counter()
    for i, x in enumerate(quarter):
        if len(x) >= HITS_K:
            for key in orc.generate_kmers(*orc.dna_encode(x), HITS_K, faithful=False).tolist():
                want[key] += 2 if i < t.n_short // 4 else 1
    assert dict(zip(sk.tolist(), sc.tolist())) == dict(want) and set(sc.tolist()) >= {1, 2}
    assert np.array_equal(tsm.canonical_keys(sk, HITS_K), canonical_np(sk, HITS_K))
    for canonical in (False, True):
        for lo, hi in ((1, U64_MAX), (2, 2)):
            rows, hits = t.pool.hits(HITS_K, sk, sc, lo, hi, canonical)
            want_rows, want_hits = ref_hits(texts, HITS_K, sk, sc, lo, hi, canonical)
            assert np.array_equal(rows[t.p], want_rows) and np.array_equal(hits[t.p], want_hits)
            assert 0 < int(want_hits.sum()) < int(want_rows.sum())


def test_model_take(small):
    """the pool with its reverse complements: a take with flips, and the classes by content"""
    t, texts = small
    rng = np.random.default_rng(SEED + 2)
    ids = rng.integers(0, t.n, 3000)
    flip = rng.random(3000) < 0.2
    ids[:4], flip[:4] = [t.placed[e][1] for e in t.long_ids], [True, False, True, True]
    both = t.pool.with_revcomp()
    choice = t.p[ids] + flip * len(t.pool)
    words, starts, n = both.table(choice)
    taken = [revcomp_text(texts[i]) if f else texts[i] for i, f in zip(ids, flip)]
    w, m = orc.dna_encode("".join(taken))
    assert m == n and np.array_equal(w, words)
    assert starts.tolist() == [0] + np.cumsum([len(x) for x in taken]).tolist()
    rep, copies, distinct = t.classes(both.content_ids()[choice])
    count, first = collections.Counter(taken), {}
    for i, x in enumerate(taken):
        first.setdefault(x, i)
    assert rep.tolist() == [first[x] for x in taken] and copies.tolist() == [count[x] for x in taken]
    assert distinct == len(count)


def test_model_text(small):
    """the LINES and FASTQ texts of the model against the two text models on the whole text"""
    t, texts = small
    ids, choice, amb = fastq_choice(t)
    assert all(0 < len(texts[i]) <= 65 for i in ids) and len(ids) > SMALL - 100
    data, line_starts = tsm.lines_pool(t.pool, t.n_short).expand(t.p[ids])
    parsed = text_model.parse(data.tobytes(), text_model.LINES)
    assert parsed.error is None and parsed.records == [texts[i] for i in ids] and parsed.pos == line_starts[:-1].tolist()
    fq = tsm.fastq_pool(t.pool, t.n_short)
    data, rec_starts = fq.expand(choice)
    assert data.tobytes().count(b"N") == int(amb.sum()) > 0
    for mode in (reads_model.DROP, reads_model.SPLIT):
        whole = reads_model.parse(data.tobytes(), reads_model.Options(format=reads_model.FASTQ, ambiguous=mode))
        assert whole.error is None and whole.records == len(ids) and whole.pos == rec_starts[:-1].tolist()
        pieces, offsets, dropped = fastq_answers(fq, mode)
        words, starts, n, src_record, src_offset = tsm.expand_pieces(pieces, offsets, choice)
        w, m = orc.dna_encode("".join(whole.sequences))
        assert m == n and np.array_equal(w, words)
        assert starts.tolist() == [0] + np.cumsum([len(x) for x in whole.sequences]).tolist()
        assert src_record.tolist() == whole.src_record and src_offset.tolist() == whole.src_offset
        assert int(dropped[choice].sum()) == whole.dropped == (int(amb.sum()) if mode == reads_model.DROP else 0)
        assert whole.ambiguous == int(amb.sum())


def test_model_structure_at_full_size():
    """what the GPU tests rely on, at the size they run at"""
    t = tsm.scale_table(SEED, N_FULL)
    assert t.n == N_FULL == CARRY + 4096 + 5 > CARRY + SCAN_TILE and t.carry == CARRY
    assert t.n_bases < 2 ** 32 and int(t.starts[-1]) == t.n_bases and len(t.starts) == N_FULL + 1
    for e in t.long_ids:
        lo, mid, hi = t.placed[e]
        assert 0 < lo < SCAN_TILE and CARRY - SCAN_TILE <= mid < CARRY and CARRY + SCAN_TILE < hi < N_FULL - 1
        assert list(np.flatnonzero(t.p == e)) == [lo, mid, hi]
    for i in (0, CARRY, N_FULL - 1):
        assert 0 < t.p[i] < t.n_short
    first, mult = t.first_index(), t.multiplicity()
    assert (mult > 0).all() and (first[:t.n_short] < CARRY).all()
    last = np.zeros(len(t.pool), dtype=np.int64)
    last[t.p] = np.arange(N_FULL)
    assert int(np.sum((first < CARRY) & (last > CARRY))) > 1000          # classes with members either side of 2^21
    assert 0.005 < mult[t.hot] / N_FULL < 0.02 and int(np.sum(mult == mult[t.hot])) == 1
    assert len(t.text_ids()) > CARRY + SCAN_TILE                         # the text table keeps more records than the carry
    assert int(np.sum(t.p == 0)) > 100                                   # empty sequences either side
    rows21 = np.maximum(t.pool.len - 21 + 1, 0)[t.p]
    assert int(rows21.sum()) > CARRY and int(rows21[CARRY + SCAN_TILE:].sum()) > 0


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(ctx):
    """the scale table, uploaded once and only ever read -> (model, resident Dna)"""
    t = tsm.scale_table(SEED, N_FULL)
    d = ctx.upload(t.words, t.n_bases)
    d.set_sequences(t.starts)
    yield t, d
    d.free()


@pytest.fixture(scope="module")
def classes(ctx, table):
    t, d = table
    c = ctx.table_classes(d)
    yield c
    c.free()


def resident(ctx, pool, choice):
    words, starts, n = pool.table(choice)
    d = ctx.upload(words if len(words) else np.zeros(1, dtype=np.uint64), n)
    d.set_sequences(starts)
    return d, words, starts


@pytest.mark.gpu
def test_scale_starts(ctx, table):
    """1. the resident starts, whole and in windows that straddle 2^21"""
    t, d = table
    assert d.n_sequences == N_FULL > CARRY + SCAN_TILE and d.n_bases == t.n_bases
    same(d.sequence_starts(), t.starts, "sequence_starts")
    for first, count in ((CARRY - 3, 7), (CARRY, 1), (CARRY - SCAN_TILE - 1, 2 * SCAN_TILE + 3), (N_FULL - 2, 3), (N_FULL, 1)):
        same(d.sequence_starts(first, count), t.starts[first:first + count], f"sequence_starts({first}, {count})")
    same(d.download(), t.words, "the stream")


@pytest.mark.gpu
def test_scale_classes(ctx, table, classes):
    """2. representatives, copies and distinct of all N sequences in one strong-fingerprint round; select with and without a
    cap; members of a class that straddles 2^21, asked through a member that is not its representative, and of the long
    classes; the 70,000-base entry and its one-base twin are two classes"""
    t, d = table
    assert classes.sequences == N_FULL > CARRY + SCAN_TILE
    rep, copies, distinct = t.classes()
    got_rep, got_copies = classes.read()
    same(got_rep, rep, "rep")
    same(got_copies, copies, "copies")
    assert classes.distinct == distinct == len(t.pool) and classes.rounds == 1
    first, mult = t.first_index(), t.multiplicity()
    hot = int(mult[t.hot])
    for lo, hi in ((1, U64_MAX), (2, U64_MAX), (hot, hot), (3, 3), (4, hot - 1)):
        keep = np.flatnonzero((mult >= lo) & (mult <= hi))
        order = np.argsort(first[keep])
        seq, cop, n = classes.select(lo, hi)
        assert n == len(keep), (lo, hi)
        same(seq, first[keep][order].astype(np.uint64), f"select({lo}, {hi}): seq")
        same(cop, mult[keep][order].astype(np.uint64), f"select({lo}, {hi}): copies")
    keep = np.argsort(first)
    seq, cop, n = classes.select(1, U64_MAX, cap=1000)
    assert n == len(t.pool) > 1000 and len(seq) == 1000
    same(seq, first[keep][:1000].astype(np.uint64), "select with a cap: seq")
    same(cop, mult[keep][:1000].astype(np.uint64), "select with a cap: copies")
    assert classes.select(3, 3)[2] == 4 and classes.select(hot, hot)[0].tolist() == [first[t.hot]]
    # members: a class either side of 2^21 through its last member, the hot class through a middle one, the long classes
    last_of_first_class = int(np.flatnonzero(t.p == t.p[0])[-1])
    hot_members = np.flatnonzero(t.p == t.hot)
    assert last_of_first_class > CARRY and int(hot_members[-1]) > CARRY + SCAN_TILE
    for s in (0, last_of_first_class, int(hot_members[len(hot_members) // 2]), CARRY, N_FULL - 1):
        ids, n = classes.members(s)
        want = np.flatnonzero(t.p == t.p[s])
        assert n == len(want)
        same(ids, want.astype(np.uint64), f"members({s})")
    for e in t.long_ids:
        for s in t.placed[e]:
            ids, n = classes.members(s)
            assert n == 3 and ids.tolist() == t.placed[e], f"members({s}) of long entry {e}"
    a, b = t.long_ids[2], t.long_ids[3]
    assert got_rep[t.placed[a][2]] == t.placed[a][0] != t.placed[b][0] == got_rep[t.placed[b][2]]
    ids, n = classes.members(int(hot_members[-1]), cap=10)
    assert n == hot and ids.tolist() == hot_members[:10].tolist()


@pytest.mark.gpu
def test_scale_match_of_the_pool(ctx, table, classes):
    """3a. the pool and 200 contents the table does not hold, probed against the classes of the scale table"""
    t, d = table
    assert classes.sequences > CARRY + SCAN_TILE
    absent = absent_contents(t.pool, 200, SEED + 3)
    probe_pool = tsm.Pool(t.pool.entries + absent)
    order = np.random.default_rng(SEED + 4).permutation(len(probe_pool))
    probe, _, _ = resident(ctx, probe_pool, order)
    try:
        first, mult = t.first_index(), t.multiplicity()
        held = order < len(t.pool)
        want_match = np.where(held, first[np.minimum(order, len(t.pool) - 1)], -1).astype(np.int64).astype(np.uint64)
        want_copies = np.where(held, mult[np.minimum(order, len(t.pool) - 1)], 0).astype(np.uint64)
        assert int((want_match == U64_MAX).sum()) == 200 and int(want_copies.max()) == int(mult[t.hot])
        match, copies, n = classes.match(probe)
        same(match, want_match, "match")
        same(copies, want_copies, "copies")
        assert n == len(t.pool)
    finally:
        probe.free()


@pytest.mark.gpu
def test_scale_match_of_the_table(ctx, table):
    """3b. the scale table as the probe (N probes, long ones past 2^21) against the classes of a small table of pool entries:
    a shuffled part of the pool with repeats, every sixteenth entry left out; a window that straddles 2^21 into device memory
    leaves the cells either side alone"""
    t, d = table
    rng = np.random.default_rng(SEED + 5)
    kept = np.flatnonzero(np.arange(len(t.pool)) % 16 != 9)
    assert all(e in kept for e in t.long_ids[:3])
    choice = rng.permutation(np.concatenate([kept, rng.choice(kept, 300)]))
    built, _, _ = resident(ctx, t.pool, choice)
    try:
        with ctx.table_classes(built) as c:
            n_built = len(choice)
            first = np.full(len(t.pool), -1, dtype=np.int64)
            first[choice[::-1]] = np.arange(n_built - 1, -1, -1)
            mult = np.bincount(choice, minlength=len(t.pool))
            want_match, want_copies = first[t.p].astype(np.uint64), mult[t.p].astype(np.uint64)
            assert 0 < int((want_match == U64_MAX).sum()) < N_FULL // 8
            assert d.n_sequences == N_FULL > CARRY + SCAN_TILE
            match, copies, n = c.match(d)
            same(match, want_match, "match")
            same(copies, want_copies, "copies")
            assert n == int((want_match != U64_MAX).sum())
            lo, count, pad = CARRY - 1000, 3000, 64
            bufs = [ctx.buffer_alloc(8 * (count + 2 * pad)) for _ in range(2)]
            try:
                for b in bufs:
                    ctx.upload_u64(b, np.full(count + 2 * pad, SENTINEL, dtype=np.uint64))
                n = c.match(d, lo, count, on_device=True, out=(bufs[0] + 8 * pad, bufs[1] + 8 * pad))
                got = [ctx.download_u64(b, count + 2 * pad) for b in bufs]
            finally:
                for b in bufs:
                    ctx.buffer_free(b)
            for a in got:
                assert (a[:pad] == SENTINEL).all() and (a[pad + count:] == SENTINEL).all()
            same(got[0][pad:pad + count], want_match[lo:lo + count], "window: match")
            same(got[1][pad:pad + count], want_copies[lo:lo + count], "window: copies")
            assert n == int((want_match[lo:lo + count] != U64_MAX).sum())
    finally:
        built.free()


@pytest.mark.gpu
def test_scale_take(ctx, table):
    """4. dna_take of N ids with repeats in random order, one in five reverse-complemented, the long ones among them: starts
    and stream of the result; and its classes, by the contents of the pool and of its reverse complements"""
    t, d = table
    rng = np.random.default_rng(SEED + 6)
    ids = rng.integers(0, N_FULL, N_FULL)
    flip = rng.random(N_FULL) < 0.2
    at = CARRY + SCAN_TILE + 100 + np.arange(4)
    ids[at], flip[at] = [t.placed[e][2] for e in t.long_ids], [True, False, True, True]
    ids[[5, 6]], flip[[5, 6]] = [t.placed[t.long_ids[2]][1], t.placed[t.long_ids[3]][0]], [False, False]
    assert len(ids) > CARRY + SCAN_TILE
    both = t.pool.with_revcomp()
    choice = t.p[ids] + flip * len(t.pool)
    words, starts, n = both.table(choice)
    assert n < 2 ** 32
    taken = ctx.dna_take(d, ids.astype(np.uint64), flip)
    try:
        assert taken.n_sequences == N_FULL and taken.n_bases == n
        same(taken.sequence_starts(), starts, "starts of the taken table")
        same(taken.download(), words, "stream of the taken table")
        rep, copies, distinct = t.classes(both.content_ids()[choice])
        with ctx.table_classes(taken) as c:
            got_rep, got_copies = c.read()
            same(got_rep, rep, "rep of the taken table")
            same(got_copies, copies, "copies of the taken table")
            assert c.distinct == distinct and c.rounds == 1
    finally:
        taken.free()


GATHER_SEGS = [1, 2047, 2048, 2049, CARRY - 1, CARRY, CARRY + 1, CARRY + SCAN_TILE + 5, 3 * CARRY + 7]
GATHER_PATTERNS = ["zeros", "ones", "last", "block heads", "at 2^21", "random"]


def gather_lengths(pattern, n, rng):
    z = np.zeros(n, dtype=np.uint64)
    if pattern == "ones":
        z[:] = 1
    elif pattern == "last":
        z[-1] = 5
    elif pattern == "block heads":
        z[::SCAN_TILE] = 3
    elif pattern == "at 2^21":
        if n <= CARRY:
            return None                                                  # there is no such segment
        z[CARRY] = 7
    elif pattern == "random":
        z = rng.integers(0, 9, n).astype(np.uint64)
    return z


@pytest.mark.gpu
@pytest.mark.parametrize("n_segs", GATHER_SEGS)
def test_scale_scan_through_gather(ctx, n_segs):
    """5. dna_gather takes the caller's segment lengths and its result's starts are their exclusive scan plus the total: the
    shared scan on chosen values, at one, two, three and four sweeps of the block sums"""
    assert n_segs in (1, 2047, 2048, 2049, 2097151, 2097152, 2097153, 2099205, 6291463)
    rng = np.random.default_rng(SEED + 7 + n_segs)
    codes = rng.integers(0, 4, 64, dtype=np.uint8)
    src = ctx.upload(tsm.pack_codes(codes), 64)
    try:
        for pattern in GATHER_PATTERNS:
            length = gather_lengths(pattern, n_segs, rng)
            if length is None:
                continue
            first = (rng.integers(0, 1 << 30, n_segs).astype(np.uint64) % (np.uint64(65) - length)).astype(np.uint64)
            want = np.zeros(n_segs + 1, dtype=np.uint64)
            np.cumsum(length, out=want[1:])
            g = ctx.dna_gather(src, first, length)
            try:
                assert g.n_sequences == n_segs and g.n_bases == int(want[-1]) <= 8 * n_segs
                same(g.sequence_starts(), want, f"{pattern}: starts of {n_segs} segments")
                if pattern in ("random", "block heads"):
                    idx, _ = tsm.ragged(first.astype(np.int64), length.astype(np.int64))
                    same(g.download(), tsm.pack_codes(codes[idx]), f"{pattern}: stream of {n_segs} segments")
            finally:
                g.free()
    finally:
        src.free()


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("k", [1, 2])
def test_scale_profile(ctx, table, k, canonical):
    """6. the profiles of all N sequences, the long ones past 2^21 among them (profile_tile_kernel's item search at its far
    end); once more into device memory between sentinel cells"""
    t, d = table
    assert d.n_sequences == N_FULL > CARRY + SCAN_TILE and max(t.placed[t.long_ids[2]]) > CARRY + SCAN_TILE
    counts, rows = t.pool.profile(k, canonical)
    got_counts, got_rows = ctx.table_profile(d, k, canonical=canonical)
    same(got_rows, rows[t.p], "rows")
    same(got_counts, counts[t.p], "counts")
    if k == 1:
        width, pad, first = 4 ** k, 64, 1
        n = N_FULL - 2
        cells = n * width
        buf, rbuf = ctx.buffer_alloc(4 * (cells + 2 * pad)), ctx.buffer_alloc(8 * n)
        try:
            ctx.upload_bytes(buf, np.full(cells + 2 * pad, SENTINEL32, dtype=np.uint32).view(np.uint8))
            ctx.table_profile(d, k, canonical=canonical, seq_first=first, seq_count=n, out_counts_dev=buf + 4 * pad, out_rows_dev=rbuf)
            got = ctx.download_bytes(buf, 4 * (cells + 2 * pad)).view(np.uint32)
            got_rows = ctx.download_u64(rbuf, n)
        finally:
            ctx.buffer_free(buf)
            ctx.buffer_free(rbuf)
        assert (got[:pad] == SENTINEL32).all() and (got[pad + cells:] == SENTINEL32).all()
        same(got[pad:pad + cells].reshape(n, width), counts[t.p[first:first + n]], "device counts")
        same(got_rows, rows[t.p[first:first + n]], "device rows")


@pytest.mark.gpu
def test_scale_hits(ctx, table):
    """7. an accumulator at k = 11 over half of the pool (one quarter added twice), probed with all N sequences: rows and hits
    of every sequence, the totals, the select, and a window across 2^21; plain and canonical, any count and count 2 only"""
    t, d = table
    assert d.n_sequences == N_FULL > CARRY + SCAN_TILE
    k, q = HITS_K, t.n_short // 4
    sk, sc = hits_set(t.pool, t.n_short, k)
    acc = ctx.accumulator(k)
    try:
        for lo, hi, times in ((0, q, 2), (q, 2 * q, 1)):
            part, _, _ = resident(ctx, t.pool, np.arange(lo, hi))
            h = ctx.count_kmers_table(part, k)
            for _ in range(times):
                acc.add(h)
            h.free()
            part.free()
        ak, ac = acc.download()
        order = np.argsort(ak)
        assert np.array_equal(ak[order], sk) and np.array_equal(ac[order], sc)
        for canonical in (False, True):
            for lo, hi in ((1, U64_MAX), (2, 2)):
                what = f"canonical={canonical} counts {lo}..{hi}"
                rows, hits = t.pool.hits(k, sk, sc, lo, hi, canonical)
                rows, hits = rows[t.p], hits[t.p]
                assert 0 < int(hits.sum()) < int(rows.sum()) and int(hits[CARRY + SCAN_TILE:].sum()) > 0
                with ctx.table_hits(d, acc, canonical=canonical, min_count=lo, max_count=hi) as sh:
                    assert (sh.sequences, sh.first, sh.k) == (N_FULL, 0, k)
                    got_rows, got_hits = sh.read()
                    same(got_rows, rows, f"{what}: rows")
                    same(got_hits, hits, f"{what}: hits")
                    assert sh.totals() == (int(rows.sum()), int(hits.sum()), int((hits > 0).sum())), what
                    seq, srows, shits, n = sh.select(min_hits=1)
                    want = np.flatnonzero(hits > 0)
                    assert n == len(want) and int(want[-1]) > CARRY + SCAN_TILE
                    same(seq, want.astype(np.uint64), f"{what}: select seq")
                    same(srows, rows[want], f"{what}: select rows")
                    same(shits, hits[want], f"{what}: select hits")
                first, count = CARRY - 1000, 3000
                with ctx.table_hits(d, acc, canonical=canonical, min_count=lo, max_count=hi, seq_first=first, seq_count=count) as sh:
                    assert (sh.sequences, sh.first) == (count, first)
                    got_rows, got_hits = sh.read()
                    same(got_rows, rows[first:first + count], f"{what}: window rows")
                    same(got_hits, hits[first:first + count], f"{what}: window hits")
                    w = hits[first:first + count]
                    assert sh.totals() == (int(rows[first:first + count].sum()), int(w.sum()), int((w > 0).sum()))
    finally:
        acc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 21, 31])
def test_scale_count_kmers_table(ctx, table, k):
    """8a. GROUP BY kmer over the table against the pool's keys weighted by multiplicity"""
    t, d = table
    assert d.n_sequences == N_FULL > CARRY + SCAN_TILE
    want_keys, want_counts = t.groups(k)
    h = ctx.count_kmers_table(d, k)
    try:
        keys, counts = h.download()
        order = np.argsort(keys, kind="stable")
        same(keys[order], want_keys, f"k = {k}: keys")
        same(counts[order], want_counts, f"k = {k}: counts")
        assert h.total == int(want_counts.sum())
    finally:
        h.free()


@pytest.mark.gpu
def test_scale_generate_kmers_table(ctx, table, pkg):
    """8b. the rows of the table at k = 21 with their sequence ids (they run past 2^21) and positions; a window of stream rows
    across the start of sequence 2^21; the fused ^@ filter on a 4-base prefix"""
    t, d = table
    k = 21
    keys, seq, pos, stream_row = t.row_list(k)
    assert d.n_sequences == N_FULL and int(seq[-1]) > CARRY + SCAN_TILE and len(keys) > CARRY
    got_keys, got_seq, got_pos, n = ctx.generate_kmers_table(d, k, cap=len(keys) + 16)
    assert n == len(keys)
    same(got_keys, keys, "keys")
    same(got_seq, seq, "sequence ids")
    same(got_pos, pos, "positions")
    first, count = int(t.starts[CARRY]) - 700, 1500
    inside = (stream_row >= first) & (stream_row < first + count)
    assert 0 < int(inside.sum()) < count and seq[inside].min() < CARRY <= seq[inside].max()
    got_keys, got_seq, got_pos, n = ctx.generate_kmers_table(d, k, first=first, count=count)
    assert n == int(inside.sum())
    same(got_keys, keys[inside], "window: keys")
    same(got_seq, seq[inside], "window: sequence ids")
    same(got_pos, pos[inside], "window: positions")
    prefix = int(keys[len(keys) // 2]) & 0xFF
    match = (keys & np.uint64(0xFF)) == np.uint64(prefix)
    assert 1000 < int(match.sum()) < len(keys) // 16 and int(seq[match][-1]) > CARRY + SCAN_TILE
    got_keys, got_seq, got_pos, n = ctx.generate_kmers_table(d, k, pkg.Filter.starts_with(4, prefix), cap=int(match.sum()) + 16)
    assert n == int(match.sum())
    same(got_keys, keys[match], "^@: keys")
    same(got_seq, seq[match], "^@: sequence ids")
    same(got_pos, pos[match], "^@: positions")


@pytest.mark.gpu
def test_scale_table_from_text(ctx, table, pkg):
    """9a. the scale table without its empty and long sequences as one line of text each: stream, starts and record offsets"""
    t, d = table
    ids = t.text_ids()
    assert len(ids) > CARRY + SCAN_TILE
    data, line_starts = tsm.lines_pool(t.pool, t.n_short).expand(t.p[ids])
    words, starts, n = t.pool.table(t.p[ids])
    got, report = ctx.table_from_text(data.tobytes(), pkg.TEXT_LINES, record_pos=len(ids) + 8)
    try:
        assert (report.records, report.bases, report.consumed) == (len(ids), n, len(data))
        assert got.n_sequences == len(ids) and got.n_bases == n
        same(got.sequence_starts(), starts, "starts")
        same(got.download(), words, "stream")
        same(report.record_pos, line_starts[:-1], "record offsets")
    finally:
        got.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["drop", "split", "drop, poisoned pool"])
def test_scale_reads_from_text(ctx, table, pkg, mode):
    """9b. the same reads as FASTQ, every seventh with one N at a position that varies: AMBIG_DROP (the kept-rank and
    kept-length scans see a 0 / 1 mix across the carry) and AMBIG_SPLIT (the pieces and their source map) against
    reads_model's answer per pool record, expanded; one run with poisoned, guarded pool buffers"""
    t, d = table
    ids, choice, amb = fastq_choice(t)
    assert len(ids) > CARRY + SCAN_TILE and int(amb[CARRY + SCAN_TILE:].sum()) > 0
    ambiguous = pkg.AMBIG_SPLIT if mode == "split" else pkg.AMBIG_DROP
    fq = tsm.fastq_pool(t.pool, t.n_short)
    data, rec_starts = fq.expand(choice)
    pieces, offsets, dropped = fastq_answers(fq, reads_model.SPLIT if mode == "split" else reads_model.DROP)
    words, starts, n, src_record, src_offset = tsm.expand_pieces(pieces, offsets, choice)
    n_seqs = len(starts) - 1
    # the scans run over the len(ids) records (drop: 0 / 1 flags and kept lengths) or over the pieces (split: more than records)
    assert (n_seqs > len(ids)) if mode == "split" else (CARRY * 6 // 7 < n_seqs < len(ids) and not amb[-1])
    ctx.set_debug(pkg.DEBUG_POISON_POOL | pkg.DEBUG_GUARD_POOL if "poisoned" in mode else 0)
    try:
        got, report = ctx.reads_from_text(data.tobytes(), pkg.TEXT_FASTQ, ambiguous=ambiguous, record_pos=len(ids) + 8,
                                          source=n_seqs + 8)
        try:
            assert (report.records, report.sequences, report.bases, report.consumed) == (len(ids), n_seqs, n, len(data))
            assert (report.ambiguous, report.dropped, report.short_out) == (int(amb.sum()), int(dropped[choice].sum()), 0)
            assert (report.dropped > 0) == (mode != "split") and (n_seqs > len(ids)) == (mode == "split")
            assert got.n_sequences == n_seqs and got.n_bases == n
            same(got.sequence_starts(), starts, "starts")
            same(got.download(), words, "stream")
            same(report.record_pos, rec_starts[:-1], "record offsets")
            same(report.src_record, src_record, "source record")
            same(report.src_offset, src_offset, "source offset")
        finally:
            got.free()
        assert pkg.lib().dnagpu_synchronize(ctx.h) == 0
    finally:
        ctx.set_debug(0)


@pytest.fixture(scope="module")
def index_column():
    """2^24 + 2048 + 3 keys of 24 bits with plentiful duplicates, and their index order (rows, keys), never modified"""
    n = INDEX_CARRY + SCAN_TILE + 3
    rng = np.random.default_rng(SEED + 8)
    col = (rng.integers(0, 1 << 20, n).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64((1 << 24) - 1)
    order = np.argsort(r_of(col, INDEX_K), kind="stable")
    col.setflags(write=False)
    order.setflags(write=False)
    return col, order


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [SCAN_TILE + 3, 0], ids=["past 2^24", "at 2^24"])
def test_scale_kmer_index(ctx, index_column, extra):
    """10. the index sort over 2^24 + 2048 + 3 keys at k = 12: three passes whose 256 x tiles histogram words pass 2^21, so the
    scan carries; and over exactly 2^24 keys, the last size that takes no carry.  The whole order, distinct, and lookups."""
    col, order = index_column
    n = INDEX_CARRY + extra
    assert n in (16_777_216, 16_779_267) and len(col) == INDEX_CARRY + SCAN_TILE + 3
    col, order = col[:n], order[order < n]                               # a stable order of a prefix: the same order, filtered
    want_keys = col[order]
    want_r = r_of(want_keys, INDEX_K)
    with ctx.kmer_index(col, INDEX_K) as idx:
        assert idx.rows == n and idx.k == INDEX_K
        rows, keys = idx.read()
        same(keys, want_keys, "keys in index order")
        same(rows, order.astype(np.uint64), "rows in index order")
        assert idx.distinct == int(np.count_nonzero(want_r[1:] != want_r[:-1])) + 1 < n // 8
        rng = np.random.default_rng(SEED + 9)
        present = col[rng.integers(0, n, 1000)]
        absent = np.setdiff1d(rng.integers(0, 1 << 24, 4000).astype(np.uint64), col)[:100]
        assert len(absent) == 100
        q = np.concatenate([present, absent, col[-1:], col[:1]])
        first, count = idx.lookup(q)
        lo = np.searchsorted(want_r, r_of(q, INDEX_K), side="left")
        hi = np.searchsorted(want_r, r_of(q, INDEX_K), side="right")
        same(count, (hi - lo).astype(np.uint64), "lookup: count")
        same(first[count > 0], lo[hi > lo].astype(np.uint64), "lookup: first")
        assert (count[:1000] > 0).all() and (count[1000:1100] == 0).all()
