"""The k-mer accumulator restated in numpy, for tests that place keys by their hash (no GPU, no package import).

splitmix64 is a bijection on 64 bits, so at k = 32 -- where every 64-bit value is a key -- a test can write the hash it wants
(partition prefix, the bits under it, the home slot) and invert it: place().  Model restates the host rules of an add from
DESIGN.md 4.9 and the constants (4096 slots, the 7/8 bound, the 3/4 mean load, bins of mean + 8 sigma): which rounds an add
takes -- "rebin", "dry", "grow", "commit" -- and how many partitions the table has afterwards.
"""
import numpy as np

U64 = np.uint64
ACC_SLOTS = 4096                                  # slots of a partition
ACC_BOUND = ACC_SLOTS // 8 * 7                    # 3584: a merge runs only when no partition can end above this
ACC_MEAN = ACC_SLOTS // 4 * 3                     # 3072: the mean load a table is sized for
ACC_MIN_BITS = 4

_GOLDEN = U64(0x9E3779B97F4A7C15)
_M1, _M2 = U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)
_M1_INV, _M2_INV = U64(pow(int(_M1), -1, 1 << 64)), U64(pow(int(_M2), -1, 1 << 64))


def splitmix64(x):
    x = np.asarray(x, dtype=U64) + _GOLDEN
    x = (x ^ (x >> U64(30))) * _M1
    x = (x ^ (x >> U64(27))) * _M2
    return x ^ (x >> U64(31))


def _unxorshift(y, s):
    """x of y = x ^ (x >> s): the top s bits of y are x's; every round makes s more bits right"""
    x = y.copy()
    for _ in range(64 // s):
        x = y ^ (x >> U64(s))
    return x


def unsplitmix64(h):
    x = _unxorshift(np.asarray(h, dtype=U64), 31) * _M2_INV
    x = _unxorshift(x, 27) * _M1_INV
    return _unxorshift(x, 30) - _GOLDEN


# ------------------------------------------------------------------ strands (complement = code ^ 1, order A < T < C < G)

def mask_of(k):
    return U64((1 << (2 * k)) - 1)


def rc_np(keys, k):
    """rc of every key: field i of the result = field k - 1 - i of the key, complemented"""
    keys = np.asarray(keys, dtype=U64) & mask_of(k)
    out = np.zeros_like(keys)
    for i in range(k):
        out |= (((keys >> U64(2 * (k - 1 - i))) & U64(3)) ^ U64(1)) << U64(2 * i)
    return out


def rank_np(keys, k):
    """the number whose order is text order: base 0 in the top field"""
    keys = np.asarray(keys, dtype=U64)
    out = np.zeros_like(keys)
    for i in range(k):
        out |= ((keys >> U64(2 * i)) & U64(3)) << U64(2 * (k - 1 - i))
    return out


def canonical_np(keys, k):
    keys = np.asarray(keys, dtype=U64) & mask_of(k)
    rc = rc_np(keys, k)
    return np.where(rank_np(keys, k) <= rank_np(rc, k), keys, rc)


# ------------------------------------------------------------------ placement

def partition_of(keys, pbits):
    """the partition of every key in a table of 2^pbits partitions: the top pbits bits of the hash"""
    if pbits == 0:
        return np.zeros(len(keys), dtype=np.int64)
    return (splitmix64(keys) >> U64(64 - pbits)).astype(np.int64)


def home_of(keys):
    return (splitmix64(keys) & U64(ACC_SLOTS - 1)).astype(np.int64)


def _distinct(keys, n, rng):
    keys = np.unique(keys)
    assert len(keys) >= n, f"{len(keys)} keys survived, {n} wanted"
    return rng.permutation(keys)[:n]


def place(rng, n, prefix, bits, home=None, canonical=None):
    """n distinct k = 32 keys whose hash has `prefix` in its top `bits` bits, `home` (if given) in its low 12 bits and every
    other bit uniform -- the bit under the prefix too, so the keys share exactly `bits` bits.  canonical=True: only keys that
    are their own canonical form and no palindromes (rejection: about half of the candidates survive)."""
    assert 0 <= bits <= 40 and 0 <= prefix < (1 << bits)
    m = 2 * n + 64 if not canonical else 5 * n + 256
    h = rng.integers(0, 1 << 64, m, dtype=U64)
    if bits:
        h = (h & U64((1 << (64 - bits)) - 1)) | (U64(prefix) << U64(64 - bits))
    if home is not None:
        assert 0 <= home < ACC_SLOTS
        h = (h & ~U64(ACC_SLOTS - 1)) | U64(home)
    keys = unsplitmix64(h)
    if canonical:
        rc = rc_np(keys, 32)
        keys = keys[(canonical_np(keys, 32) == keys) & (rc != keys)]
    return _distinct(keys, n, rng)


def place_small_k(rng, n, k, prefix, bits):
    """the same for k < 32 by forward search: random keys below 4^k are hashed and the matching ones kept (no home control)"""
    assert k < 32 and bits <= 6 and 0 <= prefix < (1 << bits)
    m = (3 * n + 256) << bits
    assert m <= 1_000_000, "the search would take more than a million hashes"
    keys = rng.integers(0, 1 << (2 * k), m, dtype=U64)
    return _distinct(keys[partition_of(keys, bits) == prefix], n, rng)


# ------------------------------------------------------------------ groups

def add_up(keys, counts):
    """equal keys summed -> (keys ascending, uint64 counts)"""
    keys = np.asarray(keys, dtype=U64)
    counts = np.asarray(counts).astype(U64)
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    if not len(keys):
        return keys, counts
    at = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return keys[at], np.add.reduceat(counts, at).astype(U64)


def acc_bits_for(groups, at_least):
    """the fewest bits >= max(at_least, 4) whose partitions hold `groups` at a mean load of 3/4"""
    b = max(at_least, ACC_MIN_BITS)
    while groups > ACC_MEAN << b:
        b += 1
    return b


def bin_cap(n_in, pbits, want_cap=0):
    """entries of a partition's bin: the mean arrivals + 8 sigma + 32, or what an overflowed round saw; whole 32s, at most a
    partition"""
    mean = -(-n_in // (1 << pbits))
    cap = max(mean + 8 * int(np.sqrt(mean)) + 32, want_cap)
    return min(ACC_SLOTS, (cap + 31) // 32 * 32)


class Model:
    """the groups of an accumulator with the table's size, and the rounds every add takes"""

    def __init__(self, k=32):
        self.k, self.pbits = k, 0
        self.keys, self.counts = np.zeros(0, U64), np.zeros(0, U64)

    @property
    def partitions(self):
        return 1 << self.pbits if len(self.keys) else 0

    @property
    def groups(self):
        return self.keys, self.counts

    def occ(self, pbits=None):
        pbits = self.pbits if pbits is None else pbits
        return np.bincount(partition_of(self.keys, pbits), minlength=1 << pbits)

    def add(self, keys, canonical=False, counts=None):
        """a histogram of distinct keys (counts: ones unless given) -> (partitions afterwards, the rounds taken)"""
        keys = np.asarray(keys, dtype=U64)
        counts = np.ones(len(keys), U64) if counts is None else np.asarray(counts).astype(U64)
        n_in = len(keys)
        if n_in == 0:
            return self.partitions, []
        assert len(np.unique(keys)) == n_in, "the keys of one histogram are distinct"
        arr = canonical_np(keys, self.k) if canonical else keys
        flipped = arr != keys
        resident = np.isin(arr, self.keys)
        first_seen = np.zeros(n_in, bool)
        first_seen[np.unique(arr, return_index=True)[1]] = True
        is_new = ~resident & first_seen             # a pair new to the table is one new key
        distinct = len(self.keys)
        pbits = self.pbits
        if distinct == 0:                            # an empty accumulator is sized from the histogram
            pbits = acc_bits_for(n_in, pbits)
        want_cap, rounds = 0, []
        while True:
            assert len(rounds) <= 64
            P = 1 << pbits
            cap = bin_cap(n_in, pbits, want_cap)
            part = partition_of(arr, pbits)
            occ = self.occ(pbits)
            arrivals = np.bincount(part, minlength=P)
            m0, m1 = int((occ + arrivals).max()), int(arrivals.max())
            commit = m1 <= cap and m0 <= ACC_BOUND
            grow_for = distinct + n_in               # an upper bound of the groups after the add
            if not commit and cap < m1 <= ACC_SLOTS and m0 <= ACC_BOUND:
                want_cap = m1                        # a bin overflowed and the table has room: bin again, wider
                rounds.append("rebin")
                continue
            if not commit and m1 <= cap:             # dry run: how many arrivals are new keys
                new = np.bincount(part[is_new], minlength=P)
                new_hi = new
                name = "dry"
                if canonical:
                    # B1 puts the new unflipped keys into LDS; past 4096 slots its claims give up, and a flipped arrival
                    # whose partner found no slot counts as new: the number is then anything up to the arrivals
                    unflipped = np.bincount(part[~resident & ~flipped], minlength=P)
                    over = occ + unflipped > ACC_SLOTS
                    if over.any():
                        name = "dry-over"
                        new_hi = np.where(over, arrivals, new)
                got = arrivals > 0
                commit = int((occ + new)[got].max()) <= ACC_BOUND
                grow_for = distinct + int(new.sum())
                hi_commit = int((occ + new_hi)[got].max()) <= ACC_BOUND
                hi_for = distinct + int(new_hi.sum())
                assert commit == hi_commit and (commit or acc_bits_for(grow_for, pbits + 1) == acc_bits_for(hi_for, pbits + 1)), \
                    "the dry run's number is not exact here, and its two ends decide differently"
                rounds.append(name)
            if not commit:
                pbits = acc_bits_for(grow_for, pbits + 1)
                want_cap = 0
                rounds.append("grow")
                continue
            rounds.append("commit")
            break
        self.pbits = pbits
        self.keys, self.counts = add_up(np.concatenate([self.keys, arr]), np.concatenate([self.counts, counts]))
        assert int(self.occ().max()) <= ACC_BOUND
        return self.partitions, rounds


# ------------------------------------------------------------------ the placed streams (tests/test_acc_placement.py runs them
# on the device, tests/test_acc_model.py holds the model to the rounds written here)

class Step:
    """one add of a case: a histogram (distinct keys, counts), the rounds DESIGN.md 4.9's rules must take for it (None: what
    the model says) and the partitions afterwards (None likewise)"""

    def __init__(self, what, keys, counts, canonical=False, rounds=None, partitions=None, must=()):
        self.what, self.keys, self.counts, self.canonical = what, np.asarray(keys, dtype=U64), np.asarray(counts, dtype=U64), canonical
        self.rounds, self.partitions, self.must = rounds, partitions, tuple(must)


def counts_for(rng, n, hi=5):
    return rng.integers(1, hi + 1, n).astype(U64)


def _rng(*what):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


PART, PREFIX11 = 9, (9 << 7) | 0x55               # the one partition of 16 the cases fill; an 11-bit prefix inside it
EDGE = 5                                          # the partition whose bin the bin cases fill
GROW_4_TO_12 = ["grow"] * 8 + ["rebin", "commit"]


def case_chain(s0, n):
    """A: n keys of one partition and one home slot into an empty table, then the same keys with other counts"""
    rng = _rng("chain", s0, n)
    keys = place(rng, n, PART, 4, home=s0)
    first = {2: ["commit"], 97: ["rebin", "commit"], 3584: ["rebin", "commit"]}[n]
    # again: all resident.  At n = 3584 the bins overflow (3584 > cap 384) while occ + arrivals = 7168 is above the bound, and
    # a dry run needs bins that fit: the host grows although no key is new
    again = first if n < 3584 else None
    return [Step("one chain", keys, counts_for(rng, n), rounds=first, partitions=16),
            Step("the chain again", keys, counts_for(rng, n) + U64(7), rounds=again, partitions=16 if again else None,
                 must=() if again else ("grow",))]


def case_chain_mixed(s0=4095, n=2000):
    """A: into a chain of 2000 keys from slot 4095, 500 of its keys and 500 new ones homed at the chain's head, inside it and
    just past its end"""
    rng = _rng("chain mixed", s0, n)
    chain = place(rng, n, PART, 4, home=s0)
    end = (s0 + n) & (ACC_SLOTS - 1)
    new = np.concatenate([place(rng, 167, PART, 4, home=s0), place(rng, 167, PART, 4, home=(s0 + 1000) & (ACC_SLOTS - 1)),
                          place(rng, 166, PART, 4, home=end)])
    keys = rng.permutation(np.concatenate([chain[:500], new]))
    return [Step("a chain of 2000", chain, counts_for(rng, n), rounds=["rebin", "commit"], partitions=16),
            Step("500 resident + 500 new", keys, counts_for(rng, 1000), rounds=["rebin", "commit"], partitions=16)]


def case_bound_first(n):
    """B: n keys that share exactly an 11-bit prefix into an empty table"""
    rng = _rng("bound first", n)
    if n <= ACC_BOUND:
        return [Step(f"{n} keys", place(rng, n, PREFIX11, 11), counts_for(rng, n), rounds=["rebin", "commit"], partitions=16)]
    return [Step(f"{n} keys", place(rng, n, PREFIX11, 11), counts_for(rng, n), rounds=GROW_4_TO_12, partitions=4096)]


def case_bound_later(extra):
    """B: 3000 such keys resident, then `extra` more"""
    rng = _rng("bound later", extra)
    keys = place(rng, 3000 + extra, PREFIX11, 11)
    fits = 3000 + extra <= ACC_BOUND
    return [Step("3000 resident", keys[:3000], counts_for(rng, 3000), rounds=["rebin", "commit"], partitions=16),
            Step(f"{extra} more", keys[3000:], counts_for(rng, extra), rounds=["rebin", "commit"] if fits else GROW_4_TO_12,
                 partitions=16 if fits else 4096)]


def spread(rng, per_partition, bits=4, canonical=None):
    """per_partition[p] placed keys for every partition p of 2^bits, shuffled"""
    return rng.permutation(np.concatenate([place(rng, int(n), p, bits, canonical=canonical) for p, n in enumerate(per_partition)]))


def case_bin_edge(m):
    """B: 20 000 keys over 16 partitions (bins of 1568), one partition receives m"""
    rng = _rng("bin edge", m)
    rest = 20_000 - m
    per = [rest // 15 + (i < rest % 15) for i in range(15)]
    per.insert(EDGE, m)
    rounds = ["commit"] if m <= 1568 else ["rebin", "commit"]
    return [Step(f"{m} of 20000 in one bin", spread(rng, per), counts_for(rng, 20_000), rounds=rounds, partitions=16)]


def case_bin_drop():
    """B: the last partition receives 3000 of 20 000 keys, about twice its bin: the entries past the bin are dropped (the
    bins end with this one), and the second binning is far wider than the first"""
    rng = _rng("bin drop")
    per = [17_000 // 15 + (i < 17_000 % 15) for i in range(15)] + [3000]
    return [Step("3000 of 20000 in the last bin", spread(rng, per), counts_for(rng, 20_000), rounds=["rebin", "commit"], partitions=16)]


def case_slots(m):
    """B: one partition receives m = 4096 | 4097 new keys, the others 7 each: past the bound whatever the bins do"""
    rng = _rng("slots", m)
    per = [7] * 16
    per[EDGE] = m
    return [Step(f"{m} arrivals in one partition", spread(rng, per), counts_for(rng, sum(per)), must=("grow",))]


def case_dry_edge(r):
    """B: 2000 keys resident in partition 9 of 16; 2000 arrivals per partition, r of partition 9's resident"""
    rng = _rng("dry edge", r)
    res = place(rng, 2000, PART, 4)
    per = [2000] * 16
    per[PART] = 2000 - r
    keys = rng.permutation(np.concatenate([spread(rng, per), res[:r]]))
    fits = 2000 + 2000 - r <= ACC_BOUND
    return [Step("2000 resident", res, counts_for(rng, 2000), rounds=["rebin", "commit"], partitions=16),
            Step(f"32000 arrivals, {r} resident", keys, counts_for(rng, 32_000), rounds=["dry", "commit"] if fits else ["dry", "grow", "commit"],
                 partitions=16 if fits else 32)]


def case_pairs_chain(s0=4000, n=800):
    """C: n canonical keys of one partition and one home slot, each with its reverse complement in the same histogram"""
    rng = _rng("pairs chain", s0, n)
    c = place(rng, n, PART, 4, home=s0, canonical=True)
    keys = rng.permutation(np.concatenate([c, rc_np(c, 32)]))
    return [Step(f"{n} pairs in one chain", keys, counts_for(rng, 2 * n), canonical=True, rounds=["rebin", "commit"], partitions=16)]


def palindromes(rng, n):
    """k = 32 keys that are their own reverse complement: 16 random bases, then their reverse complement"""
    half = np.unique(rng.integers(0, 1 << 32, 2 * n, dtype=U64))[:n]
    return (rc_np(half, 16) << U64(32)) | half


def mixed_classes(rng, k, canon):
    """a histogram over 900 canonical keys: a third arrive with their reverse complement, a third alone, a third as the
    reverse complement only; key 0 and the all-G key; at k = 32 also 64 palindromes -> keys, shuffled"""
    assert len(canon) == 900
    extra = [np.array([0, int(mask_of(k))], dtype=U64)]
    if k == 32:
        extra.append(palindromes(rng, 64))
    return rng.permutation(np.concatenate([canon[:300], rc_np(canon[:300], k), canon[300:600], rc_np(canon[600:], k)] + extra))


def case_mixed(resident_half, k=32):
    """C: the three classes into an empty table, or into one that holds every other canonical key"""
    rng = _rng("mixed", resident_half, k)
    if k == 32:
        canon = place(rng, 900, 3, 4, home=4090, canonical=True)
    else:
        some = place_small_k(rng, 2400, k, 3, 4)
        some = some[(canonical_np(some, k) == some) & (some != 0)]       # (an odd k has no palindromes)
        canon = some[:900]
    keys = mixed_classes(rng, k, canon)
    steps = [Step("pairs, unflipped only, flipped only", keys, counts_for(rng, len(keys)), canonical=True, partitions=16)]
    if resident_half:
        steps.insert(0, Step("every other canonical key", canon[::2], counts_for(rng, 450), canonical=True, partitions=16))
    return steps


def case_exception():
    """C: 3584 canonical keys resident in partition 9; 600 new pairs for it and 1000 canonical singles for every other one"""
    rng = _rng("exception")
    res = place(rng, 3584 + 600, PART, 4, canonical=True)
    per = [1000] * 16
    per[PART] = 0
    keys = rng.permutation(np.concatenate([res[3584:], rc_np(res[3584:], 32), spread(rng, per, canonical=True)]))
    return [Step("3584 resident", res[:3584], counts_for(rng, 3584), canonical=True, rounds=["rebin", "commit"], partitions=16),
            Step("600 pairs past the slots", keys, counts_for(rng, len(keys)), canonical=True, rounds=["dry-over", "grow", "commit"],
                 partitions=32)]


def case_bound_k21(n):
    """C: the bound at k = 21: n keys that share a 6-bit prefix (forward search)"""
    rng = _rng("bound k21", n)
    keys = place_small_k(rng, n, 21, 0x26, 6)
    rounds = ["rebin", "commit"] if n <= ACC_BOUND else ["grow"] * 3 + ["rebin", "commit"]
    return [Step(f"{n} keys, k = 21", keys, counts_for(rng, n), rounds=rounds, partitions=16 if n <= ACC_BOUND else 128)]


CASES = {
    **{f"chain-s{s0}-n{n}": (case_chain, (s0, n), 32) for s0 in (0, 2047, 4000, 4095) for n in (2, 97, 3584)},
    "chain-mixed": (case_chain_mixed, (), 32),
    "bound-first-3584": (case_bound_first, (3584,), 32), "bound-first-3585": (case_bound_first, (3585,), 32),
    "bound-later-584": (case_bound_later, (584,), 32), "bound-later-585": (case_bound_later, (585,), 32),
    "bin-edge-1568": (case_bin_edge, (1568,), 32), "bin-edge-1569": (case_bin_edge, (1569,), 32),
    "bin-drop-last": (case_bin_drop, (), 32),
    "slots-4096": (case_slots, (4096,), 32), "slots-4097": (case_slots, (4097,), 32),
    "dry-edge-416": (case_dry_edge, (416,), 32), "dry-edge-415": (case_dry_edge, (415,), 32),
    "pairs-chain": (case_pairs_chain, (), 32),
    "mixed-empty": (case_mixed, (False,), 32), "mixed-resident": (case_mixed, (True,), 32),
    "exception": (case_exception, (), 32),
    "k21-bound-3584": (case_bound_k21, (3584,), 21), "k21-bound-3585": (case_bound_k21, (3585,), 21),
    "k21-mixed-empty": (case_mixed, (False, 21), 21), "k21-mixed-resident": (case_mixed, (True, 21), 21),
}

_STEPS = {}


def steps_of(name):
    """the adds of a case (built once, never modified) and its k"""
    if name not in _STEPS:
        fn, args, k = CASES[name]
        steps = fn(*args)
        for s in steps:
            s.keys.setflags(write=False)
            s.counts.setflags(write=False)
        _STEPS[name] = (steps, k)
    return _STEPS[name]


def run_model(name, want_model=False):
    """every step of a case through a Model, each held to what the case says -> [(step, partitions, rounds, groups after)]
    (want_model: and the Model, to go on from)"""
    steps, k = steps_of(name)
    m, out = Model(k), []
    for s in steps:
        out.append((s,) + check_step(m, s, name))
    return (out, m) if want_model else out


def check_step(m, s, name=""):
    """one Step into the Model m, held to what the step says -> (partitions, rounds, groups after)"""
    parts, rounds = m.add(s.keys, s.canonical, s.counts)
    if s.rounds is not None:
        assert rounds == s.rounds, f"{name}, {s.what}: the model takes {rounds}, the case is written for {s.rounds}"
    if s.partitions is not None:
        assert parts == s.partitions, f"{name}, {s.what}: {parts} partitions, the case is written for {s.partitions}"
    for b in s.must:
        assert b in rounds, f"{name}, {s.what}: no {b} in {rounds}"
    return parts, rounds, m.groups
