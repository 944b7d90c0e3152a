"""Times dnagpu_acc_add (the k-mer accumulator) on the workloads DESIGN.md "accumulator" reports:

  cfg3        config 3's histogram (k = 31, 248956422 synthetic bases) into an empty accumulator, and into one already
              holding it
  cfg6        config 6's table (10^7 reads of 150 bases, k = 31) counted in 8 batches; the batches added up through the
              accumulator against the same batches through the dnagpu_hist_merge chain (which still fits under 2^32 there)
  cfg4x2      config 4's histogram (3 * 10^9 bases) added twice: total 2 * 2999999970, past 2^32
  strand      config 4's histogram (k = 31, the largest size here) through add and through add_canonical,
              each into an empty accumulator and into one that already holds it; the two alternate inside one run

usage: python tools/acc_probe.py [cfg3] [cfg6] [cfg4x2] [strand] [--reps N]     (default: the first three)
Prints one JSON line per measurement.  Times are host clocks around calls that end in a device synchronise (every add
reads its result back), after one warm-up of the same shapes."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

DIGESTS = json.load(open(os.path.join(ROOT, "tests", "golden", "config_digests.json")))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def emit(**kw):
    print(json.dumps(kw), flush=True)


def cfg3(pkg, ctx, reps):
    want = DIGESTS["3"]
    d = ctx.synth(want["seed"], want["n_bases"])
    h = ctx.count_kmers_unordered(d, want["k"])
    d.free()
    empty_ms, again_ms = [], []
    for r in range(reps + 1):                      # (rep 0: warm-up -- the pool's first hipMallocs)
        acc = ctx.accumulator(want["k"])
        t1, _ = timed(lambda: acc.add(h))
        t2, _ = timed(lambda: acc.add(h))
        if r:
            empty_ms.append(t1)
            again_ms.append(t2)
        if r == reps:
            s = acc.summary()
            assert s[0] == 2 * want["total"] and s[1] == want["distinct"], s
        acc.free()
    acc = ctx.accumulator(want["k"])
    acc.add(h)
    assert acc.summary() == (want["total"], want["distinct"], want["unique"], want["checksum"])
    acc.free()
    d_groups = h.distinct
    emit(probe="cfg3", groups=d_groups, add_empty_ms=empty_ms, add_again_ms=again_ms,
         estimate_bytes_empty=44 * d_groups, estimate_bytes_again=44 * d_groups + 43 * d_groups,
         digest_ok=True)
    h.free()


def cfg6(pkg, ctx, reps):
    import numpy as np
    seed, n_reads, read_len, k, batches = 0xD2A0006, 10_000_000, 150, 31, 8
    d = ctx.synth(seed, n_reads * read_len)
    per = n_reads // batches
    words_per = per * read_len // 32               # (150 * 1.25 M bases: a whole number of words)
    st = np.arange(per + 1, dtype=np.uint64) * np.uint64(read_len)
    views = [ctx.wrap(d.device_words + b * words_per * 8, words_per, per * read_len) for b in range(batches)]
    count_ms, hs = [], []
    for v in views:
        t, h = timed(lambda: ctx.count_kmers_batch(v, st, k))
        count_ms.append(t)
        hs.append(h)
    acc_ms, merge_ms = [], []
    for r in range(reps + 1):
        acc = ctx.accumulator(k)
        t_acc = sum(timed(lambda h=h: acc.add(h))[0] for h in hs)
        t0 = time.perf_counter()
        m = hs[0].merge(hs[1])
        for h in hs[2:]:
            m2 = m.merge(h)
            m.free()
            m = m2
        t_merge = (time.perf_counter() - t0) * 1e3
        if r:
            acc_ms.append(t_acc)
            merge_ms.append(t_merge)
        if r == reps:
            assert acc.summary() == m.summary()
            summary = acc.summary()
        m.free()
        acc.free()
    emit(probe="cfg6_8_batches", rows=sum(h.total for h in hs), count_batches_ms=count_ms, acc_adds_ms=acc_ms,
         merge_chain_ms=merge_ms, summary=summary, same_as_merge_chain=True)
    for h in hs:
        h.free()
    for v in views:
        v.free()
    d.free()


def cfg4x2(pkg, ctx, reps):
    want = DIGESTS["4"]
    d = ctx.synth(want["seed"], want["n_bases"])
    h = ctx.count_kmers_unordered(d, want["k"])
    d.free()
    acc = ctx.accumulator(want["k"])
    t1, _ = timed(lambda: acc.add(h))
    t2, _ = timed(lambda: acc.add(h))
    s = acc.summary()
    ok = s[0] == 2 * want["total"] and s[1] == want["distinct"] and s[2] == 0
    emit(probe="cfg4x2", groups=h.distinct, add_first_ms=t1, add_second_ms=t2, summary=s,
         expected=[2 * want["total"], want["distinct"], 0], ok=ok)
    acc.free()
    h.free()
    if not ok:
        raise SystemExit(3)


def strand(pkg, ctx, reps):
    want = DIGESTS["4"]
    d = ctx.synth(want["seed"], want["n_bases"])
    h = ctx.count_kmers_unordered(d, want["k"])
    d.free()
    ms = {(c, w): [] for c in (False, True) for w in ("empty", "resident")}
    distinct = {}
    for r in range(reps + 1):                      # (rep 0: warm-up -- the pool's first hipMallocs)
        for canonical in (False, True):
            acc = ctx.accumulator(want["k"])
            t1, _ = timed(lambda: acc.add(h, canonical=canonical))
            t2, _ = timed(lambda: acc.add(h, canonical=canonical))
            if r:
                ms[(canonical, "empty")].append(t1)
                ms[(canonical, "resident")].append(t2)
            assert acc.total == 2 * want["total"]
            distinct[canonical] = acc.distinct
            acc.free()                             # (back to the pool: the next accumulator takes the same buffers)
    assert distinct[False] == want["distinct"] and distinct[True] <= distinct[False]
    best = {key: min(v) for key, v in ms.items()}
    emit(probe="strand", groups=h.distinct, canonical_groups=distinct[True],
         add_empty_ms=ms[(False, "empty")], add_canonical_empty_ms=ms[(True, "empty")],
         add_resident_ms=ms[(False, "resident")], add_canonical_resident_ms=ms[(True, "resident")],
         ratio_empty=best[(True, "empty")] / best[(False, "empty")],
         ratio_resident=best[(True, "resident")] / best[(False, "resident")])
    h.free()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = 3
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
        args = [a for a in args if a != str(reps)]
    pkg = load_package()
    with pkg.Context(0) as ctx:
        for name in args or ["cfg3", "cfg6", "cfg4x2"]:
            {"cfg3": cfg3, "cfg6": cfg6, "cfg4x2": cfg4x2, "strand": strand}[name](pkg, ctx, reps)
            ctx.trim()


if __name__ == "__main__":
    main()
