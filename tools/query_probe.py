"""Times the count-ordered queries (dnagpu_*_spectrum / _select / _top / _rank) on config 3's histogram (k = 31, 248956422
synthetic bases, every count 1), on its repeat-rich variant 3m1000 and on an accumulator holding config 3, against what a
caller had to do for the same answers before: download every group (dnagpu_hist_download / dnagpu_acc_download) and let
numpy answer on the host.

usage: python tools/query_probe.py [hist3] [acc3] [hist3m1000] [--reps N] [--rank-only] [--no-baseline]     (default: all three)
rank(DESC) -- every group in count order, no LIMIT -- is timed beside the only way there was before it: download every group,
then np.lexsort on the host; both must give the same count sequence and the same set of groups.  --rank-only skips the other
queries, --no-baseline the host side (a run under a profiler).
Prints one JSON line per measurement.  Times are host clocks in ms around calls that end in a read-back, after one warm-up
of the same shapes."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle as orc  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

DIGESTS = json.load(open(os.path.join(ROOT, "tests", "golden", "config_digests.json")))
U64_MAX = 2 ** 64 - 1


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def emit(**kw):
    print(json.dumps(kw), flush=True)


def probe(name, q, want, reps, slots, slot_bytes):
    """q: a Hist or an Accumulator"""
    queries = {
        "spectrum256": lambda: q.spectrum(256),
        "select2_count": lambda: q.select(2, U64_MAX, cap=0),
        "select2_rows": lambda: q.select(2, U64_MAX),
        "top100": lambda: q.top(100),
    }
    ms = {k: [] for k in queries}
    for r in range(reps + 1):                      # (rep 0: warm-up -- the pool's first hipMallocs)
        for k, fn in queries.items():
            t, res = timed(fn)
            if r:
                ms[k].append(round(t, 3))
    sp = q.spectrum(256)
    _, _, n2 = q.select(2, U64_MAX, cap=0)
    tk, tc = q.top(100)
    assert int(sp.sum()) == want["distinct"] and int(sp[0]) == want["unique"]
    assert n2 == want["distinct"] - want["unique"] and int(tc[0]) == want["max_count"]
    # the baseline: every group over the bus, numpy on the host (existing code, timed once: it takes seconds)
    t_dl, (keys, counts) = timed(q.download)
    t_sp, sp_host = timed(lambda: np.bincount(np.minimum(counts, np.uint64(256)).astype(np.int64), minlength=257)[1:])
    t_sel, sel = timed(lambda: np.flatnonzero(counts >= 2))
    def host_top():
        part = np.argpartition(counts, len(counts) - 100)[-100:]
        order = np.lexsort((keys[part], -counts[part].astype(np.int64)))
        return keys[part][order], counts[part][order]
    t_top, (hk, hc) = timed(host_top)
    assert np.array_equal(sp_host.astype(np.uint64), sp) and len(sel) == n2 and np.array_equal(hc, tc)
    emit(probe=name, groups=want["distinct"], slots=slots, ms=ms,
         estimate_ms_at_4TBs={"spectrum256": slots * slot_bytes / 4e9, "select2": (slots * slot_bytes + 16 * n2) / 4e9},
         baseline_ms={"download_all": round(t_dl, 1), "numpy_spectrum": round(t_sp, 1), "numpy_select": round(t_sel, 1),
                      "numpy_top100": round(t_top, 1)},
         answers_equal=True)


def probe_rank(name, q, want, reps, slots, slot_bytes, baseline):
    """rank(DESC) of a Hist or an Accumulator: the call (it ends in a read-back), then the whole order over the bus"""
    ms, r = [], None
    for i in range(reps + 1):                      # (rep 0: warm-up)
        if r is not None:
            r.free()
        t, r = timed(q.rank)
        if i:
            ms.append(round(t, 3))
    assert r.rows == want["distinct"]
    t_read, (gk, gc) = timed(r.read)
    r.free()
    assert np.all(gc[1:] <= gc[:-1]) and int(gc[0]) == want["max_count"] and int(gc.sum()) == want["total"]
    total, distinct, unique, checksum = q.summary()
    assert orc.hist_summary(gk, gc) == (total, distinct, unique, checksum)     # the same (key, count) pairs, digest-wise
    # 4 B (histogram) or 16 B (accumulator) per slot for the sizes, 12 B / 16 B per slot read again, 16 B per row written
    est = (slots * slot_bytes + slots * (12 if slot_bytes == 4 else 16) + 16 * want["distinct"]) / 4e9
    out = dict(probe=name + ":rank", groups=want["distinct"], slots=slots, ms={"rank_desc": ms, "read_all_rows": round(t_read, 1)},
               estimate_ms_at_4TBs={"rank_desc": round(est, 3)})
    if baseline:
        emit(probe=name + ":rank", step="the baseline: download every group, np.lexsort on the host (minutes)")
        t_dl, (keys, counts) = timed(q.download)
        t_sort, order = timed(lambda: np.lexsort((keys, -counts.astype(np.int64))))
        assert np.array_equal(counts[order], gc), "rank and the host sort disagree on the count sequence"
        del order, counts
        assert np.array_equal(np.sort(gk), np.sort(keys)), "rank and the download disagree on the set of groups"
        out["baseline_ms"] = {"download_all": round(t_dl, 1), "numpy_lexsort": round(t_sort, 1)}
        out["baseline_over_rank"] = round((t_dl + t_sort) / (sorted(ms)[len(ms) // 2] + t_read), 1)
        out["answers_equal"] = True
    emit(**out)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rank_only, baseline = "--rank-only" in sys.argv, "--no-baseline" not in sys.argv
    reps = 3
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
        args = [a for a in args if a != str(reps)]
    pkg = load_package()
    with pkg.Context(0) as ctx:
        for name in args or ["hist3", "acc3", "hist3m1000"]:
            want = DIGESTS["3m1000" if name.endswith("m1000") else "3"]
            d = ctx.synth(want["seed"], want["n_bases"], want["motif"])
            h = ctx.count_kmers_unordered(d, want["k"])
            d.free()
            if name.startswith("acc"):
                acc = ctx.accumulator(want["k"])
                acc.add(h)
                h.free()
                pbits = 4
                while want["distinct"] > ((4096 << pbits) // 4) * 3:       # (acc_bits_for of dnagpu_api.hip)
                    pbits += 1
                if not rank_only:
                    probe(name, acc, want, reps, 4096 << pbits, 16)
                probe_rank(name, acc, want, reps, 4096 << pbits, 16, baseline)
                acc.free()
            else:
                if not rank_only:
                    probe(name, h, want, reps, h.extent, 4)
                probe_rank(name, h, want, reps, h.extent, 4, baseline)
                h.free()
            ctx.trim()


if __name__ == "__main__":
    main()
