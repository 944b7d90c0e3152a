"""Times the count-ordered queries (dnagpu_*_spectrum / _select / _top) on config 3's histogram (k = 31, 248956422
synthetic bases, every count 1), on its repeat-rich variant 3m1000 and on an accumulator holding config 3, against what a
caller had to do for the same answers before: download every group (dnagpu_hist_download / dnagpu_acc_download) and let
numpy answer on the host.

usage: python tools/query_probe.py [hist3] [acc3] [hist3m1000] [--reps N]     (default: all three)
Prints one JSON line per measurement.  Times are host clocks in ms around calls that end in a read-back, after one warm-up
of the same shapes."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
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
                probe(name, acc, want, reps, 4096 << pbits, 16)
                acc.free()
            else:
                probe(name, h, want, reps, h.extent, 4)
                h.free()
            ctx.trim()


if __name__ == "__main__":
    main()
