"""Times dnagpu_table_hits (per-sequence hits of a table's k-mers in a counted set) on a resident synthetic
table -- seed 0xD2A0001, 10^9 bases by default -- once cut into reads of 100 bases and once as a single sequence, at k = 21
and 31, against sets of growing size counted from a second synthetic sequence:
  empty     an accumulator without a table: the sweep is skipped, what remains is the gather
  one key   a set of one group: every row forms its key, hashes it and finds its partition empty -- the sweep without probes
  1e6, 1e8  sets of about that many groups (the table fits an XCD's L2 share / lies beyond the Infinity Cache)
and, as the floor, dnagpu_generate_kmers_table with no filter and no output arrays (its count sweep) over the same table.

usage: python tools/table_hits_probe.py [--reps N] [--bases N] [--sets 1000000,100000000] [--ks 21,31] [--read 100]
Per measurement one JSON line: host-clock ms per call (after one warm-up; the call waits for its work), the table's rows, the
rows per second at the median, the totals the call returned, and the set's groups and partitions."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SEED, SET_SEED = 0xD2A0001, 0xD2A0005


def timed(fn, reps):
    ms, out = [], None
    for r in range(reps + 1):                      # (rep 0: warm-up)
        t0 = time.perf_counter()
        out = fn()
        t = (time.perf_counter() - t0) * 1e3
        if r:
            ms.append(round(t, 3))
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    ap.add_argument("--sets", default="1000000,100000000")
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--read", type=int, default=100)
    a = ap.parse_args()
    pkg = load_package()
    n = a.bases
    read_starts = np.arange(0, n + a.read, a.read, dtype=np.uint64)
    read_starts = read_starts[read_starts < n]
    read_starts = np.concatenate([read_starts, np.array([n], dtype=np.uint64)])
    layouts = [("reads", read_starts), ("single", np.array([0, n], dtype=np.uint64))]

    def report(**kw):
        print(json.dumps(kw), flush=True)

    with pkg.Context(0) as ctx:
        d = ctx.synth(SEED, n)
        for k in [int(x) for x in a.ks.split(",")]:
            sets = [("empty", ctx.accumulator(k))]
            for groups in [1] + [int(x) for x in a.sets.split(",")]:
                src = ctx.synth(SET_SEED, groups + k - 1)
                h = ctx.count_kmers(src, k) if groups == 1 else ctx.count_kmers_unordered(src, k)
                acc = ctx.accumulator(k)
                acc.add(h)
                h.free()
                src.free()
                sets.append(("one key" if groups == 1 else f"{groups:.0e}", acc))
            for layout, starts in layouts:
                d.set_sequences(starts)
                table_rows = int(np.maximum(np.diff(starts).astype(np.int64) - k + 1, 0).sum())
                stream_rows = n - k + 1
                ms, got = timed(lambda: ctx.generate_kmers_table_device(d, k, None, 0, stream_rows, None, None, None, 0), a.reps)
                assert got == table_rows
                floor = float(np.median(ms))
                report(form="count sweep of generate_kmers_table", k=k, layout=layout, sequences=len(starts) - 1, rows=table_rows,
                       host_ms=ms, median_ms=floor, rows_per_s=round(table_rows / floor * 1e3))

                for name, acc in sets:
                    def call():
                        with ctx.table_hits(d, acc) as sh:
                            return sh.totals()
                    ms, tot = timed(call, a.reps)
                    med = float(np.median(ms))
                    assert tot[0] == table_rows
                    report(form="table_hits", k=k, layout=layout, set=name, set_groups=acc.distinct, set_partitions=acc.partitions,
                           sequences=len(starts) - 1, rows=table_rows, hits=tot[1], seqs_hit=tot[2], host_ms=ms, median_ms=med,
                           rows_per_s=round(table_rows / med * 1e3), ratio_to_count_sweep=round(med / floor, 3))
            for _, acc in sets:
                acc.free()
        d.free()


if __name__ == "__main__":
    main()
