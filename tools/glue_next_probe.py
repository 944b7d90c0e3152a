"""Times the per-row _next loops of the glue's streaming objects: about 10^6 served rows each from count_kmers (one sequence),
count_kmers_agg and table_kmers (a table of rows of 1000 bases) and table_hits (10^6 short rows).  The loop is the ctypes
loop of glue.py, so a figure is the call overhead of Python plus the glue's own work per row; the first _next, which runs
the last flush and the device work, is timed apart.

usage: python tools/glue_next_probe.py [--rows N] [--reps N]      (default 1000000 rows, 5 repetitions)
Prints one JSON line per object: `ms` is the median over the repetitions of the loop over all rows but the first, `ms_best`
the least, `first_ms` the median of the first call."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SEED = 0x61CE


def text(rng, n):
    return np.frombuffer(b"ATCG", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)].tobytes().decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    glue = importlib.import_module(load_package().__name__ + ".glue")
    L = glue.lib()
    rng = np.random.default_rng(SEED)
    k = 16
    one = glue.dna(text(rng, a.rows + k - 1))
    table = [glue.dna(text(rng, 1000)) for _ in range(max(1, a.rows // (1000 - k + 1)))]
    short = [glue.dna(text(rng, k + 3)) for _ in range(1000)]
    km, v = glue._Kmer(), [C.c_int64() for _ in range(3)]
    kmr, vr = C.byref(km), [C.byref(x) for x in v]

    def count_kmers():
        h = L.count_kmers_begin(one.p, k)
        return h, (lambda: L.count_kmers_next(h, kmr, vr[0])), L.count_kmers_end

    def count_kmers_agg():
        h = L.count_kmers_agg_begin(k)
        for r in table:
            assert L.count_kmers_agg_add(h, r.p)
        return h, (lambda: L.count_kmers_agg_next(h, kmr, vr[0])), L.count_kmers_agg_end

    def table_kmers():
        h = L.table_kmers_begin(k, b"\0", None, None)
        for r in table:
            assert L.table_kmers_add(h, r.p)
        return h, (lambda: L.table_kmers_next(h, vr[0], vr[1], kmr)), L.table_kmers_end

    set_agg = glue.count_kmers_table_agg(k, rows=table[:8])

    def table_hits():
        h = L.table_hits_begin(set_agg.a, False, 1, -1)
        for i in range(a.rows):
            L.table_hits_add(h, short[i % len(short)].p)
        return h, (lambda: L.table_hits_next(h, vr[0], vr[1], vr[2])), L.table_hits_end

    for make in (count_kmers, count_kmers_agg, table_kmers, table_hits):
        first, loop, rows = [], [], 0
        for _ in range(a.reps + 1):
            h, step, end = make()
            assert h, L.dna_glue_errmsg()
            t0 = time.perf_counter()
            ok = step()
            t1 = time.perf_counter()
            rows = 1 if ok else 0
            while step():
                rows += 1
            t2 = time.perf_counter()
            end(h)
            first.append((t1 - t0) * 1e3)
            loop.append((t2 - t1) * 1e3)
        first, loop = first[1:], loop[1:]                             # (the first round warms up)
        print(json.dumps(dict(what=make.__name__ + "_next", rows=rows, ms=float(np.median(loop)), ms_best=min(loop),
                              ns_per_row=float(np.median(loop)) * 1e6 / max(rows, 1), first_ms=float(np.median(first)))), flush=True)
    set_agg.end()


if __name__ == "__main__":
    main()
