"""Times dnagpu_generate_kmers_table (the rows of a table of sequences) on config 5's data -- seed 0xD2A0001,
100 Mbase, k = 21, pattern NNNNNNNNNNWSNNNNNNNNN -- cut into reads of 150 bases, beside dnagpu_generate_kmers_filtered over
the same packed stream in the same process (the single-sequence kernels: what there was before).  All outputs stay in device
memory, so the times are the two sweeps and nothing else.

usage: python tools/table_rows_probe.py [--reps N] [--bases N]
Forms: single keys+pos | table keys | table keys+pos | table keys+seq+pos | table, no filter, keys+seq+pos over a 2^26-row
window.  Per form one JSON line: host-clock ms per call (after one warm-up), the HIP-event phase times of the last call
(dnagpu_set_profiling), the rows written, and the bytes the form must move: both sweeps read the packed input (2 bits per
base; the table forms also the marks, 1 bit per base), the write sweep stores 8 bytes per array and row."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SEED, K, PATTERN, READ = 0xD2A0001, 21, "NNNNNNNNNNWSNNNNNNNNN", 150


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bases", type=int, default=100_000_000)
    a = ap.parse_args()
    pkg = load_package()
    n = a.bases
    rows = n - K + 1
    starts = np.arange(0, n + READ, READ, dtype=np.uint64)
    starts[-1] = n
    if len(starts) > 1 and starts[-2] >= n:
        starts = starts[:-1]
        starts[-1] = n
    with pkg.Context(0) as ctx:
        d = ctx.synth(SEED, n)
        d.set_sequences(starts)
        flt = pkg.Filter.contains(PATTERN)
        window = min(1 << 26, rows)
        cap = max(rows // 3, window)               # the pattern keeps a quarter of the rows
        bufs = [ctx.buffer_alloc(cap * 8) for _ in range(3)]
        pk, ps, pp = (C.c_void_p(b) for b in bufs)
        forms = [
            ("single keys+pos", rows, 2, 2, lambda: ctx.count_matches_device(d, K, flt, 0, rows, pk, pp, cap)),
            ("table keys", rows, 3, 1, lambda: ctx.generate_kmers_table_device(d, K, flt, 0, rows, pk, None, None, cap)),
            ("table keys+pos", rows, 3, 2, lambda: ctx.generate_kmers_table_device(d, K, flt, 0, rows, pk, None, pp, cap)),
            ("table keys+seq+pos", rows, 3, 3, lambda: ctx.generate_kmers_table_device(d, K, flt, 0, rows, pk, ps, pp, cap)),
            ("table no filter keys+seq+pos 2^26 rows", window, 3, 3,
             lambda: ctx.generate_kmers_table_device(d, K, None, 0, window, pk, ps, pp, cap)),
        ]
        ctx.set_profiling(True)
        for name, swept, bits, arrays, fn in forms:
            ms = []
            for r in range(a.reps + 1):            # (rep 0: warm-up)
                t0 = time.perf_counter()
                n_out = fn()
                t = (time.perf_counter() - t0) * 1e3
                if r:
                    ms.append(round(t, 3))
            assert n_out <= cap
            nbytes = 2 * swept * bits / 8 + n_out * 8 * arrays
            print(json.dumps({"form": name, "stream_rows": swept, "rows_out": n_out, "host_ms": ms, "median_ms": float(np.median(ms)),
                              "phases_ms": [(p, round(v, 3)) for p, v in ctx.last_phase_times()],
                              "bytes": int(nbytes), "GBps_at_median": round(nbytes / np.median(ms) / 1e6, 1)}), flush=True)
        for b in bufs:
            ctx.buffer_free(b)
        d.free()


if __name__ == "__main__":
    main()
