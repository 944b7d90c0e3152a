"""Times dnagpu_table_profile (the k-mer profile of every sequence of a table) with device output on a resident
synthetic table -- seed 0xD2A0001, 10^9 bases by default -- cut into reads of 100 bases, into contigs of 10^4 bases, and as a
single sequence, at k = 1, 4 and 6, forward and canonical.  The matrix of a whole table need not fit: the table is walked in
windows of at most --matrix-bytes of output (as a caller pages), and a time is that of ALL windows.  Beside each time, in the
same process:
  count sweep   dnagpu_generate_kmers_table with no filter and no output arrays over the same rows: what reading the stream
                and its boundaries costs
  fill          hipMemsetAsync of one window's matrix, times the windows: what writing the answer costs
  host path     what a caller has without this entry point: dnagpu_generate_kmers_table with keys and sequence ids to the
                host, then np.bincount(seq * 4^k + key).  Measured on the sequences of the first --host-bases bases only (it
                moves 16 bytes per row; a layout whose first sequence is longer has no such line), with the profile of the
                SAME window beside it.

usage: python tools/table_profile_probe.py [--reps N] [--bases N] [--ks 1,4,6] [--layouts reads,contigs,single]
                                           [--matrix-bytes N] [--host-bases N] [--host-rows N]
Per measurement one JSON line: host-clock ms (after one warm-up; every call waits for its work)."""
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

SEED = 0xD2A0001
LAYOUTS = {"reads": 100, "contigs": 10_000, "single": 0}


def timed(fn, reps):
    ms, out = [], None
    for r in range(reps + 1):                      # (rep 0: warm-up)
        t0 = time.perf_counter()
        out = fn()
        t = (time.perf_counter() - t0) * 1e3
        if r:
            ms.append(round(t, 3))
    return ms, out


def starts_of(n, piece):
    if not piece:
        return np.array([0, n], dtype=np.uint64)
    s = np.arange(0, n, piece, dtype=np.uint64)
    return np.concatenate([s, np.array([n], dtype=np.uint64)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    ap.add_argument("--ks", default="1,4,6")
    ap.add_argument("--layouts", default="reads,contigs,single")
    ap.add_argument("--matrix-bytes", type=int, default=4 << 30)
    ap.add_argument("--host-bases", type=int, default=100_000_000)
    ap.add_argument("--host-rows", type=int, default=25_000_000, help="stream rows per call of the host path")
    a = ap.parse_args()
    pkg = load_package()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    n = a.bases

    def report(**kw):
        print(json.dumps(kw), flush=True)

    with pkg.Context(0) as ctx:
        d = ctx.synth(SEED, n)
        for layout in a.layouts.split(","):
            starts = starts_of(n, LAYOUTS[layout])
            n_seqs = len(starts) - 1
            d.set_sequences(starts)
            for k in [int(x) for x in a.ks.split(",")]:
                width = pkg.profile_width(k)
                table_rows = int(np.maximum(np.diff(starts).astype(np.int64) - k + 1, 0).sum())
                per_window = max(min(n_seqs, a.matrix_bytes // (4 * width)), 1)
                windows = [(f, min(per_window, n_seqs - f)) for f in range(0, n_seqs, per_window)]
                out = ctx.buffer_alloc(4 * width * per_window)
                common = dict(layout=layout, k=k, sequences=n_seqs, rows=table_rows, windows=len(windows),
                              matrix_bytes=4 * width * n_seqs)

                ms, got = timed(lambda: ctx.generate_kmers_table_device(d, k, None, 0, n - k + 1, None, None, None, 0), a.reps)
                assert got == table_rows
                sweep = float(np.median(ms))
                report(form="count sweep of generate_kmers_table", host_ms=ms, median_ms=sweep, **common)

                def fill():
                    for _, c in windows:
                        assert hip.hipMemsetAsync(out, 0, 4 * width * c, ctx.stream) == 0
                    ctx.synchronize()
                ms, _ = timed(fill, a.reps)
                fill_ms = float(np.median(ms))
                report(form="hipMemsetAsync of the matrix", host_ms=ms, median_ms=fill_ms, **common)

                for canonical in (False, True):
                    def call():
                        for f, c in windows:
                            ctx.table_profile(d, k, canonical=canonical, seq_first=f, seq_count=c, out_counts_dev=out)
                    ms, _ = timed(call, a.reps)
                    med = float(np.median(ms))
                    report(form="table_profile", canonical=canonical, host_ms=ms, median_ms=med,
                           rows_per_s=round(table_rows / med * 1e3), ratio_to_sweep_plus_fill=round(med / (sweep + fill_ms), 3),
                           **common)

                # the path a caller has today, on the first sequences only, and the profile of the same window
                hs = min(int(np.searchsorted(starts, a.host_bases, side="right")) - 1, n_seqs, per_window,
                         (1 << 27) // width)               # (and a host matrix of at most 2^27 int64 cells)
                if hs < 1:                                 # (a single sequence of 10^9 bases: 16 GB would cross the bus)
                    ctx.buffer_free(out)
                    continue
                end = int(starts[hs])
                stream_rows = max(end - k + 1, 0)          # (rows that start before `end`; the last sequences' own are among them)

                def host_path():
                    acc = np.zeros(hs * width, dtype=np.int64)
                    for f in range(0, stream_rows, a.host_rows):
                        keys, seq, _, _ = ctx.generate_kmers_table(d, k, None, f, min(a.host_rows, stream_rows - f), want_pos=False)
                        keep = seq < hs
                        acc += np.bincount(seq[keep].astype(np.int64) * width + keys[keep].astype(np.int64), minlength=hs * width)
                    return acc
                ms_h, ref = timed(host_path, 1)
                ms_p, _ = timed(lambda: ctx.table_profile(d, k, seq_first=0, seq_count=hs, out_counts_dev=out), a.reps)
                got = ctx.download_bytes(out, 4 * width * hs).view(np.uint32)
                assert np.array_equal(got.astype(np.int64), ref), "the two paths disagree"
                report(form="host path against table_profile, same window", layout=layout, k=k, sequences=hs, bases=end,
                       host_path_ms=ms_h, table_profile_ms=ms_p, ratio=round(float(np.median(ms_h)) / float(np.median(ms_p)), 1))
                ctx.buffer_free(out)
        d.free()


if __name__ == "__main__":
    main()
