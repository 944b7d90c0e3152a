"""Times the index over a stored kmer column (dnagpu_kmer_index_*) against the sequential scan it replaces:
the build, and the three queries of test.sql:188-262 (`= 'ATCGC'`, `^@ 'ACTG'`, `'MRKYN' @>`) as index scans, each beside
dnagpu_kmer_match over the same device-resident column plus the host compaction of its flags (download n bytes,
np.flatnonzero) -- what a caller had to do for row ids before.  Shapes: n = 10^6 rows at k = 5 (test.sql's own), and the same
queries at n = 10^8, k = 31 (the prefix and the pattern padded with N's; `=` asks for a key of the column).

Updates: an append of m rows to an index of n (dnagpu_kmer_index_append) and a delete of m listed row ids from it
(dnagpu_kmer_index_delete), each beside dnagpu_kmer_index_build of the n + m rows in the same run: m = 10^4 at n = 10^6, k = 5;
m = 10^4, 10^6 and 10^7 at n = 10^8, k = 31.  The appended index is compared with that build (rows, distinct, windows of
the index order).

usage: python tools/kmer_index_probe.py [--reps N] [--small-only] [--updates-only] [--out FILE]
Every answer is checked: the index's row ids, sorted, must equal the flags' positions.  Times are medians of --reps repeats
after one warm-up of the same shapes: host clocks in ms around calls that end in a read-back, and for the library's own calls
the device time between HIP events on the context's stream (dnagpu_set_profiling).  Prints one JSON line per shape and, with
--out, writes them to a file."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle as orc  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def med(xs):
    return round(statistics.median(xs), 4)


def probe(pkg, ctx, n, k, reps):
    nb = n + k - 1
    dna = ctx.synth(0x1DE5 + k, nb)
    dev_col = ctx.buffer_alloc(8 * n)
    ctx.generate_kmers_device(dna, k, 0, n, dev_col)
    dna.free()
    dev_flags = ctx.buffer_alloc(n)
    present = int(ctx.download_u64(dev_col + 8 * (n // 3), 1)[0])
    pad = "N" * (k - 5)
    queries = {
        "eq": pkg.Filter.equals(*orc.kmer_encode("ATCGC")) if k == 5 else pkg.Filter.equals(k, present),
        "starts_with_ACTG": pkg.Filter.starts_with(*orc.kmer_encode("ACTG")),
        "contains_MRKYN": pkg.Filter.contains("MRKYN" + pad),
    }
    ctx.set_profiling(True)
    # build: warm-up + reps
    build_host, build_dev, pass_dev, passes = [], [], [], 0
    idx = None
    for r in range(reps + 1):
        if idx is not None:
            idx.free()
        t, idx = timed(lambda: ctx.kmer_index_device(dev_col, n, k))
        ph = ctx.last_phase_times()
        if r:
            build_host.append(t)
            build_dev.append(sum(ms for _, ms in ph))
            pass_dev.append(sum(ms for name, ms in ph if name == "index_pass"))
    passes = (2 * k + 7) // 8
    out = {"probe": "kmer_index", "n": n, "k": k, "reps": reps, "distinct": idx.distinct,
           "build": {"host_ms": med(build_host), "device_ms": med(build_dev), "passes_device_ms": med(pass_dev), "passes": passes,
                     # the plan of DESIGN.md 4.12: 32 bytes per row and pass (8 histogram, 12 read + 12 written by the scatter)
                     "planned_bytes": 32 * n * passes,
                     "planned_bytes_over_passes_time_GBs": round(32 * n * passes / (med(pass_dev) * 1e6), 1)},
           "queries": {}}
    for name, flt in queries.items():
        ix_host, ix_dev, seq_match, seq_total = [], [], [], []
        rows = visited = flags_pos = None
        for r in range(reps + 1):
            t, (rows, _, n_out, visited) = timed(lambda: idx.scan(flt, want_keys=False))
            ph = ctx.last_phase_times()
            if r:
                ix_host.append(t)
                ix_dev.append(sum(ms for _, ms in ph))
            t1, _ = timed(lambda: ctx.kmer_match_device(dev_col, n, k, flt, dev_flags))
            t2, flags_pos = timed(lambda: np.flatnonzero(ctx.download_bytes(dev_flags, n)))
            if r:
                seq_match.append(t1)
                seq_total.append(t1 + t2)
        assert np.array_equal(np.sort(rows), flags_pos.astype(np.uint64)), name
        out["queries"][name] = {"rows": int(n_out), "visited": int(visited),
                                "index_scan_host_ms": med(ix_host), "index_scan_device_ms": med(ix_dev),
                                "seq_scan_match_ms": med(seq_match), "seq_scan_with_host_compaction_ms": med(seq_total),
                                "answers_equal": True}
    idx.free()
    ctx.buffer_free(dev_col)
    ctx.buffer_free(dev_flags)
    ctx.trim()
    return out


def phases(ctx):
    ph = ctx.last_phase_times()
    return sum(ms for _, ms in ph), {name: ms for name, ms in ph}


def probe_updates(pkg, ctx, n, k, ms, reps):
    """append of m rows to n / delete of m ids from n, beside the build of n + m rows; device keys and ids throughout"""
    m_max = max(ms)
    nb = n + m_max + k - 1
    dna = ctx.synth(0x1DE5 + k, nb)
    dev_col = ctx.buffer_alloc(8 * (n + m_max))
    ctx.generate_kmers_device(dna, k, 0, n + m_max, dev_col)
    dna.free()
    ctx.set_profiling(True)
    rng = np.random.default_rng(n + k)
    out = []
    for m in ms:
        ids = rng.integers(0, n, m, dtype=np.uint64)              # repeats are ignored by the delete: n_deleted is reported
        dev_ids = ctx.buffer_alloc(8 * m)
        ctx.upload_u64(dev_ids, ids)
        listed = len(np.unique(ids))
        t = {x: [] for x in ("build_host", "build_dev", "append_host", "append_dev", "delete_host", "delete_dev")}
        parts = {"append": {}, "delete": {}}
        n_deleted = 0
        for r in range(reps + 1):
            th, fresh = timed(lambda: ctx.kmer_index_device(dev_col, n + m, k))
            td, _ = phases(ctx)
            idx = ctx.kmer_index_device(dev_col, n, k)
            ta, _ = timed(lambda: idx.append((dev_col + 8 * n, m), on_device=True))
            tad, pa = phases(ctx)
            if r == 0:                                            # the appended index is the build of the n + m rows
                assert (idx.rows, idx.distinct, idx.next_row) == (fresh.rows, fresh.distinct, n + m)
                for first in (0, (n + m) // 2, n + m - min(n + m, 100_000)):
                    a, b = idx.read(first, min(n + m, 100_000)), fresh.read(first, min(n + m, 100_000))
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (m, first)
            idx.free()
            fresh.free()
            idx = ctx.kmer_index_device(dev_col, n, k)
            tdl, n_deleted = timed(lambda: idx.delete((dev_ids, m), on_device=True))
            tdd, pd = phases(ctx)
            assert n_deleted == listed and idx.rows == n - n_deleted
            idx.free()
            if r:
                for name, v in (("build_host", th), ("build_dev", td), ("append_host", ta), ("append_dev", tad),
                                ("delete_host", tdl), ("delete_dev", tdd)):
                    t[name].append(v)
                for what, ph in (("append", pa), ("delete", pd)):
                    for name, v in ph.items():
                        parts[what].setdefault(name, []).append(v)
        ctx.buffer_free(dev_ids)
        total = n + m
        out.append({
            "m": m,
            "build_n_plus_m": {"host_ms": med(t["build_host"]), "device_ms": med(t["build_dev"])},
            "append": {"host_ms": med(t["append_host"]), "device_ms": med(t["append_dev"]),
                       "phases_device_ms": {name: med(v) for name, v in parts["append"].items()},
                       # the plan of DESIGN.md 4.12: the merge reads and writes 12 bytes per row of the result
                       "planned_merge_bytes": 24 * total, "equals_the_build": True},
            "delete": {"host_ms": med(t["delete_host"]), "device_ms": med(t["delete_dev"]), "n_deleted": int(n_deleted),
                       "phases_device_ms": {name: med(v) for name, v in parts["delete"].items()}},
        })
    ctx.buffer_free(dev_col)
    ctx.trim()
    return out


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    shapes = [(10 ** 6, 5)] + ([] if "--small-only" in args else [(10 ** 8, 31)])
    pkg = load_package()
    results = []
    with pkg.Context(0) as ctx:
        for n, k in shapes:
            res = {"probe": "kmer_index", "n": n, "k": k, "reps": reps} if "--updates-only" in args else probe(pkg, ctx, n, k, reps)
            res["updates"] = probe_updates(pkg, ctx, n, k, [10 ** 4] if n == 10 ** 6 else [10 ** 4, 10 ** 6, 10 ** 7], reps)
            print(json.dumps(res), flush=True)
            results.append(res)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
