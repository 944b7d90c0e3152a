"""Times dnagpu_dna_take / dnagpu_dna_gather (sequences by id and stream segments gathered into a new resident table,
DESIGN.md 4.16) on a resident synthetic table -- seed 0xD2A0001, 10^9 bases as 10^7 reads of 100 bases by default -- with
the id lists already in device memory (what dnagpu_seq_hits_select leaves there):
  all ids       every read, in order: the output is the table
  every 32nd    one read in 32
  random 3 %    a sorted random sample: what survives a screen
  all flipped   every read, reverse-complemented
  one segment   dnagpu_dna_gather of ONE segment of all the table's bases from base 13 on: two source words per output word
  short ones    dnagpu_dna_gather of the first 10 bases of every read: three to four pieces per output word, and more
                segments to a tile of the sweep than it keeps in LDS (the other of its two forms)
Beside each, the time of a plain device-to-device hipMemcpy of the same number of OUTPUT bytes on the same device: the copy
is the yardstick the ratio is reported against (the gather also reads the starts and writes the result's starts and marks).

usage: python tools/take_probe.py [--reps N] [--bases N] [--read 100]
Per measurement one JSON line: host-clock ms per call (after one warm-up; both calls wait for their work), the ids, the output
bytes, the copy's ms, the ratio of the medians, and the device time of every stage of one further, profiled call."""
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
HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def hip_runtime():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            L = C.CDLL(name)
        except OSError:
            continue
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipDeviceSynchronize.argtypes = []
        return L
    raise ImportError("libamdhip64.so not found")


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    ap.add_argument("--read", type=int, default=100)
    a = ap.parse_args()
    pkg = load_package()
    hip = hip_runtime()
    n, read = a.bases, a.read
    n_reads = n // read
    n = n_reads * read
    slack = 64                                     # bases behind the reads, so that a segment of n bases fits at base 13
    starts = np.concatenate([np.arange(0, n + read, read, dtype=np.uint64), np.array([n + slack], dtype=np.uint64)])
    rng = np.random.default_rng(SEED)
    all_ids = np.arange(n_reads, dtype=np.uint64)
    cases = [("all ids", all_ids, False), ("every 32nd", all_ids[::32], False),
             ("random 3 %", np.sort(rng.choice(n_reads, max(n_reads * 3 // 100, 1), replace=False)).astype(np.uint64), False),
             ("all flipped", all_ids, True)]

    def report(**kw):
        print(json.dumps(kw), flush=True)

    with pkg.Context(0) as ctx:
        d = ctx.synth(SEED, n + slack)
        d.set_sequences(starts)
        out_bytes_max = 8 * ((n + 31) // 32)
        copy_src, copy_dst = ctx.buffer_alloc(out_bytes_max), ctx.buffer_alloc(out_bytes_max)
        dev_ids = ctx.buffer_alloc(8 * n_reads)
        dev_flip = ctx.buffer_alloc(n_reads)
        ctx.upload_bytes(dev_flip, np.ones(n_reads, dtype=np.uint8))
        dev_seg = ctx.buffer_alloc(16)
        ctx.upload_u64(dev_seg, np.array([13, n], dtype=np.uint64))

        def copy_ms(nbytes):
            def call():
                hip.hipMemcpy(copy_dst, copy_src, nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE)
                hip.hipDeviceSynchronize()
            return timed(call, a.reps)[0]

        def measure(form, name, n_ids, call):
            def run():
                t = call()
                got = (t.n_bases, t.n_sequences)
                t.free()
                return got
            ms, (bases, seqs) = timed(run, a.reps)
            nbytes = 8 * ((bases + 31) // 32)
            cms = copy_ms(nbytes)
            ctx.set_profiling(True)                # one more call, with an event between the stages: device ms per stage
            run()
            phases = {name: round(t, 4) for name, t in ctx.last_phase_times()}
            ctx.set_profiling(False)
            med, cmed = float(np.median(ms)), float(np.median(cms))
            report(form=form, case=name, ids=n_ids, out_bases=bases, out_sequences=seqs, out_bytes=nbytes, host_ms=ms, median_ms=med,
                   out_gb_per_s=round(nbytes / med / 1e6, 1), copy_ms=cms, copy_median_ms=cmed, ratio_to_copy=round(med / cmed, 3), phases_ms=phases)

        for name, ids, flipped in cases:
            ctx.upload_u64(dev_ids, ids)
            measure("dna_take", name, len(ids), lambda: ctx.dna_take_device(d, dev_ids, len(ids), dev_flip if flipped else None))
        measure("dna_gather", "one segment at base 13", 1, lambda: ctx.dna_gather_device(d, dev_seg, dev_seg + 8, 1))
        dev_len = ctx.buffer_alloc(8 * n_reads)
        ctx.upload_u64(dev_ids, all_ids * np.uint64(read))
        ctx.upload_u64(dev_len, np.full(n_reads, 10, dtype=np.uint64))
        measure("dna_gather", "the first 10 bases of every read", n_reads, lambda: ctx.dna_gather_device(d, dev_ids, dev_len, n_reads))
        for p in (copy_src, copy_dst, dev_ids, dev_flip, dev_seg, dev_len):
            ctx.buffer_free(p)
        d.free()


if __name__ == "__main__":
    main()
