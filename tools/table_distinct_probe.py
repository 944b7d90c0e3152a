"""Times dnagpu_table_classes (the classes of equal sequences of a table) and dnagpu_table_match of the table
against itself on a resident synthetic table: n reads of L bases of which a share d are copies of earlier reads (seed
0xD2A0001; 10^7 x 150 and d = 0.3 by default).  The table is made on the device: a synthetic stream cut into reads, then
dnagpu_dna_take with ids that repeat.  Per step one JSON line:
  build   host-clock ms of the whole call and device ms per stage (fingerprint, sort, verify, copies) from the context's
          phase times, with distinct and rounds
  match   host-clock ms of the match of the table against itself, device output
Beside each, in the same process, the time of dnagpu_kmer_index_build over n device keys at k = 32: the same stable LSD sort
of (64-bit key, 32-bit id) pairs, and the only comparable thing the library had before.

Each GPU step runs in a child process of its own under `timeout`; the first step that fails ends the run.

usage: python tools/table_distinct_probe.py [--reads N] [--length L] [--copies D] [--reps N] [--step-seconds S]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0xD2A0001
STEPS = ("build", "match")
STAGES = {"seqeq_fingerprint": "fingerprint", "seqeq_sort": "sort", "seqeq_verify": "verify", "seqeq_copies": "copies"}


def timed(fn, reps):
    ms, out = [], None
    for r in range(reps + 1):                      # (rep 0: warm-up)
        t0 = time.perf_counter()
        out = fn()
        t = (time.perf_counter() - t0) * 1e3
        if r:
            ms.append(round(t, 3))
    return ms, out


def make_table(ctx, n, length, share):
    """-> (Dna with n sequences of `length` bases, the number of distinct contents expected)"""
    rng = np.random.default_rng(SEED)
    ids = np.arange(n, dtype=np.uint64)
    is_copy = rng.random(n) < share
    is_copy[0] = False
    originals = np.flatnonzero(~is_copy)
    # a copy repeats an original that comes before it
    pick = (rng.random(int(is_copy.sum())) * np.searchsorted(originals, np.flatnonzero(is_copy))).astype(np.int64)
    ids[is_copy] = originals[pick]
    src = ctx.synth(SEED, n * length)
    try:
        src.set_sequences(np.arange(0, (n + 1) * length, length, dtype=np.uint64))
        return ctx.dna_take(src, ids), len(originals)
    finally:
        src.free()


def index_build_ms(ctx, n, reps):
    """dnagpu_kmer_index_build over n device keys at k = 32"""
    d = ctx.synth(SEED + 1, n + 31)
    keys = ctx.buffer_alloc(8 * n)
    try:
        ctx.generate_kmers_device(d, 32, 0, n, keys)

        def build():
            ctx.kmer_index_device(keys, n, 32).free()
        return timed(build, reps)[0]
    finally:
        ctx.buffer_free(keys)
        d.free()


def run_step(step, a):
    from __graft_entry__ import load_package
    pkg = load_package()
    n = a.reads
    with pkg.Context(0) as ctx:
        table, originals = make_table(ctx, n, a.length, a.copies)
        common = dict(step=step, reads=n, length=a.length, copies_share=a.copies)
        try:
            if step == "build":
                ctx.set_profiling(True)
                stages = {}

                def build():
                    with ctx.table_classes(table) as c:
                        stages.clear()
                        for name, ms in ctx.last_phase_times():
                            if name in STAGES:
                                stages[STAGES[name]] = round(stages.get(STAGES[name], 0.0) + ms, 3)
                        return c.distinct, c.rounds
                ms, (distinct, rounds) = timed(build, a.reps)
                ctx.set_profiling(False)
                # (random reads of this length do not collide: the distinct contents are the originals)
                print(json.dumps(dict(host_ms=ms, median_ms=float(np.median(ms)), stage_ms=stages, distinct=distinct,
                                      expected_distinct=originals, rounds=rounds, **common)), flush=True)
            else:
                out = [ctx.buffer_alloc(8 * n) for _ in range(2)]
                try:
                    with ctx.table_classes(table) as c:
                        ms, matched = timed(lambda: c.match(table, on_device=True, out=out), a.reps)
                    print(json.dumps(dict(host_ms=ms, median_ms=float(np.median(ms)), matched=matched, **common)), flush=True)
                finally:
                    for b in out:
                        ctx.buffer_free(b)
            ims = index_build_ms(ctx, n, a.reps)
            print(json.dumps(dict(step=step, form="kmer_index_build over n device keys, k = 32", keys=n, host_ms=ims,
                                  median_ms=float(np.median(ims)))), flush=True)
        finally:
            table.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--copies", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of each GPU step")
    ap.add_argument("--step", choices=STEPS, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.reads * a.length > 0xFFFFFFFF:
        sys.exit("a resident table holds at most 2^32 - 1 bases")
    if a.step:
        run_step(a.step, a)
        return
    for step in STEPS:                             # this process never opens the GPU
        cmd = ["timeout", "-k", "10", str(a.step_seconds), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reads", str(a.reads), "--length", str(a.length), "--copies", str(a.copies), "--reps", str(a.reps)]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit(f"step {step} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
