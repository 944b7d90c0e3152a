"""Times dnagpu_table_from_text (the loader of a text file of sequences into a resident table) with the text
already in device memory, over three shapes of the same size:
  lines150   lines of 150 bases, one sequence per line
  one_line   one single line with no newline at all
  fasta      FASTA, records of 10,000 bases in lines 60 wide
then dnagpu_reads_from_text over lines150 again under the ERROR policy -- the cost of the general path -- and
over two shapes of real data at the same size:
  fastq150      FASTQ, reads of 150 bases, 1 in 50 with an N, policy DROP
  fasta_masked  FASTA 60 wide, about 5 % of the bases in runs of N of 100 to 50,000, about half lower case, SPLIT + FOLD_CASE
and, as the yardstick, dnagpu_dna_pack over the same number of bytes of bases in device memory (it reads the text once,
writes the words once and makes one read-back); and, as the path this replaces, the glue's dna_in per row on one host core
over a sample of the same 150-base lines.

usage: python tools/table_load_probe.py [--bytes N] [--reps N]      (default 2^28 bytes, 9 repetitions)
Prints one JSON line per measurement.  Times are host clocks around calls that wait for the device, after two warm-up calls;
`ms` is the median, `ms_best` the least, `per_pack` the ratio of the medians to the yardstick's.  The stage times are
dnagpu_last_phase_times of one more call with profiling on (events between the stages: that call is not among the timed)."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SEED = 0x7AB1E


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    fn()
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), min(ms)


def bases(rng, n):
    return np.frombuffer(b"ATCG", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]


def with_newlines(text, width):
    """text cut into lines of `width` bases: a newline behind every one (the last may be shorter)"""
    n = len(text)
    rows = (n + width - 1) // width
    out = np.full(rows * (width + 1), ord("\n"), dtype=np.uint8)
    pad = np.full(rows * width, ord("A"), dtype=np.uint8)
    pad[:n] = text
    out.reshape(rows, width + 1)[:, :width] = pad.reshape(rows, width)
    return out


def shapes(rng, n_bytes):
    lines = with_newlines(bases(rng, n_bytes * 150 // 151), 150)[:n_bytes]
    lines[-1] = ord("\n")
    yield "lines150", 1, lines
    yield "one_line", 1, bases(rng, n_bytes)
    record = 10_000
    body = with_newlines(bases(rng, record), 60)
    header = np.frombuffer(b">read 0000000 sampled N n\n", dtype=np.uint8)
    one = np.concatenate([header, body])
    fasta = np.tile(one, n_bytes // len(one) + 1)[:n_bytes].copy()
    fasta[-1] = ord("\n")
    yield "fasta", 2, fasta


def reads_shapes(rng, n_bytes):
    """(name, format, ambiguous, fold_case, text) of the shapes of real data, n_bytes each"""
    name = np.frombuffer(b"@read 0000000\n", dtype=np.uint8)
    width = len(name) + 151 + 2 + 151
    rows = n_bytes // width - 1
    m = np.empty((rows, width), dtype=np.uint8)
    m[:, :len(name)] = name
    m[:, len(name):len(name) + 150] = bases(rng, rows * 150).reshape(rows, 150)
    m[:, len(name) + 150:len(name) + 153] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    m[:, len(name) + 153:width - 1] = rng.integers(33, 127, (rows, 150), dtype=np.uint8)
    m[:, width - 1] = ord("\n")
    hit = np.arange(0, rows, 50)
    m[hit, len(name) + rng.integers(0, 150, len(hit))] = ord("N")
    last = np.concatenate([np.frombuffer(b"@", dtype=np.uint8), np.full(n_bytes - rows * width - width + len(name) - 2, ord("p"), np.uint8),
                           m[0, len(name) - 1:]])
    yield "fastq150", 3, 1, False, np.concatenate([m.reshape(-1), last])
    seq = bases(rng, n_bytes * 60 // 61)
    at = 0
    while at < len(seq):                              # about half in lower-case stretches
        a, b = int(rng.integers(1000, 100_000)), int(rng.integers(1000, 100_000))
        seq[at:at + a] |= 32
        at += a + b
    for at in rng.integers(0, len(seq), max(1, len(seq) // 20 // 25_000)):      # about 5 % in runs of N
        seq[at:at + int(rng.integers(100, 50_001))] = ord("N")
    fasta = np.concatenate([np.frombuffer(b">chr1 soft-masked\n", dtype=np.uint8), with_newlines(seq, 60)])[:n_bytes].copy()
    fasta[-1] = ord("\n")
    yield "fasta_masked", 2, 2, True, fasta


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    n_bytes, reps = arg("--bytes", 1 << 28), arg("--reps", 9)
    pkg = load_package()
    glue = importlib.import_module(pkg.__name__ + ".glue")
    rng = np.random.default_rng(SEED)
    with pkg.Context(0) as ctx:
        dev = ctx.buffer_alloc(n_bytes)

        def load(fmt):
            d, rep = ctx.table_from_text_device(dev, n_bytes, fmt)
            d.free()
            return rep

        ctx.upload_bytes(dev, bases(rng, n_bytes))
        pack_ms, pack_best = timed(lambda: ctx.pack_device(dev, n_bytes).free(), reps)
        emit(what="dnagpu_dna_pack", bytes=n_bytes, ms=pack_ms, ms_best=pack_best, gbytes_per_s=n_bytes / pack_ms / 1e6)
        sample = None
        for name, fmt, text in shapes(rng, n_bytes):
            ctx.upload_bytes(dev, text)
            rep = load(fmt)
            ms, best = timed(lambda: load(fmt), reps)
            ctx.set_profiling(True)
            load(fmt)
            stages = {k: round(v, 4) for k, v in ctx.last_phase_times()}
            ctx.set_profiling(False)
            emit(what="dnagpu_table_from_text", shape=name, bytes=n_bytes, records=rep.records, bases=rep.bases, ms=ms, ms_best=best,
                 gbytes_per_s=n_bytes / ms / 1e6, per_pack=ms / pack_ms, stages_ms=stages)
            if name == "lines150":
                sample = bytes(text[:151 * (1 << 18)])
                lines_ms, lines = ms, text

        def reads(fmt, amb, fold):
            d, rep = ctx.reads_from_text_device(dev, n_bytes, fmt, amb, fold)
            d.free()
            return rep

        general = [("lines150", 1, 0, False, lines)]
        for name, fmt, amb, fold, text in general + list(reads_shapes(rng, n_bytes)):
            assert len(text) == n_bytes, (name, len(text))
            ctx.upload_bytes(dev, text)
            rep = reads(fmt, amb, fold)
            ms, best = timed(lambda: reads(fmt, amb, fold), reps)
            ctx.set_profiling(True)
            reads(fmt, amb, fold)
            stages = {k: round(v, 4) for k, v in ctx.last_phase_times()}
            ctx.set_profiling(False)
            emit(what="dnagpu_reads_from_text", shape=name, bytes=n_bytes, records=rep.records, sequences=rep.sequences, bases=rep.bases,
                 ambiguous=rep.ambiguous, dropped=rep.dropped, ms=ms, ms_best=best, gbytes_per_s=n_bytes / ms / 1e6,
                 per_pack=ms / pack_ms, **({"per_table_from_text": ms / lines_ms} if name == "lines150" else {}), stages_ms=stages)
        ctx.buffer_free(dev)
    # the host path: dna_in per row, one core, on 2^18 of the same lines
    rows = sample.split(b"\n")[:-1]
    t0 = time.perf_counter()
    for r in rows:
        glue.lib().dna_free(glue.lib().dna_in(r))
    host_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for r in rows:
        pass
    loop_ms = (time.perf_counter() - t0) * 1e3
    emit(what="glue dna_in per row, one core", rows=len(rows), bytes=len(sample), ms=host_ms, python_loop_ms=loop_ms,
         mbytes_per_s=len(sample) / host_ms / 1e3)


if __name__ == "__main__":
    main()
