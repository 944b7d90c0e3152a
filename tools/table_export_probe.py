"""Times dnagpu_table_to_text (a resident table written out as text): the plan plus the read of the WHOLE image
into a device buffer, over four images of the same number of bases:
  lines150   reads of 150 bases as one sequence per line
  fasta150   the same reads as FASTA in lines of 60
  fastq150   the same reads as FASTQ
  fasta_one  one sequence of all the bases as FASTA in lines of 60
and, as the yardstick, dnagpu_dna_unpack of the same bases into the same device buffer (it reads the words once and writes
one byte per base with the same whole 16-byte stores).

usage: python tools/table_export_probe.py [--bases N] [--reps N]      (default 2^28 bases, 21 repetitions)
Prints one JSON line per measurement.  Times are host clocks around calls that wait for the device, after two warm-up calls;
`ms` is the median of plan + read, `read_ms` the median of the read alone, `gbytes_per_s` the image's bytes over `ms`, and
`per_byte_vs_unpack` the time per output byte over unpack's time per output byte (read alone: `read_per_byte_vs_unpack`)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SEED = 0xE7907


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


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    n, reps = arg("--bases", 1 << 28), arg("--reps", 21)
    pkg = load_package()
    with pkg.Context(0) as ctx:
        d = ctx.synth(SEED, n)
        n_reads = n // 150
        starts = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(150)
        starts[-1] = n                                       # (the last read takes the rest)
        shapes = [("lines150", pkg.TEXT_LINES, 0, starts), ("fasta150", pkg.TEXT_FASTA, 60, starts),
                  ("fastq150", pkg.TEXT_FASTQ, 0, starts), ("fasta_one", pkg.TEXT_FASTA, 60, np.array([0, n], dtype=np.uint64))]
        cap = 2 * n + 32 * n_reads + 4096
        dev = ctx.buffer_alloc(cap)
        unpack_ms, unpack_best = timed(lambda: ctx.unpack_device(d, 0, n, dev), reps)
        emit(what="dnagpu_dna_unpack", bases=n, bytes=n, ms=unpack_ms, ms_best=unpack_best, gbytes_per_s=n / unpack_ms / 1e6)
        for name, fmt, width, st in shapes:
            d.set_sequences(st)
            with ctx.table_to_text(d, fmt, line_width=width, prefix=b"read") as img:
                size = img.bytes
                assert size <= cap
                read_ms, read_best = timed(lambda: img.read_device(0, size, dev), reps)

            def whole():
                with ctx.table_to_text(d, fmt, line_width=width, prefix=b"read") as im:
                    im.read_device(0, size, dev)
            ms, best = timed(whole, reps)
            ctx.set_profiling(True)
            ctx.table_to_text(d, fmt, line_width=width, prefix=b"read").free()
            stages = {k: round(v, 4) for k, v in ctx.last_phase_times()}
            ctx.set_profiling(False)
            emit(what="dnagpu_table_to_text", shape=name, sequences=len(st) - 1, bases=n, bytes=size, ms=ms, ms_best=best, read_ms=read_ms,
                 read_ms_best=read_best, gbytes_per_s=size / ms / 1e6, read_gbytes_per_s=size / read_ms / 1e6,
                 per_byte_vs_unpack=(ms / size) / (unpack_ms / n), read_per_byte_vs_unpack=(read_ms / size) / (unpack_ms / n),
                 plan_stages_ms=stages)
        ctx.buffer_free(dev)
        d.free()


if __name__ == "__main__":
    main()
