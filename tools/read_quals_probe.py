"""Times the quality column of a table of reads (dnagpu_quals_*) on one FASTQ text of 150-base reads that
is resident in device memory, every call beside the yardstick it is bounded by:
  load        dnagpu_quals_from_fastq, beside dnagpu_reads_from_text on the same bytes
  gather      dnagpu_quals_gather of every read (the segment list dnagpu_quals_trim wrote, in device memory) and
  trim        dnagpu_quals_trim (cut_front = cut_tail = 20, min_bases = 30, every output in device memory), both beside a
              device-to-device copy of the column's bytes: the floor of a pass that reads one byte per base
  write back  dnagpu_text_image_read_quals of the whole image, beside dnagpu_text_image_read of the same image

usage: python tools/read_quals_probe.py [--bytes N] [--reps N]      (default 2^28 bytes of text, 21 repetitions)
Prints one JSON line per measurement.  Times are host clocks around calls that wait for the device, after two warm-up calls;
`ms` is the median, `ms_best` the minimum, `gbytes_per_s` the named bytes over `ms`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SEED = 0x9A157
READ = 150
NAME = 9                                                     # "@r" + 6 base-36 digits + "\n"
RECORD = NAME + READ + 1 + 2 + READ + 1


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


def fastq(rng, reads):
    """reads records of RECORD bytes each: good qualities in the middle of a read, worse ones towards its ends"""
    t = np.empty((reads, RECORD), dtype=np.uint8)
    t[:, 0], t[:, 1] = ord("@"), ord("r")
    ids = np.arange(reads, dtype=np.int64)
    digits = np.frombuffer(b"0123456789abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    for k in range(6):
        t[:, 2 + 5 - k] = digits[ids % 36]
        ids //= 36
    t[:, NAME - 1] = 10
    t[:, NAME:NAME + READ] = np.frombuffer(b"ATCG", dtype=np.uint8)[rng.integers(0, 4, size=(reads, READ), dtype=np.uint8)]
    t[:, NAME + READ] = 10
    t[:, NAME + READ + 1], t[:, NAME + READ + 2] = ord("+"), 10
    ramp = np.minimum(np.arange(READ), np.arange(READ)[::-1])
    mean = np.minimum(12 + 2 * ramp, 36)
    q = mean[None, :] + rng.integers(-10, 6, size=(reads, READ))
    t[:, NAME + READ + 3:NAME + READ + 3 + READ] = 33 + np.clip(q, 2, 41)
    t[:, RECORD - 1] = 10
    return t.reshape(-1)


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    n_bytes, reps = arg("--bytes", 1 << 28), arg("--reps", 21)
    reads = n_bytes // RECORD
    size = reads * RECORD
    bases = reads * READ
    pkg = load_package()
    text = fastq(np.random.default_rng(SEED), reads)
    with pkg.Context(0) as ctx:
        dev_text = ctx.buffer_alloc(size)
        ctx.upload_bytes(dev_text, text)
        del text
        u64s = lambda n: ctx.buffer_alloc(8 * max(n, 1))
        src_rec, src_off = u64s(reads), u64s(reads)
        per, seg = [u64s(reads) for _ in range(4)], [u64s(reads) for _ in range(3)]
        out = ctx.buffer_alloc(size + 4096)

        def load_table():
            d, _ = ctx.reads_from_text_device(dev_text, size, pkg.TEXT_FASTQ, dev_src_record=src_rec, dev_src_offset=src_off, seq_cap=reads)
            d.free()
        ms, best = timed(load_table, reps)
        emit(what="dnagpu_reads_from_text", reads=reads, text_bytes=size, ms=ms, ms_best=best, gbytes_per_s=size / ms / 1e6)
        d, rep = ctx.reads_from_text_device(dev_text, size, pkg.TEXT_FASTQ, dev_src_record=src_rec, dev_src_offset=src_off, seq_cap=reads)
        assert rep.sequences == reads and d.n_bases == bases

        def load_quals():
            ctx.quals_from_fastq_device(dev_text, size, d, src_rec, src_off)[0].free()
        ms, best = timed(load_quals, reps)
        ctx.set_profiling(True)
        load_quals()
        stages = {k: round(v, 4) for k, v in ctx.last_phase_times()}
        ctx.set_profiling(False)
        emit(what="dnagpu_quals_from_fastq", reads=reads, text_bytes=size, column_bytes=bases, ms=ms, ms_best=best,
             gbytes_per_s=size / ms / 1e6, stages_ms=stages)
        q, _ = ctx.quals_from_fastq_device(dev_text, size, d, src_rec, src_off)

        copy_ms, copy_best = timed(lambda: q.read_device(0, bases, out), reps)
        emit(what="device-to-device copy of the column", column_bytes=bases, ms=copy_ms, ms_best=copy_best,
             gbytes_per_s=bases / copy_ms / 1e6)

        opt = dict(cut_front=20, cut_tail=20, min_bases=30)
        ms, best = timed(lambda: ctx.quals_trim_device(d, q, opt, per, seg, reads), reps)
        r = ctx.quals_trim_device(d, q, opt, per, seg, reads)
        emit(what="dnagpu_quals_trim", reads=reads, column_bytes=bases, passed=r.passed, bases_kept=r.bases_kept, ms=ms, ms_best=best,
             gbytes_per_s=bases / ms / 1e6, vs_copy=ms / copy_ms)

        def gather(m):
            ctx.quals_gather(q, (seg[1], m), seg[2], None, on_device=True).free()
        ms, best = timed(lambda: gather(r.passed), reps)
        emit(what="dnagpu_quals_gather of the trimmed reads", segments=r.passed, bytes_out=r.bases_kept, ms=ms, ms_best=best,
             gbytes_per_s=r.bases_kept / ms / 1e6, vs_copy=ms / copy_ms)
        plain = ctx.quals_trim_device(d, q, {}, per, seg, reads)
        assert plain.passed == reads and plain.bases_kept == bases
        ms, best = timed(lambda: gather(reads), reps)
        emit(what="dnagpu_quals_gather of every read, whole", segments=reads, bytes_out=bases, ms=ms, ms_best=best,
             gbytes_per_s=bases / ms / 1e6, vs_copy=ms / copy_ms)

        with ctx.table_to_text(d, pkg.TEXT_FASTQ, prefix=b"r") as img:
            image = img.bytes
            assert image <= size + 4096
            read_ms, read_best = timed(lambda: img.read_device(0, image, out), reps)
            emit(what="dnagpu_text_image_read", image_bytes=image, ms=read_ms, ms_best=read_best, gbytes_per_s=image / read_ms / 1e6)
            ms, best = timed(lambda: img.read_quals_device(q, 0, image, out), reps)
            emit(what="dnagpu_text_image_read_quals", image_bytes=image, ms=ms, ms_best=best, gbytes_per_s=image / ms / 1e6,
                 vs_read=ms / read_ms)
        q.free()
        d.free()
        for p in [dev_text, src_rec, src_off, out] + per + seg:
            ctx.buffer_free(p)


if __name__ == "__main__":
    main()
