"""Times the names column of a table of reads (dnagpu_names_*, dnagpu_table_to_text_named) on one FASTQ text of
150-base reads named "r" + their decimal index that is resident in device memory, every call beside its yardstick:
  names load   dnagpu_names_from_text, beside dnagpu_quals_from_fastq on the same bytes (both sweep the text once and copy a
               column; the names are about a tenth of the qualities' bytes)
  named image  dnagpu_table_to_text_named + dnagpu_text_image_read of the whole FASTQ image and of the FASTA image in lines of
               60, beside dnagpu_table_to_text with the prefix "r" (the same names, so the same bytes, formed by the digit walk)
  numbered     the numbered images with the prefix "read", the shapes fastq150 / fasta150 of tools/table_export_probe.py
  take         dnagpu_names_take of every second read (ids in device memory)

usage: python tools/read_names_probe.py [--bases N] [--reps N]      (default 2^28 bases, 21 repetitions)
Prints one JSON line per measurement.  Times are host clocks around calls that wait for the device, after two warm-up calls;
`ms` is the median, `ms_best` / `ms_worst` the extremes of the repetitions, `gbytes_per_s` the named bytes over `ms`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SEED = 0x7A3E7
READ = 150


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
    return dict(ms=float(np.median(ms)), ms_best=min(ms), ms_worst=max(ms))


def fastq(rng, reads):
    """reads records "@r<index>\\n<150 bases>\\n+\\n<150 qualities>\\n" -> (the text, the bytes of all names)"""
    parts, name_bytes, lo = [], 0, 0
    while lo < reads:
        digits = len(str(lo))
        hi = min(reads, 10 ** digits)
        m, name = hi - lo, 1 + digits
        rec = 1 + name + 1 + READ + 1 + 2 + READ + 1
        t = np.empty((m, rec), dtype=np.uint8)
        t[:, 0], t[:, 1] = ord("@"), ord("r")
        ids = np.arange(lo, hi, dtype=np.int64)
        for k in range(digits):
            t[:, 1 + digits - k] = 48 + ids % 10
            ids //= 10
        at = 1 + name
        t[:, at] = 10
        t[:, at + 1:at + 1 + READ] = np.frombuffer(b"ATCG", dtype=np.uint8)[rng.integers(0, 4, size=(m, READ), dtype=np.uint8)]
        t[:, at + 1 + READ] = 10
        t[:, at + 2 + READ], t[:, at + 3 + READ] = ord("+"), 10
        t[:, at + 4 + READ:at + 4 + 2 * READ] = rng.integers(35, 74, size=(m, READ), dtype=np.uint8)
        t[:, rec - 1] = 10
        parts.append(t.reshape(-1))
        name_bytes += m * name
        lo = hi
    return np.concatenate(parts), name_bytes


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    n_bases, reps = arg("--bases", 1 << 28), arg("--reps", 21)
    reads = n_bases // READ
    bases = reads * READ
    pkg = load_package()
    text, name_bytes = fastq(np.random.default_rng(SEED), reads)
    size = int(text.size)
    with pkg.Context(0) as ctx:
        dev_text = ctx.buffer_alloc(size)
        ctx.upload_bytes(dev_text, text)
        del text
        u64s = lambda n: ctx.buffer_alloc(8 * max(n, 1))
        pos, src_rec, src_off = u64s(reads), u64s(reads), u64s(reads)
        out = ctx.buffer_alloc(size + 4 * reads + 4096)
        d, rep = ctx.reads_from_text_device(dev_text, size, pkg.TEXT_FASTQ, dev_record_pos=pos, record_cap=reads,
                                            dev_src_record=src_rec, dev_src_offset=src_off, seq_cap=reads)
        assert rep.sequences == reads and rep.records == reads and d.n_bases == bases

        # ---- 1. the names load beside the qualities load
        def staged(fn):
            ctx.set_profiling(True)
            fn()
            stages = {k: round(v, 4) for k, v in ctx.last_phase_times()}
            ctx.set_profiling(False)
            return stages

        def load_quals():
            ctx.quals_from_fastq_device(dev_text, size, d, src_rec, src_off)[0].free()

        def load_names(first_word=False):
            ctx.names_from_text_device(dev_text, size, pkg.TEXT_FASTQ, pos, reads, src_rec, reads, first_word=first_word).free()
        t = timed(load_quals, reps)
        emit(what="dnagpu_quals_from_fastq", reads=reads, text_bytes=size, column_bytes=bases, gbytes_per_s=size / t["ms"] / 1e6,
             stages_ms=staged(load_quals), **t)
        quals_ms = t["ms"]
        for fw in (False, True):
            t = timed(lambda: load_names(fw), reps)
            emit(what="dnagpu_names_from_text", first_word=fw, reads=reads, text_bytes=size, column_bytes=name_bytes,
                 gbytes_per_s=size / t["ms"] / 1e6, vs_quals=t["ms"] / quals_ms, stages_ms=staged(lambda: load_names(fw)), **t)
        names = ctx.names_from_text_device(dev_text, size, pkg.TEXT_FASTQ, pos, reads, src_rec, reads)
        assert names.n_sequences == reads and names.n_bytes == name_bytes
        assert names.read(0, 12) == b"r0r1r2r3r4r5"

        # ---- 2. the named image beside the numbered image of the same bytes; 3. the numbered shapes of table_export_probe.py
        def image(make, what, **kw):
            with make() as img:
                n = img.bytes
                assert n <= size + 4 * reads + 4096
                r = timed(lambda: img.read_device(0, n, out), reps)

            def whole():
                with make() as im:
                    im.read_device(0, n, out)
            w = timed(whole, reps)
            emit(what=what, image_bytes=n, ms=w["ms"], ms_best=w["ms_best"], ms_worst=w["ms_worst"], read_ms=r["ms"],
                 read_ms_best=r["ms_best"], read_ms_worst=r["ms_worst"], gbytes_per_s=n / w["ms"] / 1e6,
                 read_gbytes_per_s=n / r["ms"] / 1e6, **kw)
            return n
        for shape, fmt, width in (("fastq150", pkg.TEXT_FASTQ, 0), ("fasta150", pkg.TEXT_FASTA, 60)):
            a = image(lambda: ctx.table_to_text_named(d, names, fmt, line_width=width), "dnagpu_table_to_text_named", shape=shape)
            b = image(lambda: ctx.table_to_text(d, fmt, line_width=width, prefix=b"r"), "dnagpu_table_to_text", shape=shape, prefix="r")
            assert a == b
            image(lambda: ctx.table_to_text(d, fmt, line_width=width, prefix=b"read"), "dnagpu_table_to_text", shape=shape, prefix="read")
        with ctx.table_to_text_named(d, names, pkg.TEXT_FASTQ) as img, ctx.table_to_text(d, pkg.TEXT_FASTQ, prefix=b"r") as num:
            for first in (0, img.bytes // 2, img.bytes - 4096):          # the two images are the same bytes
                assert img.read(first, 4096) == num.read(first, 4096)

        # ---- take
        ids = np.arange(0, reads, 2, dtype=np.uint64)
        dev_ids = u64s(ids.size)
        ctx.upload_bytes(dev_ids, ids.view(np.uint8))
        t = timed(lambda: ctx.names_take(names, (dev_ids, int(ids.size)), on_device=True).free(), reps)
        emit(what="dnagpu_names_take of every second read", ids=int(ids.size), gbytes_per_s=name_bytes / 2 / t["ms"] / 1e6, **t)
        names.free()
        d.free()
        for p in (dev_text, pos, src_rec, src_off, out, dev_ids):
            ctx.buffer_free(p)


if __name__ == "__main__":
    main()
