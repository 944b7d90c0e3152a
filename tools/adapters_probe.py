"""Times dnagpu_dna_adapters on the resident table of tools/read_quals_probe.py -- one FASTQ text of 150-base
reads -- with an adapter read-through planted into half the reads (the adapter's head at a random position, clipped by the
read's end, 0 .. 2 letters substituted), beside its two yardsticks from the same run:
  trim        dnagpu_quals_trim on the same table (cut_front = cut_tail = 20, min_bases = 30, outputs in device memory)
  copy        a device-to-device copy of as many bytes as the packed stream holds (a quarter byte per base): the floor of a
              pass that reads the stream once
Cases: one adapter and eight adapters; rate 1/10, min_overlap 3; the segments are the table's sequences; every output in
device memory.

usage: python tools/adapters_probe.py [--bytes N] [--reps N]      (default 2^28 bytes of text, 21 repetitions)
Prints one JSON line per measurement.  Times are host clocks around calls that wait for the device, after two warm-up calls;
`ms` is the median, `ms_best` the minimum."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from __graft_entry__ import load_package  # noqa: E402
from read_quals_probe import NAME, READ, RECORD, SEED, emit, fastq, timed  # noqa: E402

ADAPTERS = ["AGATCGGAAGAGCACACGTCTGAACTCCAGTC", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTG", "CTGTCTCTTATACACATCTCCGAGCCCACGAG",
            "CTGTCTCTTATACACATCTGACGCTGCCGACG", "TGGAATTCTCGGGTGCCAAGGAACTCCAGTCA", "GATCGTCGGACTGTAGAACTCTGAAC",
            "AATGATACGGCGACCACCGAGATCTACAC", "CAAGCAGAAGACGGCATACGAGAT"]


def plant(rng, text, reads):
    """the head of ADAPTERS[0] into every second read, from a random position to the read's end at the most"""
    t = text.reshape(reads, RECORD)
    ad = np.frombuffer(ADAPTERS[0].encode(), dtype=np.uint8)
    rows = np.arange(0, reads, 2)
    at = rng.integers(0, READ, size=len(rows))
    k = np.arange(READ)[None, :] - at[:, None]
    inside = (k >= 0) & (k < len(ad))
    seqs = t[rows, NAME:NAME + READ]
    seqs[inside] = ad[k[inside]]
    n = np.minimum(len(ad), READ - at)
    subs = rng.integers(0, 3, size=len(rows))
    for j in range(2):
        do = np.flatnonzero(subs > j)
        seqs[do, at[do] + rng.integers(0, 1 << 30, size=len(do)) % n[do]] = ord("A")
    t[rows, NAME:NAME + READ] = seqs
    return t.reshape(-1)


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    n_bytes, reps = arg("--bytes", 1 << 28), arg("--reps", 21)
    reads = n_bytes // RECORD
    size, bases = reads * RECORD, reads * READ
    pkg = load_package()
    rng = np.random.default_rng(SEED)
    text = plant(rng, fastq(rng, reads), reads)
    with pkg.Context(0) as ctx:
        dev_text = ctx.buffer_alloc(size)
        ctx.upload_bytes(dev_text, text)
        del text
        u64s = lambda n: ctx.buffer_alloc(8 * max(n, 1))
        src_rec, src_off = u64s(reads), u64s(reads)
        per, seg = [u64s(reads) for _ in range(4)], [u64s(reads) for _ in range(3)]
        out = ctx.buffer_alloc(bases // 4 + 4096)
        d, rep = ctx.reads_from_text_device(dev_text, size, pkg.TEXT_FASTQ, dev_src_record=src_rec, dev_src_offset=src_off, seq_cap=reads)
        assert rep.sequences == reads and d.n_bases == bases
        q, _ = ctx.quals_from_fastq_device(dev_text, size, d, src_rec, src_off)

        copy_ms, copy_best = timed(lambda: q.read_device(0, bases // 4, out), reps)
        emit(what="device-to-device copy of the packed stream's size", bytes=bases // 4, ms=copy_ms, ms_best=copy_best,
             gbytes_per_s=bases / 4 / copy_ms / 1e6)
        opt = dict(cut_front=20, cut_tail=20, min_bases=30)
        trim_ms, trim_best = timed(lambda: ctx.quals_trim_device(d, q, opt, per, seg, reads), reps)
        emit(what="dnagpu_quals_trim", reads=reads, column_bytes=bases, ms=trim_ms, ms_best=trim_best, vs_copy=trim_ms / copy_ms)

        for n_ad in (1, 8):
            ads = ADAPTERS[:n_ad]
            call = lambda: ctx.dna_adapters_device(d, ads, reads, (None,) * 3, 1, per[:3], seg, reads, 1, err=(1, 10), min_overlap=3,
                                                   min_bases=30)
            ms, best = timed(call, reps)
            r = call()
            ctx.set_profiling(True)
            call()
            stages = {k: round(v, 4) for k, v in ctx.last_phase_times()}
            ctx.set_profiling(False)
            emit(what="dnagpu_dna_adapters", adapters=n_ad, reads=reads, bases=bases, trimmed=r.trimmed, passed=r.passed,
                 bases_cut=r.bases_cut, per_adapter=r.per_adapter[:n_ad], ms=ms, ms_best=best, gbases_per_s=bases / ms / 1e6,
                 vs_quals_trim=ms / trim_ms, vs_copy=ms / copy_ms, stages_ms=stages)
        q.free()
        d.free()
        for p in [dev_text, src_rec, src_off, out] + per + seg:
            ctx.buffer_free(p)


if __name__ == "__main__":
    main()
