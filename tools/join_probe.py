"""Times dnagpu_acc_join (the hash join of two accumulators) on both of its paths, each forced with its debug
flag, over size ratios right / left of 1/256, 1/16, 1, 4, 16, 64 and 256 -- the smallest right sides stay in L2 -- then 2, 4
and 8 at larger sizes around the crossover, and, for one size, the way without it: two dnagpu_acc_download calls plus a join on the host.

usage: python tools/join_probe.py [--reps N] [--small]      (--small: every side 16 times shorter, a quick check)
Prints one JSON line per measurement: the partitions of both sides, the path, the best and median time of the
statistics-only INNER call and of the call that also stores the rows in device arrays, the byte estimate of the path and the
rate that estimate gives at the best time.  Times are host clocks around calls that wait for the device, after one warm-up.
  partition path: 2 * 2^max(s, t) * 64 KB
  direct path:    left's table once + one 64-byte sector per left group"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

K = 31
SEED = 0x10B0 << 32
PART_BYTES = 4096 * 16
# (left bases, right bases): about one group per base at k = 31
PAIRS = [(64_000_000, 250_000), (16_000_000, 1_000_000), (4_000_000, 4_000_000), (1_000_000, 4_000_000),
         (1_000_000, 16_000_000), (1_000_000, 64_000_000), (250_000, 64_000_000),
         # around the crossover, at sizes where a launch's fixed cost is small: t - s = 1, 2, 3
         (8_000_000, 16_000_000), (8_000_000, 32_000_000), (4_000_000, 32_000_000)]
HOST_PAIR = (1_000_000, 4_000_000)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), float(np.median(ms))


def make_acc(ctx, seed, n):
    d = ctx.synth(seed, n)
    h = ctx.count_kmers_unordered(d, K)
    d.free()
    a = ctx.accumulator(K)
    a.add(h)
    h.free()
    return a


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    shrink = 16 if "--small" in sys.argv else 1
    pkg = load_package()
    with pkg.Context(0) as ctx:
        made = {}

        def acc(seed, n):
            if (seed, n) not in made:
                made[(seed, n)] = make_acc(ctx, seed, n)
            return made[(seed, n)]

        for nl, nr in PAIRS:
            nl, nr = nl // shrink, nr // shrink
            # the right sequence starts inside the left one: the two sides share a long stretch
            left, right = acc(SEED, nl), acc(SEED + min(nl, nr) // 64, nr)
            s, t = left.partitions.bit_length() - 1, right.partitions.bit_length() - 1
            est = {"partition": 2 * (1 << max(s, t)) * PART_BYTES, "direct": left.partitions * PART_BYTES + 64 * left.distinct}
            want = None
            for name, flag in (("partition", pkg.DEBUG_JOIN_PARTITION), ("direct", pkg.DEBUG_JOIN_DIRECT)):
                ctx.set_debug(flag)
                st = left.join(right, pkg.JOIN_INNER, want_rows=False)[3].as_tuple()
                want = want or st
                assert st == want, (name, st, want)
                best, med = timed(lambda: left.join(right, pkg.JOIN_INNER, want_rows=False), reps)
                bufs = tuple(ctx.buffer_alloc(8 * max(st[0], 1)) for _ in range(3))
                rbest, rmed = timed(lambda: left.join(right, pkg.JOIN_INNER, cap=st[0], on_device=True, out=bufs), reps)
                for p in bufs:
                    ctx.buffer_free(p)
                ctx.set_debug(0)
                emit(probe="join", ratio=f"{nr}/{nl}", left_groups=left.distinct, right_groups=right.distinct, s=s, t=t,
                     path=name, rows=st[0], stats_ms=round(best, 4), stats_median_ms=round(med, 4), rows_ms=round(rbest, 4),
                     rows_median_ms=round(rmed, 4), estimate_bytes=est[name], rate_gb_s=round(est[name] / best / 1e6, 1))
            if (nl * shrink, nr * shrink) == HOST_PAIR:
                def host_join():
                    lk, lc = left.download()
                    rk, rc = right.download()
                    _, il, ir = np.intersect1d(lk, rk, assume_unique=True, return_indices=True)
                    return len(il), int(np.minimum(lc[il], rc[ir]).sum())
                assert host_join()[0] == want[0]
                t0 = time.perf_counter()
                lk, lc = left.download()
                rk, rc = right.download()
                t_down = (time.perf_counter() - t0) * 1e3
                best, med = timed(host_join, max(reps // 2, 1))
                emit(probe="download_and_host_join", ratio=f"{nr}/{nl}", rows=want[0], downloads_ms=round(t_down, 3),
                     total_ms=round(best, 3), total_median_ms=round(med, 3), bytes_over_the_bus=16 * (len(lk) + len(rk)))
            if nl * shrink >= 16_000_000 or nr * shrink >= 16_000_000:      # the large tables go back before the next pair
                for key in [x for x in made if x[1] * shrink >= 16_000_000]:
                    made.pop(key).free()
                ctx.trim()
        for a in made.values():
            a.free()


if __name__ == "__main__":
    main()
