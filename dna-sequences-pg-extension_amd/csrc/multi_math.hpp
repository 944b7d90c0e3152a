// multi_math.hpp -- the arithmetic of the multi-GPU counts, shared by the host driver (multi_host.hip) and the
// host check tests/host/multi_plan_check.cpp: the rows of a rank's chunk, the bucket plan of the record exchange, and the
// layout of a bucket group's landing buffer.  Pure host code: no HIP call, no context.  The bucket plan is the rule of
// shard_math.py (bucket_owner_ranges_weighted, then bucket_group_cuts on every owner's range), which the process-per-GPU
// path uses; tests/test_sharded.py::test_exchange_plan_matches_shard_math holds the two together.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dnagpu {

typedef uint32_t u32;       // (as in kmer_device.hpp)
typedef uint64_t u64;

// Rank r is resident with words [r * per, (r + 1) * per) of the n_words packed words and sweeps the rows of
// [first, first + count) that START there: [row_lo, row_hi), empty when row_hi <= row_lo.  A row reaches at most k - 1 <= 31
// bases into the next chunk: one word, w_hi, the neighbour's first -- needed (halo) when the rank has rows and its chunk
// ends before the sequence does (then r + 1 is a rank: per * ranks >= n_words).
struct RankRows {
    u64 w_hi, row_lo, row_hi;
    bool halo;
    u64 n() const { return row_hi > row_lo ? row_hi - row_lo : 0; }
};
inline RankRows rank_rows(u64 n_words, u64 per, int r, u64 first, u64 count)
{
    const u64 w_lo = std::min((u64)r * per, n_words), w_hi = std::min((u64)(r + 1) * per, n_words);
    RankRows rr;
    rr.w_hi = w_hi;
    rr.row_lo = std::max<u64>(first, w_lo * 32);
    rr.row_hi = std::min<u64>(first + count, w_hi * 32);
    rr.halo = w_hi < n_words && rr.row_hi > rr.row_lo;
    return rr;
}

// Buckets [lo, hi) cut into `ways` consecutive parts whose weights stand as 1 : grow : grow^2 ...: out[0] = lo,
// out[ways] = hi, and part j ends where the running weight comes closest to its share of the whole -- a bucket goes to the
// side its middle falls on.  The arithmetic is double on purpose: shard_math.py computes the same targets.
inline void weighted_cuts(const std::vector<u64> &wgt, u32 lo, u32 hi, int ways, double grow, u32 *out)
{
    u64 tot = 0;
    for (u32 b = lo; b < hi; b++)
        tot += wgt[b];
    double wsum = 0, acc = 0, wp = 1;
    for (int j = 0; j < ways; j++, wp *= grow)
        wsum += wp;
    out[0] = lo;
    out[ways] = hi;
    u64 run = 0;
    u32 b = lo;
    wp = 1;
    for (int j = 1; j < ways; j++, wp *= grow) {
        acc += wp;
        const double target = (double)tot * acc / wsum;
        while (b < hi && (double)run + (double)wgt[b] / 2 <= target) {
            run += wgt[b];
            b++;
        }
        out[j] = b;
    }
}

// The bucket plan of the record exchange.  wgt[b] = the records bucket b holds on all ranks.  Returns cuts[j] for
// j = 0 .. W * P: owner o's group p = buckets [cuts[o * P + p], cuts[o * P + p + 1]).  Owners first: contiguous ranges of
// equal weight (bucket_owner_ranges_weighted).  Then every owner's range into P groups that grow geometrically, 1 : 3 : 9 ...
// (bucket_group_cuts): the first one lands -- and its counting starts -- after a small share of the transfer, and every later
// group is still in flight while a group a third of its size is being counted.  Nothing to weigh: the even W * P split.
inline std::vector<u32> exchange_cuts(const std::vector<u64> &wgt, int W, int P)
{
    const u32 nb = (u32)wgt.size();
    const int WP = W * P;
    std::vector<u32> cuts((size_t)WP + 1, 0);
    cuts[(size_t)WP] = nb;
    u64 wtotal = 0;
    for (u64 w : wgt)
        wtotal += w;
    if (wtotal == 0) {
        for (int j = 1; j < WP; j++)
            cuts[(size_t)j] = (u32)(((u64)j * nb + (u64)WP - 1) / (u64)WP);
        return cuts;
    }
    std::vector<u32> ocut((size_t)W + 1, 0);
    weighted_cuts(wgt, 0, nb, W, 1.0, ocut.data());
    for (int o = 0; o < W; o++)
        weighted_cuts(wgt, ocut[(size_t)o], std::max(ocut[(size_t)o + 1], ocut[(size_t)o]), P, 3.0, &cuts[(size_t)o * P]);
    return cuts;
}

// The landing buffer of the bucket group [b_lo, b_hi): the records of its buckets, bucket after bucket, in the form
// count_sk_received takes -- blen[d] records at boff[d] for every coarse bucket d < n_coarse (0 outside the group),
// boff[n_coarse] = n_recs = all of them.  (The buckets of a plan are coarse buckets: wgt.size() <= n_coarse.)
struct GroupLayout {
    std::vector<u64> blen, boff;
    u64 n_recs = 0;
};
inline GroupLayout group_layout(const std::vector<u64> &wgt, u32 b_lo, u32 b_hi, u32 n_coarse)
{
    GroupLayout l;
    l.blen.assign(n_coarse, 0);
    l.boff.assign((size_t)n_coarse + 1, 0);
    for (u32 b = b_lo; b < b_hi; b++)
        l.blen[b] = wgt[b];
    for (u32 d = 0; d < n_coarse; d++)
        l.boff[d + 1] = l.boff[d] + l.blen[d];
    l.n_recs = l.boff[n_coarse];
    return l;
}

}  // namespace dnagpu
