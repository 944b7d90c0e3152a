// Host-side driver of multi_math.hpp, the arithmetic of the multi-GPU counts: it computes, the test compares.  Built and run
// by tests/test_sharded.py with hipcc (host code only: no device is touched), once more with AddressSanitizer and
// UndefinedBehaviorSanitizer.  Cases are read from stdin, one per line, until it ends.
//
// No argument -- the bucket plan of the record exchange.  In: W P nb w0 .. w(nb-1).  Out, three lines per case:
//   cuts   the W * P + 1 cut points of exchange_cuts
//   groups per group, in owner-then-group order: n_recs:boff[n_coarse] of its group_layout (n_coarse = the power of two
//          >= max(nb, 2), as the record count's coarse buckets are)
//   layout per bucket, in bucket order: blen[b]:boff[b] in the layout of the group that holds b, or "x" if no group or more
//          than one does; then "rest=0" if every blen[] entry outside its group's buckets is 0, else "rest=1"
// Argument "rows" -- a rank's rows.  In: n_words per W first count.  Out, one line: per rank w_hi:row_lo:row_hi:halo.
#include <cstdio>
#include <cstring>
#include <vector>
#include "multi_math.hpp"

using namespace dnagpu;

static bool read_u64(unsigned long long *v) { return scanf("%llu", v) == 1; }

static int plan_cases()
{
    unsigned long long W, P, nb;
    while (read_u64(&W)) {
        if (!read_u64(&P) || !read_u64(&nb) || W < 1 || P < 1)
            return 2;
        std::vector<u64> wgt((size_t)nb);
        for (u64 &w : wgt) {
            unsigned long long v;
            if (!read_u64(&v))
                return 2;
            w = v;
        }
        u32 n_coarse = 2;
        while (n_coarse < nb)
            n_coarse *= 2;
        const std::vector<u32> cuts = exchange_cuts(wgt, (int)W, (int)P);
        printf("cuts");
        for (u32 c : cuts)
            printf(" %u", c);
        printf("\ngroups");
        std::vector<int> holders((size_t)nb, 0);
        std::vector<u64> len_of((size_t)nb, 0), off_of((size_t)nb, 0);
        bool rest_zero = true;
        for (size_t j = 0; j + 1 < cuts.size(); j++) {
            const u32 b_lo = cuts[j], b_hi = std::max(cuts[j + 1], b_lo);
            const GroupLayout l = group_layout(wgt, b_lo, b_hi, n_coarse);
            printf(" %llu:%llu", (unsigned long long)l.n_recs, (unsigned long long)l.boff[n_coarse]);
            for (u32 d = 0; d < n_coarse; d++) {
                if (d >= b_lo && d < b_hi) {
                    holders[d]++;
                    len_of[d] = l.blen[d];
                    off_of[d] = l.boff[d];
                } else if (l.blen[d]) {
                    rest_zero = false;
                }
            }
        }
        printf("\nlayout");
        for (size_t b = 0; b < (size_t)nb; b++) {
            if (holders[b] == 1)
                printf(" %llu:%llu", (unsigned long long)len_of[b], (unsigned long long)off_of[b]);
            else
                printf(" x");
        }
        printf(" rest=%d\n", rest_zero ? 0 : 1);
    }
    return 0;
}

static int rows_cases()
{
    unsigned long long n_words, per, W, first, count;
    while (read_u64(&n_words)) {
        if (!read_u64(&per) || !read_u64(&W) || !read_u64(&first) || !read_u64(&count))
            return 2;
        for (int r = 0; r < (int)W; r++) {
            const RankRows rr = rank_rows(n_words, per, r, first, count);
            printf("%s%llu:%llu:%llu:%d", r ? " " : "", (unsigned long long)rr.w_hi, (unsigned long long)rr.row_lo,
                   (unsigned long long)rr.row_hi, rr.halo ? 1 : 0);
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    const int rc = argc > 1 && !strcmp(argv[1], "rows") ? rows_cases() : plan_cases();
    if (rc)
        fprintf(stderr, "malformed case\n");
    return rc;
}
