// Host-side check of the merge-path split of index_math.hpp (index_merge_split: what the append's partition kernel asks in
// global memory and every thread of its merge kernel asks in LDS) against a host stable merge, for EVERY diagonal of every
// input: random runs, one repeated value on both sides, an empty A, an empty B, B wholly below / above A, and the values 0
// and UINT64_MAX.  Asserted: the split is the one the stable merge takes (ties go to A), its two defining inequalities, and
// that no element outside [0, |A|) x [0, |B|) is ever read and no split outside [0, |A|] x [0, |B|] produced.  Then the way
// the kernels compose it -- the split of every tile boundary, then of every thread's diagonal inside the tile's slices --
// must reproduce the merge.  Built and run by tests/test_kmer_index_update.py with hipcc (host code only: no device is
// touched).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "index_math.hpp"

using namespace dnagpu;

static int bad = 0;
#define CHECK(cond, ...)                                                                                                          \
    do {                                                                                                                          \
        if (!(cond)) {                                                                                                            \
            printf(__VA_ARGS__);                                                                                                  \
            printf("  [%s:%d]\n", __FILE__, __LINE__);                                                                            \
            bad++;                                                                                                                \
        }                                                                                                                         \
    } while (0)

typedef std::vector<u64> Run;

// a run read through a window [first, first + count) whose every access is checked
struct Window {
    const Run *run;
    u64 first, count;
    const char *what;
    u64 operator()(u64 i) const
    {
        CHECK(i < count && first + i < run->size(), "%s: read of element %llu of %llu", what, (unsigned long long)i,
              (unsigned long long)count);
        return i < count && first + i < run->size() ? (*run)[(size_t)(first + i)] : 0;
    }
};

static void check_case(const char *name, const Run &A, const Run &B)
{
    const u64 na = A.size(), nb = B.size();
    // the host's stable merge: (value, side), A's entry first among equal values
    std::vector<std::pair<u64, int>> ta, tb, merged(na + nb);
    for (u64 v : A)
        ta.push_back({v, 0});
    for (u64 v : B)
        tb.push_back({v, 1});
    std::merge(ta.begin(), ta.end(), tb.begin(), tb.end(), merged.begin(),
               [](const std::pair<u64, int> &x, const std::pair<u64, int> &y) { return x.first < y.first; });
    const Window wa{&A, 0, na, name}, wb{&B, 0, nb, name};
    u64 from_a = 0;                                     // entries of A among the first d outputs of the stable merge
    for (u64 d = 0; d <= na + nb; d++) {
        const u64 a = index_merge_split(wa, na, wb, nb, d), b = d - a;
        CHECK(a <= na && a <= d && b <= nb, "%s: d=%llu split (%llu, %llu) outside", name, (unsigned long long)d,
              (unsigned long long)a, (unsigned long long)b);
        if (a > na || a > d || b > nb)
            return;
        CHECK(a == from_a, "%s: d=%llu split a=%llu, the stable merge took %llu of A", name, (unsigned long long)d,
              (unsigned long long)a, (unsigned long long)from_a);
        if (a > 0 && b < nb)
            CHECK(A[a - 1] <= B[b], "%s: d=%llu A[a-1] > B[b]", name, (unsigned long long)d);
        if (b > 0 && a < na)
            CHECK(B[b - 1] < A[a], "%s: d=%llu B[b-1] >= A[a]: a tie went to B", name, (unsigned long long)d);
        if (d < na + nb)
            from_a += merged[(size_t)d].second == 0;
    }
    // the kernels' two levels, in small: tiles of TILE outputs, threads of ITEMS outputs
    for (u64 TILE : {(u64)16, (u64)6}) {
        const u64 ITEMS = 2, n_tiles = (na + nb + TILE - 1) / TILE;
        std::vector<std::pair<u64, int>> out;
        for (u64 t = 0; t < n_tiles; t++) {
            const u64 d0 = t * TILE, d1 = std::min(d0 + TILE, na + nb);
            const u64 a0 = index_merge_split(wa, na, wb, nb, d0), a1 = index_merge_split(wa, na, wb, nb, d1);
            const u64 b0 = d0 - a0, b1 = d1 - a1;
            CHECK(a1 >= a0 && b1 >= b0, "%s: tile %llu: the splits do not ascend", name, (unsigned long long)t);
            if (a1 < a0 || b1 < b0)
                return;
            const Window sa{&A, a0, a1 - a0, name}, sb{&B, b0, b1 - b0, name};
            for (u64 th = 0; th * ITEMS < d1 - d0; th++) {
                u64 a = index_merge_split(sa, sa.count, sb, sb.count, th * ITEMS), b = th * ITEMS - a;
                for (u64 i = 0; i < ITEMS && th * ITEMS + i < d1 - d0; i++) {
                    const bool has_a = a < sa.count, has_b = b < sb.count;
                    const bool take_a = has_a && (!has_b || sa(a) <= sb(b));
                    CHECK(has_a || has_b, "%s: tile %llu: both slices exhausted early", name, (unsigned long long)t);
                    if (take_a)
                        out.push_back({sa(a++), 0});
                    else if (has_b)
                        out.push_back({sb(b++), 1});
                }
            }
        }
        CHECK(out == merged, "%s: tiles of %llu: the composed merge differs from the stable merge", name, (unsigned long long)TILE);
    }
}

static Run sorted_run(u64 *s, size_t n, u64 mask)
{
    Run r(n);
    for (u64 &v : r) {
        *s = splitmix64(*s);
        v = *s & mask;
    }
    std::sort(r.begin(), r.end());
    return r;
}

int main()
{
    const u64 ONES = ~(u64)0;
    u64 s = 0x3E26E;
    // random runs: 64-bit values (no ties), and few values (long ties across both sides)
    for (int round = 0; round < 60; round++) {
        s = splitmix64(s);
        const size_t na = (size_t)(splitmix64(s + 1) % 70), nb = (size_t)(splitmix64(s + 2) % 70);
        const u64 mask = round % 3 == 0 ? ONES : round % 3 == 1 ? 7 : 1;
        const Run A = sorted_run(&s, na, mask), B = sorted_run(&s, nb, mask);
        check_case("random", A, B);
    }
    check_case("one value on both sides", Run(37, 5), Run(29, 5));
    check_case("one value on both sides, B longer", Run(3, ONES), Run(50, ONES));
    check_case("empty A", Run(), sorted_run(&s, 41, 15));
    check_case("empty B", sorted_run(&s, 41, 15), Run());
    check_case("both empty", Run(), Run());
    check_case("one and one, tied", Run(1, 9), Run(1, 9));
    {
        Run lo = sorted_run(&s, 33, 0xFFFF), hi = sorted_run(&s, 35, 0xFFFF);
        for (u64 &v : hi)
            v += 0x10000;
        check_case("B wholly below A", hi, lo);
        check_case("B wholly above A", lo, hi);
    }
    {
        Run A = {0, 0, 0, 7, ONES, ONES}, B = {0, 0, ONES, ONES, ONES};
        check_case("0 and UINT64_MAX on both sides", A, B);
        check_case("0 and UINT64_MAX, sides swapped", B, A);
        check_case("only UINT64_MAX against only 0", Run(20, ONES), Run(20, 0));
        check_case("only 0 against only UINT64_MAX", Run(20, 0), Run(20, ONES));
        Run top = sorted_run(&s, 40, ONES);
        for (u64 &v : top)
            v |= (u64)1 << 63;                          // the top bit set: an unsigned comparison, not a signed one
        std::sort(top.begin(), top.end());
        check_case("top bit set against clear", top, sorted_run(&s, 40, ONES >> 1));
    }
    if (bad) {
        printf("%d checks failed\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
