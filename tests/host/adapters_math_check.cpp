// Host-side check of adapters_math.hpp: the mismatches of a window (planes, deny masks, overlap mask, popcount) and the
// thr table against a per-base loop -- every adapter length 1..32, every overlap 1..L, every IUPAC letter, 10^5 random
// windows -- and the sixteen positions of one lane (the word loads, the funnel shift, the segment's end) against the
// contract's plain loops over random streams at every alignment.  Built and run by tests/test_adapters_model.py with hipcc
// (host code only: no device is touched).  Stand-alone, so it may also be built with a host sanitizer and run directly.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "adapters_math.hpp"

using namespace dnagpu;

static const char LETTERS[] = "ATCGUWSMKRYBDHVN";
// the sets of the qkmer alphabet, written out again here (bit0 = A, bit1 = T, bit2 = C, bit3 = G)
static int letter_set(char c)
{
    switch (c) {
    case 'A': return 1; case 'T': return 2; case 'C': return 4; case 'G': return 8; case 'U': return 0;
    case 'W': return 1 | 2; case 'S': return 4 | 8; case 'M': return 1 | 4; case 'K': return 2 | 8;
    case 'R': return 1 | 8; case 'Y': return 2 | 4; case 'B': return 2 | 4 | 8; case 'D': return 1 | 2 | 8;
    case 'H': return 1 | 2 | 4; case 'V': return 1 | 4 | 8; case 'N': return 15;
    }
    return -1;
}

static u64 rng_state = 0x2545F4914F6CDD1Dull;
static u64 rnd() { return rng_state = splitmix64(rng_state); }

static int base_at(const std::vector<u64> &words, u64 b) { return (int)((words[b >> 5] >> (2 * (b & 31))) & 3); }

// the contract's rule by plain loops: the least (p, m, a) among positions [p_lo, p_hi) of the segment
static u64 slow_best(const std::vector<u64> &words, u64 first, u64 n, u64 p_lo, u64 p_hi, const std::vector<std::vector<int>> &sets,
                     u32 err_num, u32 err_den, u32 min_overlap)
{
    for (u64 p = p_lo; p < p_hi && p < n; p++) {
        u64 best = ADAPTERS_NONE;
        for (u32 a = 0; a < sets.size(); a++) {
            const u64 L = sets[a].size(), o = L < n - p ? L : n - p, need = min_overlap < L ? min_overlap : L;
            u64 m = 0;
            for (u64 j = 0; j < o; j++)
                m += !((sets[a][j] >> base_at(words, first + p + j)) & 1);
            if (o >= need && m * err_den <= (u64)err_num * o) {
                const u64 key = adapter_key(p, (u32)m, a);
                best = key < best ? key : best;
            }
        }
        if (best != ADAPTERS_NONE)
            return best;
    }
    return ADAPTERS_NONE;
}

int main()
{
    int bad = 0;
    // ---- the thr table: every length, overlap, min_overlap and a set of rationals
    const u32 rates[][2] = {{0, 1}, {1, 10}, {1, 5}, {1, 3}, {1, 1}, {3, 32}, {7, 9}};
    for (u32 L = 1; L <= 32; L++)
        for (u32 mo = 1; mo <= 32; mo++)
            for (auto &r : rates) {
                int sets[32];
                for (u32 j = 0; j < L; j++)
                    sets[j] = 15;
                AdapterDesc d;
                adapter_build(sets, L, r[0], r[1], mo, &d);
                for (u32 o = 0; o <= 32; o++) {
                    int want = -1;
                    if (o <= L && o >= (mo < L ? mo : L))
                        for (u32 m = 0; m <= o; m++)
                            if ((u64)m * r[1] <= (u64)r[0] * o)
                                want = (int)m;
                    if (d.thr[o] != want && bad++ < 20)
                        printf("thr: L=%u min_overlap=%u rate=%u/%u o=%u: %d, expected %d\n", L, mo, r[0], r[1], o, d.thr[o], want);
                }
            }
    // ---- the mismatches of a window: every length, every overlap, letters drawn from the whole alphabet (each letter at each
    // position in turn for the first sixteen windows), 10^5 windows in all
    u64 windows = 0;
    while (windows < 100000)
        for (u32 L = 1; L <= 32 && windows < 100000; L++) {
            int sets[32];
            for (u32 j = 0; j < L; j++)
                sets[j] = letter_set(LETTERS[windows < 16 * 32 ? (windows + j) % 16 : rnd() % 16]);
            AdapterDesc d;
            adapter_build(sets, L, 1, 1, 1, &d);
            for (u32 o = 1; o <= L; o++, windows++) {
                const u64 win = rnd();
                u32 want = 0;
                for (u32 j = 0; j < o; j++)
                    want += !((sets[j] >> ((win >> (2 * j)) & 3)) & 1);
                const u32 got = adapter_mismatches(adapter_planes(win), d.deny, o);
                if (got != want && bad++ < 20)
                    printf("mismatches: L=%u o=%u window=%llx: %u, expected %u\n", L, o, (unsigned long long)win, got, want);
            }
        }
    // ---- one lane: random streams, segments at every alignment, the stream ending with the segment (no word behind it)
    for (int round = 0; round < 4000; round++) {
        const u64 first = rnd() % 70, n = 1 + rnd() % 90, total = first + n + (round & 1 ? 0 : rnd() % 40);
        std::vector<u64> words((total + 31) / 32);
        for (auto &w : words)
            w = round % 7 == 0 ? 0 : rnd();          // (a stream of A: many hits at every position)
        const u32 n_ads = 1 + (u32)(rnd() % 3), mo = 1 + (u32)(rnd() % 8);
        const auto &r = rates[rnd() % 4];
        std::vector<std::vector<int>> sets(n_ads);
        std::vector<AdapterDesc> ads(n_ads);
        for (u32 a = 0; a < n_ads; a++) {
            const u32 L = a == 0 ? 1 + (u32)(rnd() % 32) : (rnd() & 1 ? 32 : 31);
            for (u32 j = 0; j < L; j++)
                sets[a].push_back(letter_set(LETTERS[rnd() % 5 == 0 ? rnd() % 16 : rnd() % 4]));
            adapter_build(sets[a].data(), L, r[0], r[1], mo, &ads[a]);
        }
        u64 out_of_range = 0;
        const auto word = [&](u64 w) {
            if (w >= words.size() || w > ((first + n - 1) >> 5) || w < (first >> 5))
                out_of_range++;
            return w < words.size() ? words[w] : ~(u64)0;
        };
        for (u64 p0 = 0; p0 < n + ADAPTERS_LANE_POS; p0 += ADAPTERS_LANE_POS) {
            const u64 got = adapter_lane_best(word, first, n, p0, ads.data(), n_ads);
            const u64 want = slow_best(words, first, n, p0, p0 + ADAPTERS_LANE_POS, sets, r[0], r[1], mo);
            if (got != want && bad++ < 20)
                printf("lane: round %d first=%llu n=%llu p0=%llu: key %llx, expected %llx\n", round, (unsigned long long)first,
                       (unsigned long long)n, (unsigned long long)p0, (unsigned long long)got, (unsigned long long)want);
        }
        if (out_of_range && bad++ < 20)
            printf("lane: round %d asked for %llu words that hold no base of the segment\n", round, (unsigned long long)out_of_range);
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
