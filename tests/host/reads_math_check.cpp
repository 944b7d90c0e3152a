// Host-side check of what text_math.hpp adds for dnagpu_reads_from_text: the masks one lane makes of its 32
// bytes, each against a loop over the bytes that states the contract of include/dnagpu.h.
//   - the class of every one of the 256 bytes, with and without DNAGPU_READS_FOLD_CASE, through reads_chunk_byte;
//   - the FASTQ role masks for every line index mod 4 and every newline mask of 16 bytes (at both ends of the chunk), and
//     random 32-byte ones;
//   - the piece-start mask of DNAGPU_AMBIG_SPLIT and its undecided bit, for every pattern of 8 bytes over {other, base, break,
//     base that is a break} with and without a kept base / a break before the chunk, and random 32-byte ones;
//   - the newline that DNAGPU_TEXT_MORE cuts a FASTQ text at and the truncated record begins at, and text_nth_bit.
// Built and run by tests/test_reads_from_text.py with hipcc (host code only: no device is touched).
#include <cstdio>
#include <cstring>
#include <string>
#include "text_math.hpp"

using namespace dnagpu;

static int bad = 0;
#define CHECK(cond, ...)                                                                                                          \
    do {                                                                                                                          \
        if (!(cond)) {                                                                                                            \
            if (bad < 20) {                                                                                                       \
                printf(__VA_ARGS__);                                                                                              \
                printf("  [%s:%d]\n", __FILE__, __LINE__);                                                                        \
            }                                                                                                                     \
            bad++;                                                                                                                \
        }                                                                                                                         \
    } while (0)

static u64 rng_state = 0x13198A2E03707344ull;
static u64 rng() { return rng_state = splitmix64(rng_state); }

static void check_classes()
{
    for (int fold = 0; fold < 2; fold++)
        for (u32 byte = 0; byte < 256; byte++) {
            const char ch = (char)byte;
            bool base = byte && strchr("ATCG", ch), amb = byte && strchr("NRYKMSWBDHV", ch);
            if (fold) {
                base = base || (byte && strchr("atcg", ch));
                amb = amb || (byte && strchr("nrykmswbdhv", ch));
            }
            for (u32 j = 0; j < 32; j += 31) {
                ReadsChunk r = {};
                reads_chunk_byte(r, j, byte, fold != 0);
                const u32 bit = 1u << j;
                CHECK(r.c.base == (base ? bit : 0u) && r.amb == (amb ? bit : 0u), "class of byte %u fold %d", byte, fold);
                CHECK(r.at == (byte == '@' ? bit : 0u) && r.plus == (byte == '+' ? bit : 0u), "'@' / '+' of byte %u", byte);
                CHECK(r.c.nl == (byte == '\n' ? bit : 0u) && r.c.cr == (byte == '\r' ? bit : 0u) && r.c.gt == (byte == '>' ? bit : 0u),
                      "terminator class of byte %u", byte);
                if (base) {
                    const char up = (char)(byte & ~32u);
                    CHECK(((r.c.codes >> (2 * j)) & 3) == (u64)(strchr("ATCG", up) - "ATCG"), "code of byte %u", byte);
                } else {
                    CHECK(r.c.codes == 0, "code of the non-base %u", byte);
                }
            }
        }
}

static void check_roles_of(u32 nl, u32 line0)
{
    u32 role[4], want[4] = {0, 0, 0, 0};
    reads_roles(nl, line0, role);
    u32 line = line0;
    for (u32 j = 0; j < 32; j++) {
        want[line % 4] |= 1u << j;
        if ((nl >> j) & 1)
            line++;
    }
    CHECK(!memcmp(role, want, sizeof role), "roles of nl %08x from line %u", nl, line0);
    CHECK((role[0] | role[1] | role[2] | role[3]) == ~0u && (role[0] & role[1]) == 0 && (role[2] & role[3]) == 0, "roles overlap");
}
static void check_roles()
{
    for (u32 line0 = 0; line0 < 8; line0++) {
        for (u32 m = 0; m < 65536; m++) {
            check_roles_of(m, line0);
            check_roles_of(m << 16, line0);
        }
        for (int i = 0; i < 100000; i++)
            check_roles_of((u32)rng() & (u32)rng(), line0 + (u32)rng() % 1000);
        check_roles_of(~0u, line0);
    }
}

static void check_pieces_of(u32 keep, u32 brk, u32 at, u32 pk, u32 pb)
{
    u32 und = 0, want = 0, want_und = 0;
    const u32 got = reads_piece_starts(keep, brk, at, pk, pb, &und);
    u32 k = pk, b = pb;
    for (u32 j = 0; j < 32; j++) {
        if ((brk >> j) & 1)
            b = at + j;                              // a break at the base itself counts: a line start that is a base
        if ((keep >> j) & 1) {
            if (!(k | b))
                want_und |= 1u << j;
            else if (k < b)
                want |= 1u << j;
            k = at + j;
        }
    }
    CHECK(got == want && und == want_und, "pieces of keep %08x brk %08x at %u pk %u pb %u: %08x/%08x, want %08x/%08x", keep, brk, at,
          pk, pb, got, und, want, want_und);
}
static void check_pieces()
{
    const u32 at = 5 * TEXT_CHUNK + 1;
    const u32 before[4] = {0, 1, at - 2, at - 1};
    for (u32 pat = 0; pat < 65536; pat++) {          // 8 bytes, 2 bits each: bit 0 kept base, bit 1 break
        u32 keep = 0, brk = 0;
        for (u32 j = 0; j < 8; j++) {
            keep |= ((pat >> (2 * j)) & 1) << j;
            brk |= ((pat >> (2 * j + 1)) & 1) << j;
        }
        for (u32 pk : before)
            for (u32 pb : before) {
                check_pieces_of(keep, brk, at, pk, pb);
                check_pieces_of(keep << 24, brk << 24, at, pk, pb);
            }
    }
    for (int i = 0; i < 300000; i++) {
        const u32 keep = (u32)rng() | ((u32)rng() & (u32)rng()), brk = (u32)rng() & (u32)rng() & (u32)rng();
        check_pieces_of(keep, brk, at, before[rng() % 4], before[rng() % 4]);
        check_pieces_of(keep, i % 2 ? brk & ~keep : brk, 1, 0, 0);
    }
    check_pieces_of(~0u, 0, 1, 0, 0);
    check_pieces_of(~0u, 1, 1, 0, 0);
    check_pieces_of(~0u, 0x80000000u, at, 3, 2);
}

static void check_fastq_cut()
{
    for (u32 m = 1; m < 4096; m++)
        for (u32 k = 1; k <= (u32)__builtin_popcount(m); k++) {
            u32 seen = 0, j = 0;
            for (; j < 32; j++)
                if (((m >> j) & 1) && ++seen == k)
                    break;
            CHECK(text_nth_bit(m, k) == j && text_nth_bit(m << 20, k) == j + 20, "bit %u of %08x", k, m);
        }
    for (int i = 0; i < 20000; i++) {
        std::string t;
        const u32 n = 1 + (u32)rng() % 40;
        for (u32 j = 0; j < n; j++)
            t += rng() % 3 ? 'A' : '\n';
        // the lines, one by one
        u64 lines = 0, newlines = 0;
        for (u32 j = 0; j < n; j++)
            if (t[j] == '\n')
                newlines++;
        for (u32 j = 0; j < n;) {
            lines++;
            while (j < n && t[j] != '\n')
                j++;
            j++;
        }
        const bool ends = t[n - 1] == '\n';
        CHECK(fastq_lines(newlines, ends) == lines, "lines of a text of %u bytes", n);
        for (int more = 0; more < 2; more++) {
            // whole records: four lines each, every one of them ended by a newline under MORE
            const u64 whole = (more ? newlines : lines) / 4;
            CHECK(fastq_cut_newline(newlines, ends, more != 0) == 4 * whole, "cut newline, more %d", more);
            CHECK(more || lines % 4 == 0 || 4 * whole <= newlines, "the truncated record begins behind a newline");
        }
    }
}

int main()
{
    check_classes();
    check_roles();
    check_pieces();
    check_fastq_cut();
    if (bad) {
        printf("%d checks failed\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
