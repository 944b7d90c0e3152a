// Host-side check of text_math.hpp (what the kernels of dnagpu_table_from_text and their host driver share): the text is
// parsed twice -- by a byte-by-byte parser that states the contract of include/dnagpu.h line by line, and chunk by chunk (32
// bytes, as a lane sees them) with the header's masks: terminators, line starts, header bytes, the kept bases closed up by
// text_compact, the error word, the cut of a chunk that more text follows.  Both must give the same error (kind and offset),
// or the same bases, record starts and record offsets.  Hand-written texts first, then random ones over an alphabet of bases,
// terminators and every kind of invalid byte, in both formats, with and without DNAGPU_TEXT_MORE.
// Built and run by tests/test_table_from_text.py with hipcc (host code only: no device is touched).
#include <cstdio>
#include <string>
#include <vector>
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

static u64 rng_state = 0x243F6A8885A308D3ull;
static u64 rng() { return rng_state = splitmix64(rng_state); }

struct Parsed {
    u64 err = TEXT_NO_ERROR;
    std::string bases;                // the records' bases back to back
    std::vector<u64> starts, pos;     // per record: its first base, the offset of its first byte
    u64 consumed = 0;
};
static void note(Parsed &p, u64 at, u32 kind)
{
    const u64 k = text_error_key(at, kind);
    if (k < p.err)
        p.err = k;
}
static bool is_base(unsigned char c) { return c == 'A' || c == 'T' || c == 'C' || c == 'G'; }

// ---- the contract, byte by byte
static Parsed by_the_contract(const std::string &t, int format, bool more)
{
    Parsed p;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(t.data());
    u64 n = t.size();
    if (more) {                       // the cut, found forwards: independent of text_more_cut
        u64 cut = format == TEXT_FORMAT_LINES ? 0 : n;
        for (u64 i = 0; i < n; i++) {
            if (format == TEXT_FORMAT_LINES && s[i] == '\n')
                cut = i + 1;
            if (format == TEXT_FORMAT_FASTA && s[i] == '>' && (i == 0 || s[i - 1] == '\n'))
                cut = i;
        }
        n = cut;
    }
    p.consumed = n;
    bool open = false;                // FASTA: a header has been seen
    u64 open_at = 0, open_bases = 0;
    for (u64 a = 0; a < n;) {
        u64 e = a;
        while (e < n && s[e] != '\n')
            e++;
        const bool terminated = e < n;
        u64 c = e;                    // the line's content: [a, c)
        if (terminated && c > a && s[c - 1] == '\r')
            c--;
        if (format == TEXT_FORMAT_LINES) {
            if (c == a)
                note(p, a, TEXT_ERR_EMPTY);
            p.starts.push_back(p.bases.size());
            p.pos.push_back(a);
            for (u64 i = a; i < c; i++) {
                if (is_base(s[i]))
                    p.bases.push_back((char)s[i]);
                else
                    note(p, i, TEXT_ERR_CHAR);
            }
        } else if (s[a] == '>') {
            if (open && open_bases == 0)
                note(p, open_at, TEXT_ERR_EMPTY);
            open = true;
            open_at = a;
            open_bases = 0;
            p.starts.push_back(p.bases.size());
            p.pos.push_back(a);
        } else {
            for (u64 i = a; i < c; i++) {
                if (!open)
                    note(p, i, TEXT_ERR_ORPHAN);
                else if (is_base(s[i])) {
                    p.bases.push_back((char)s[i]);
                    open_bases++;
                } else
                    note(p, i, TEXT_ERR_CHAR);
            }
        }
        a = e + 1;
    }
    if (format == TEXT_FORMAT_FASTA && open && open_bases == 0)
        note(p, open_at, TEXT_ERR_EMPTY);
    return p;
}

// ---- the same through the header, a lane's chunk at a time
static Parsed by_the_chunks(const std::string &t, int format, bool more)
{
    Parsed p;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(t.data());
    const u64 n = more ? text_more_cut(s, t.size(), format) : t.size();
    p.consumed = n;
    const bool fasta = format == TEXT_FORMAT_FASTA;
    bool in_header = false, seen = false;
    u64 last_header = 0, last_base = 0;      // offset + 1, 0: none
    std::vector<u64> words;
    u64 n_bases = 0;
    for (u64 b = 0; b < n; b += TEXT_CHUNK) {
        TextChunk c = {};
        const u64 left = n - b;
        c.valid = text_low_bits(left >= TEXT_CHUNK ? TEXT_CHUNK : (u32)left);
        for (u32 j = 0; j < TEXT_CHUNK; j++)
            text_chunk_byte(c, j, j < left ? s[b + j] : 0u);
        c.prev_nl = b == 0 || s[b - 1] == '\n';
        c.next_nl = left > TEXT_CHUNK && s[b + TEXT_CHUNK] == '\n';
        const u32 starts = text_line_starts(c), headers = fasta ? starts & c.gt : 0u;
        const u32 header_bytes = fasta ? text_header_bytes(starts, headers, in_header) & c.valid : 0u;
        if (starts)
            in_header = (headers >> text_top_bit(starts)) & 1;
        const u32 keep = c.base & ~header_bytes, invalid = text_invalid(c) & ~header_bytes;
        CHECK(!(c.base & ~c.valid) && !(invalid & text_terminators(c)), "masks leave the text at %llu", (unsigned long long)b);
        if (!fasta) {
            const u32 empty = starts & text_terminators(c);
            for (u32 j = 0; j < TEXT_CHUNK; j++) {
                if ((invalid >> j) & 1)
                    note(p, b + j, TEXT_ERR_CHAR);
                if ((empty >> j) & 1)
                    note(p, b + j, TEXT_ERR_EMPTY);
            }
        }
        for (u32 j = 0; j < TEXT_CHUNK; j++) {
            if (((fasta ? headers : starts) >> j) & 1) {
                if (fasta) {
                    if (last_header && last_base < last_header)
                        note(p, last_header - 1, TEXT_ERR_EMPTY);
                    last_header = b + j + 1;
                    seen = true;
                }
                p.starts.push_back(n_bases + (u64)__builtin_popcount(keep & text_low_bits(j)));
                p.pos.push_back(b + j);
            }
            if (fasta && (((keep | invalid) >> j) & 1)) {
                if (!seen)
                    note(p, b + j, TEXT_ERR_ORPHAN);
                else if ((invalid >> j) & 1)
                    note(p, b + j, TEXT_ERR_CHAR);
                if ((keep >> j) & 1)
                    last_base = b + j + 1;
            }
        }
        // the kept bases, closed up and appended at bit 2 n_bases
        const u64 v = text_compact(c.codes, keep);
        const u32 cnt = (u32)__builtin_popcount(keep), at = (u32)(n_bases & 31);
        CHECK(cnt == 32 || (v >> (2 * cnt)) == 0, "text_compact leaves bits behind its bases at %llu", (unsigned long long)b);
        if (cnt) {
            if (at == 0)
                words.push_back(0);
            words.back() |= v << (2 * at);
            if (at + cnt > 32)
                words.push_back(v >> (64 - 2 * at));
            n_bases += cnt;
        }
    }
    if (fasta && last_header && last_base < last_header)
        note(p, last_header - 1, TEXT_ERR_EMPTY);
    for (u64 i = 0; i < n_bases; i++)
        p.bases.push_back("ATCG"[(words[(size_t)(i >> 5)] >> (2 * (i & 31))) & 3]);
    return p;
}

static void compare(const std::string &t, int format, bool more)
{
    const Parsed a = by_the_contract(t, format, more), b = by_the_chunks(t, format, more);
    CHECK(a.consumed == b.consumed, "consumed %llu / %llu (format %d more %d, %zu bytes)", (unsigned long long)a.consumed,
          (unsigned long long)b.consumed, format, (int)more, t.size());
    CHECK(a.err == b.err, "error word %llx / %llx (format %d more %d, %zu bytes)", (unsigned long long)a.err,
          (unsigned long long)b.err, format, (int)more, t.size());
    if (a.err == TEXT_NO_ERROR && b.err == TEXT_NO_ERROR)
        CHECK(a.bases == b.bases && a.starts == b.starts && a.pos == b.pos, "records differ (format %d more %d, %zu bytes)", format,
              (int)more, t.size());
}

struct Hand {
    const char *text;
    int format;
    bool more;
    u64 err;                // TEXT_NO_ERROR, or the error word
    const char *bases;
    u64 records, consumed;
};

int main()
{
    const u64 OK = TEXT_NO_ERROR;
    const int L = TEXT_FORMAT_LINES, F = TEXT_FORMAT_FASTA;
    const Hand hand[] = {
        {"AT\nCG", L, false, OK, "ATCG", 2, 5},
        {"AT\nCG", L, true, OK, "AT", 1, 3},
        {"AT\r\nCG\r\n", L, false, OK, "ATCG", 2, 8},
        {"AT\r\nCG\r\n", L, true, OK, "ATCG", 2, 8},
        {"\n", L, false, text_error_key(0, TEXT_ERR_EMPTY), "", 0, 0},
        {"\n", L, true, text_error_key(0, TEXT_ERR_EMPTY), "", 0, 0},
        {"A\n\nT\n", L, false, text_error_key(2, TEXT_ERR_EMPTY), "", 0, 0},
        {"A\n\nT\n", L, true, text_error_key(2, TEXT_ERR_EMPTY), "", 0, 0},
        {">x\nAT\nCG\n>y\n\nGG", F, false, OK, "ATCGGG", 2, 15},
        {">x\nAT\nCG\n>y\n\nGG", F, true, OK, "ATCG", 1, 9},
        {">x\n>y\nA", F, false, text_error_key(0, TEXT_ERR_EMPTY), "", 0, 0},
        {">x\n>y\nA", F, true, text_error_key(0, TEXT_ERR_EMPTY), "", 0, 0},
        {"A\n>x\nT", F, false, text_error_key(0, TEXT_ERR_ORPHAN), "", 0, 0},
        {"A\n>x\nT", F, true, text_error_key(0, TEXT_ERR_ORPHAN), "", 0, 0},
        {"AT\rCG\n", L, false, text_error_key(2, TEXT_ERR_CHAR), "", 0, 0},
        {"ATCG", L, true, OK, "", 0, 0},
        {"\n\r\n", F, true, OK, "", 0, 3},
        {">x N a\nAT\n>y", F, false, text_error_key(10, TEXT_ERR_EMPTY), "", 0, 0},
        {">x N a\nAT\n>y", F, true, OK, "AT", 1, 10},
    };
    for (const Hand &h : hand) {
        const std::string t(h.text);
        for (int which = 0; which < 2; which++) {
            const Parsed p = which ? by_the_chunks(t, h.format, h.more) : by_the_contract(t, h.format, h.more);
            CHECK(p.err == h.err, "hand case %d of parser %d: error word %llx", (int)(&h - hand), which, (unsigned long long)p.err);
            if (h.err == OK)
                CHECK(p.bases == h.bases && p.starts.size() == h.records && p.consumed == h.consumed,
                      "hand case %d of parser %d: %s, %zu records, consumed %llu", (int)(&h - hand), which, p.bases.c_str(),
                      p.starts.size(), (unsigned long long)p.consumed);
        }
    }
    // text_compact on every run shape: keep = bits [a, b) and its complement
    for (u32 a = 0; a <= 32; a++)
        for (u32 b = a; b <= 32; b++)
            for (int inv = 0; inv < 2; inv++) {
                const u32 keep = inv ? ~text_bit_range(a, b) : text_bit_range(a, b);
                const u64 codes = rng();
                u64 want = 0;
                u32 at = 0;
                for (u32 j = 0; j < 32; j++)
                    if ((keep >> j) & 1)
                        want |= ((codes >> (2 * j)) & 3) << (2 * at++);
                CHECK(text_compact(codes, keep) == want, "text_compact keep %08x", keep);
            }
    for (u32 c = 0; c < 256; c++)
        CHECK(base_code(c) == (c == 'A' ? 0u : c == 'T' ? 1u : c == 'C' ? 2u : c == 'G' ? 3u : 4u), "base_code %u", c);
    // random texts: mostly valid lines of 0 .. 70 bytes, now and then a header, a blank line, CRLF, an invalid byte
    const char odd[] = {'N', 'a', ' ', '\t', '\\', '\r', '>', 'U'};
    for (int iter = 0; iter < 60000; iter++) {
        std::string t;
        const u32 lines = (u32)(rng() % 8), dirt = (u32)(rng() % 4);      // dirt 0: clean; else one odd byte per ~dirt * 40
        const bool fasta_like = rng() & 1, crlf = rng() & 1;
        for (u32 i = 0; i < lines; i++) {
            const u64 r = rng();
            if (fasta_like && (i == 0 ? r % 8 != 0 : r % 3 == 0)) {
                t += '>';
                for (u32 j = (u32)(rng() % 40); j > 0; j--)
                    t += "ATCGN >x\t"[rng() % 9];
            } else {
                for (u32 j = (u32)((r >> 8) % 71) * (u32)((r >> 20) % 16 != 0); j > 0; j--)
                    t += dirt && rng() % (dirt * 40) == 0 ? odd[rng() % sizeof odd] : "ATCG"[rng() & 3];
            }
            if (i + 1 < lines || rng() % 3)
                t += crlf && rng() % 8 ? "\r\n" : "\n";
        }
        for (int format = 1; format <= 2; format++)
            for (int more = 0; more < 2; more++)
                compare(t, format, more != 0);
    }
    printf(bad ? "%d FAILED\n" : "ok\n", bad);
    return bad != 0;
}
