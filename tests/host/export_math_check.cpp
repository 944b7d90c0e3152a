// Host-side check of export_math.hpp (the record arithmetic that the sweep of dnagpu_text_image_read and the plan of
// dnagpu_table_to_text share): for hand-written and ~50,000 random tables -- lengths with empties among them, a line width, a
// terminator, numbers up to 2^64 - 1, a prefix -- a naive writer forms the image record by record and line by line, and the
// header's map must give the same bytes when it starts at EVERY offset of every record (export_locate, one division) and
// walks 16 bytes on from there (export_emit / export_advance / export_begin), across record ends.  The sizes the plan sums
// (export_extras) and the header length the sweep derives from a record's size must agree with the naive image; the digit
// count is checked at every power of ten and one below, up to 2^64 - 1.
// Built and run by tests/test_table_to_text.py with hipcc (host code only: no device is touched).
#include <cstdio>
#include <string>
#include <vector>
#include "export_math.hpp"

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

struct Table {
    std::vector<std::vector<unsigned>> seqs;      // codes
    std::vector<u64> numbers;
    std::string prefix;
};

static std::string naive_number(u64 v)
{
    char buf[32];
    snprintf(buf, sizeof buf, "%llu", (unsigned long long)v);
    return buf;
}

// the contract, written out: record after record, line after line
static std::string naive_record(const Table &t, size_t s, int format, bool crlf, u64 width, char quality)
{
    const std::string T = crlf ? "\r\n" : "\n";
    std::string bases, out;
    for (unsigned c : t.seqs[s])
        bases += "ATCG"[c];
    if (format == EXPORT_LINES)
        return bases + T;
    out = (format == EXPORT_FASTA ? ">" : "@") + t.prefix + naive_number(t.numbers[s]) + T;
    if (format == EXPORT_FASTA) {
        const size_t w = width == 0 || width >= bases.size() ? bases.size() : (size_t)width;
        for (size_t at = 0; at < bases.size(); at += w)
            out += bases.substr(at, w) + T;
        return out;
    }
    return out + bases + T + "+" + T + std::string(bases.size(), quality) + T;
}

static void plain_divmod(u64 x, u64 d, u64 *q, u64 *m)
{
    *q = x / d;
    *m = x % d;
}

static void check_table(const Table &t, int format, bool crlf, u64 width, char quality, const char *what)
{
    ExportFmt f;
    f.format = format;
    f.term = crlf ? 2 : 1;
    f.width = width;
    f.prefix_len = format == EXPORT_LINES ? 0 : (u32)t.prefix.size();
    f.quality = (unsigned char)quality;
    const size_t n = t.seqs.size();
    std::string image;
    std::vector<u64> pos(n + 1, 0), start(n + 1, 0);
    std::vector<unsigned> stream;
    for (size_t s = 0; s < n; s++) {
        const std::string rec = naive_record(t, s, format, crlf, width, quality);
        const u64 len = t.seqs[s].size();
        const u32 hl = export_header_len(f, t.numbers[s]);
        CHECK(export_extras(f, len, hl) == rec.size() - len, "%s: extras of record %zu: %llu, the record has %zu bytes and %llu bases",
              what, s, (unsigned long long)export_extras(f, len, hl), rec.size(), (unsigned long long)len);
        CHECK(export_header_from_size(f, len, rec.size()) == hl, "%s: header length from the size of record %zu", what, s);
        image += rec;
        pos[s + 1] = image.size();
        start[s + 1] = start[s] + len;
        stream.insert(stream.end(), t.seqs[s].begin(), t.seqs[s].end());
    }
    const unsigned char *prefix = reinterpret_cast<const unsigned char *>(t.prefix.data());
    for (size_t s0 = 0; s0 < n; s0++)
        for (u64 off = 0; off < pos[s0 + 1] - pos[s0]; off++) {
            size_t s = s0;
            ExportRec r = {t.seqs[s].size(), t.numbers[s], export_header_len(f, t.numbers[s])};
            ExportCursor c = export_locate(f, r, off, plain_divmod);
            u64 next = start[s] + c.base;            // the next base of the stream: consecutive from here on
            const u64 p0 = pos[s0] + off;
            for (u64 j = 0; j < EXPORT_CHUNK && p0 + j < image.size(); j++) {
                while (c.rem == 0) {
                    if (!export_advance(f, r, c)) {
                        s++;
                        r = ExportRec{t.seqs[s].size(), t.numbers[s], export_header_len(f, t.numbers[s])};
                        c = export_begin(f, r);
                        CHECK(start[s] == next, "%s: record %zu begins at base %llu, the walk stands at %llu", what, s,
                              (unsigned long long)start[s], (unsigned long long)next);
                    }
                }
                const u32 b = export_emit(f, r, c, prefix, [&]() { return stream[(size_t)next++]; });
                CHECK(b == (unsigned char)image[(size_t)(p0 + j)], "%s: byte %llu (from offset %llu of record %zu, step %llu): %u, expected %u",
                      what, (unsigned long long)(p0 + j), (unsigned long long)off, s0, (unsigned long long)j, b,
                      (unsigned)(unsigned char)image[(size_t)(p0 + j)]);
                if (bad > 20)
                    return;
            }
        }
}

static Table make_table(const std::vector<u64> &lens, const std::vector<u64> &numbers, const std::string &prefix)
{
    Table t;
    t.prefix = prefix;
    for (size_t i = 0; i < lens.size(); i++) {
        std::vector<unsigned> seq((size_t)lens[i]);
        for (auto &c : seq)
            c = (unsigned)(rng() & 3);
        t.seqs.push_back(seq);
        t.numbers.push_back(i < numbers.size() ? numbers[i] : (u64)i);
    }
    return t;
}

int main()
{
    // ---- digits
    u64 p = 1;
    for (u32 d = 1; d <= 20; d++) {
        CHECK(export_digits(p) == d, "digits of 10^%u", d - 1);
        if (d > 1)
            CHECK(export_digits(p - 1) == d - 1, "digits of 10^%u - 1", d - 1);
        const std::string text = naive_number(p + 7 * (p / 10));
        for (u32 i = 0; i < text.size(); i++)
            CHECK('0' + export_digit_at(p + 7 * (p / 10), (u32)text.size(), i) == (u32)text[i], "digit %u of %s", i, text.c_str());
        if (d < 20)
            p *= 10;
    }
    CHECK(export_digits(0) == 1 && export_digits(9) == 1 && export_digits(10) == 2, "digits of 0, 9, 10");
    CHECK(export_digits(~(u64)0) == 20, "digits of 2^64 - 1");
    const std::string top = naive_number(~(u64)0);
    for (u32 i = 0; i < 20; i++)
        CHECK('0' + export_digit_at(~(u64)0, 20, i) == (u32)top[i], "digit %u of 2^64 - 1", i);

    // ---- hand-written tables: every format, both terminators, the widths around the lengths
    const std::vector<u64> lens = {0, 1, 0, 0, 0, 2, 3, 15, 16, 17, 31, 32, 33, 0, 64, 65, 1, 1, 1};
    const std::vector<u64> numbers = {0, 9, 10, 99, 100, 10000000000000000000ull, ~(u64)0, 7, 8};
    const std::string long_prefix(64, 'p');
    for (int format = EXPORT_LINES; format <= EXPORT_FASTQ; format++)
        for (int crlf = 0; crlf < 2; crlf++)
            for (u64 width : {0ull, 1ull, 2ull, 3ull, 7ull, 15ull, 16ull, 17ull, 60ull, 64ull, 65ull, 1000ull}) {
                if (format != EXPORT_FASTA && width)
                    continue;
                for (const std::string &prefix : {std::string(), std::string("r"), long_prefix}) {
                    char what[96];
                    snprintf(what, sizeof what, "format %d crlf %d width %llu prefix %zu", format, crlf, (unsigned long long)width,
                             prefix.size());
                    check_table(make_table(lens, numbers, prefix), format, crlf != 0, width, '#', what);
                }
            }

    // ---- random tables
    for (int it = 0; it < 50000 && bad == 0; it++) {
        const int format = 1 + (int)(rng() % 3);
        const bool crlf = rng() & 1;
        const u64 width = format == EXPORT_FASTA ? (rng() % 4 == 0 ? 0 : 1 + rng() % 24) : 0;
        const size_t n = 1 + (size_t)(rng() % 5);
        std::vector<u64> ls, nums;
        for (size_t i = 0; i < n; i++) {
            ls.push_back(rng() % 8 == 0 ? 0 : rng() % 4 == 0 ? 1 + rng() % 3 : rng() % 50);
            const unsigned bits = (unsigned)(rng() % 65);
            nums.push_back(bits == 0 ? 0 : rng() >> (64 - bits));
        }
        const std::string prefix(rng() % 3 == 0 ? 0 : (size_t)(rng() % 20), 'x');
        char what[96];
        snprintf(what, sizeof what, "random %d: format %d crlf %d width %llu", it, format, (int)crlf, (unsigned long long)width);
        check_table(make_table(ls, nums, prefix), format, crlf, width, 'I', what);
    }
    if (bad) {
        printf("%d mismatches\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
