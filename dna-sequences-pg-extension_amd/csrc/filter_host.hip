// filter_host.hip -- the WHERE operators of include/dnagpu.h (`=`, `^@`, `@>`): the reference's operator semantics as
// device filters, generate_kmers fused with one of them over one sequence (dnagpu_generate_kmers_filtered) or over a table
// of sequences (dnagpu_generate_kmers_table), and the operator over a batch of keys (dnagpu_kmer_match).  The two fused
// calls check their own arguments and then run the same two sweeps (filter_kernels.hip).
#include "host_common.hpp"

using namespace dnagpu;

// ------------------------------------------------------------------------------------------------
// filters: reference operator semantics -> FilterDev
// IUPAC sets as 4-bit masks over codes (bit0 = A, bit1 = T, bit2 = C, bit3 = G), dna.c:1064-1081.
int dnagpu::iupac_set(char c)
{
    switch (c) {
    case 'A': return 0x1;
    case 'T': return 0x2;
    case 'C': return 0x4;
    case 'G': return 0x8;
    case 'U': return 0x0;   // compares the decoded base with 'U': never true (dna.c:1070)
    case 'W': return 0x3;
    case 'S': return 0xC;
    case 'M': return 0x5;
    case 'K': return 0xA;
    case 'R': return 0x9;
    case 'Y': return 0x6;
    case 'B': return 0xE;
    case 'D': return 0xB;
    case 'H': return 0x7;
    case 'V': return 0xD;
    case 'N': return 0xF;
    }
    return -1;
}

// Returns the error of a malformed filter.  *op_error: the operator's own ERROR (DNAGPU_OK when it has none), which the
// reference raises only when the operator is actually evaluated -- the caller returns it if a row reaches the operator;
// *out then matches nothing.
static int build_filter(const dnagpu_filter *f, int k, FilterDev *out, int *op_error)
{
    if (!f)
        return DNAGPU_ERR_BAD_ARG;
    FilterDev d;
    memset(&d, 0, sizeof d);
    *op_error = DNAGPU_OK;
    switch (f->kind) {
    case DNAGPU_FILTER_EQUALS:
        // kmer_eq_internal: lengths must be equal, then bits (dna.c:655-668)
        if (f->length != k) {
            d.and_mask = 0;
            d.eq_value = 1;                     // (key & 0) == 1: matches nothing
        } else {
            d.and_mask = ~(u64)0;
            d.eq_value = f->bits;
        }
        break;
    case DNAGPU_FILTER_STARTS_WITH:
        if (f->length < 0)
            return DNAGPU_ERR_BAD_ARG;
        if (f->length > k) {                    // dna.c:854-856
            *op_error = DNAGPU_ERR_PREFIX_TOO_LONG;
            d.and_mask = 0;
            d.eq_value = 1;
            break;
        }
        d.and_mask = kmer_mask(f->length);      // dna.c:862, defined for length 32 too
        if (f->length == 0)
            d.and_mask = 0;
        d.eq_value = f->bits;
        break;
    case DNAGPU_FILTER_CONTAINS: {
        size_t len = strnlen(f->pattern, sizeof f->pattern);
        if (len == 0 || len > 32)               // dna.c:877-886
            return DNAGPU_ERR_QKMER_INVALID;
        for (size_t i = 0; i < len; i++)
            if (iupac_set(f->pattern[i]) < 0)   // dna.c:888-896
                return DNAGPU_ERR_QKMER_INVALID;
        if ((int)len != k) {                    // dna.c:1106-1108
            *op_error = DNAGPU_ERR_QKMER_LEN_MISMATCH;
            d.and_mask = 0;
            d.eq_value = 1;
            break;
        }
        d.use_planes = 1;
        for (size_t i = 0; i < len; i++) {
            int set = iupac_set(f->pattern[i]);
            for (int c = 0; c < 4; c++)
                if (!(set & (1 << c)))
                    d.deny[c] |= (u64)1 << (2 * i);
        }
        break;
    }
    default:
        return DNAGPU_ERR_BAD_ARG;
    }
    *out = d;
    return DNAGPU_OK;
}

// no WHERE: N at every position
static FilterBits all_rows(int k)
{
    FilterBits fb;
    for (int q = 0; q < 4; q++)
        fb.sets[q] = 0xFFFFFFFFu;
    fb.k = k;
    return fb;
}

// The same operator as per-position sets for the bit-sliced stream kernels.  *none: no row can match
// (an `=` of another length, stray bits behind the right-hand kmer's length, a 'U' in the pattern, an operator that
// would raise *op_error).
int dnagpu::build_filter_bits(const dnagpu_filter *f, int k, FilterBits *out, bool *none, int *op_error)
{
    FilterDev fd;
    RC_TRY(build_filter(f, k, &fd, op_error));           // argument checks and the reference's ERRORs
    FilterBits fb = all_rows(k);
    *none = false;
    auto put = [&](int i, u32 set) { fb.sets[i >> 3] = (fb.sets[i >> 3] & ~(15u << ((i & 7) * 4))) | (set << ((i & 7) * 4)); };
    switch (f->kind) {
    case DNAGPU_FILTER_EQUALS:
    case DNAGPU_FILTER_STARTS_WITH: {
        const int len = f->length;
        if (fd.and_mask == 0 && fd.eq_value != 0) {      // build_filter's "matches nothing", or an empty prefix with bits
            *none = true;
            break;
        }
        if (len < 32 && len >= 0 && (f->bits >> (2 * len)) != 0) {
            *none = true;                                // bits behind the right-hand kmer's own length never compare equal
            break;
        }
        for (int i = 0; i < len && i < k; i++)
            put(i, 1u << ((f->bits >> (2 * i)) & 3));
        break;
    }
    case DNAGPU_FILTER_CONTAINS: {
        size_t len = strnlen(f->pattern, sizeof f->pattern);
        if ((int)len != k) {                             // (*op_error says why)
            *none = true;
            break;
        }
        for (int i = 0; i < k; i++) {
            int set = iupac_set(f->pattern[i]);
            if (set == 0)
                *none = true;                            // 'U' matches no base (dna.c:1070)
            put(i, (u32)set);
        }
        break;
    }
    }
    *out = fb;
    return DNAGPU_OK;
}

// ------------------------------------------------------------------------------------------------
// the two sweeps
static FilterSource source_of(const dnagpu_dna *dna, bool table)
{
    if (!table)
        return FilterSource{dna->words, dna->n_words, nullptr, 0, nullptr, 0};
    return FilterSource{dna->words, dna->n_words, dna->seq_marks, dna->n_mark_words, dna->seq_starts, dna->n_seqs};
}

// one count per group of the sweeps over `count` rows
static int alloc_groups(PoolScope &ps, u64 count, u32 *n_groups, u32 **group_counts)
{
    u32 tpg = 0;
    filter_bits_geometry(count, n_groups, &tpg);
    return ps.alloc((size_t)*n_groups, group_counts);
}

// the groups' counts through the mailbox to the host, summed; waits for the stream
static int sum_groups(dnagpu_ctx *ctx, const u32 *group_counts, u32 n_groups, u64 *total)
{
    static_assert(MAILBOX_BYTES >= FILTER_MAX_GROUPS * sizeof(u32), "mailbox holds one count per group");
    u32 *hc = reinterpret_cast<u32 *>(ctx->mailbox);
    HIP_TRY(hipMemcpyAsync(hc, group_counts, (size_t)n_groups * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *total = 0;
    for (u32 g = 0; g < n_groups; g++)
        *total += hc[g];
    return DNAGPU_OK;
}

// Rows [first, first + count) (count in [1, 2^32 - 1]) of src under fb: *n_out = the rows of the result, the first `cap` of
// them into the arrays of out[] that are not null (keys, sequences, positions / ordinals; see launch_filter_bits_write).
struct FilterJob {
    FilterSource src;
    u64 first, count;
    FilterBits fb;
    u64 *out[3];
    u64 cap;
    int out_on_device;
};

static int run_sweeps(dnagpu_ctx *ctx, const FilterJob &j, u64 *n_out)
{
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    u32 n_groups = 0, *group_counts = nullptr;
    RC_TRY(alloc_groups(ps, j.count, &n_groups, &group_counts));
    prof_begin(ctx);
    prof_mark(ctx, "filter_count");
    HIP_TRY(launch_filter_bits_count(j.src, j.first, j.count, j.fb, group_counts, ctx->stream));
    const bool want = j.cap > 0 && (j.out[0] || j.out[1] || j.out[2]);
    if (want && j.out_on_device) {
        // both sweeps queued back to back; the total arrives in the pinned mailbox
        prof_mark(ctx, "filter_write");
        HIP_TRY(launch_filter_bits_write(j.src, j.first, j.count, j.fb, group_counts, j.out[0], j.out[1], j.out[2], j.cap,
                                         ctx->mailbox, ctx->stream));
        prof_mark(ctx, "end");
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        prof_end(ctx);
        *n_out = ctx->mailbox[0];
        return DNAGPU_OK;
    }
    u64 total = 0;
    RC_TRY(sum_groups(ctx, group_counts, n_groups, &total));
    *n_out = total;
    const u64 nwrite = std::min<u64>(total, j.cap);
    if (nwrite == 0 || !want)
        return DNAGPU_OK;
    u64 *dev[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; i++)
        if (j.out[i])
            RC_TRY(ps.alloc((size_t)nwrite, &dev[i]));
    HIP_TRY(launch_filter_bits_write(j.src, j.first, j.count, j.fb, group_counts, dev[0], dev[1], dev[2], nwrite, nullptr,
                                     ctx->stream));
    for (int i = 0; i < 3; i++)
        if (j.out[i])
            HIP_TRY(hipMemcpyAsync(j.out[i], dev[i], nwrite * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
}

extern "C" int dnagpu_generate_kmers_filtered(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k,
                                              const dnagpu_filter *filter, uint64_t first, uint64_t count,
                                              uint64_t *out_keys, uint64_t *out_pos, uint64_t cap,
                                              uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_range(dna, k, first, count));
    FilterBits fb;
    bool none = false;
    int op_error = DNAGPU_OK;
    RC_TRY(build_filter_bits(filter, k, &fb, &none, &op_error));
    if (count > 0)
        RC_TRY(op_error);
    *n_out = 0;
    if (count == 0 || none)
        return DNAGPU_OK;
    if (count > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    return run_sweeps(ctx, FilterJob{source_of(dna, false), first, count, fb, {out_keys, nullptr, out_pos}, cap, out_on_device},
                      n_out);
    });
}

// The rows of a TABLE of sequences (FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) [WHERE ...],
// test.sql:140-150, 172-176): the same two sweeps with the in-one-sequence mask, every row labelled with its sequence and
// its ordinal inside it.
extern "C" int dnagpu_generate_kmers_table(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, const dnagpu_filter *filter,
                                           uint64_t first, uint64_t count, uint64_t *out_keys, uint64_t *out_seq,
                                           uint64_t *out_pos, uint64_t cap, uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_range(dna, k, first, count));
    if (table_without_set(dna))
        return DNAGPU_ERR_BAD_ARG;
    FilterBits fb = all_rows(k);
    bool none = false;
    int op_error = DNAGPU_OK;                      // raised only if a table row evaluates the operator
    if (filter)
        RC_TRY(build_filter_bits(filter, k, &fb, &none, &op_error));      // a malformed filter is always an error
    *n_out = 0;
    if (count == 0)
        return DNAGPU_OK;
    if (count > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    if (none && op_error == DNAGPU_OK)
        return DNAGPU_OK;
    const FilterSource src = source_of(dna, true);
    if (op_error != DNAGPU_OK) {
        // the reference raises the ERROR when the operator is first evaluated: on the window's first table row, if any
        HIP_TRY(hipSetDevice(ctx->device));
        PoolScope ps(ctx);
        u32 n_groups = 0, *group_counts = nullptr;
        RC_TRY(alloc_groups(ps, count, &n_groups, &group_counts));
        HIP_TRY(launch_filter_bits_count(src, first, count, all_rows(k), group_counts, ctx->stream));
        u64 rows = 0;
        RC_TRY(sum_groups(ctx, group_counts, n_groups, &rows));
        return rows ? op_error : DNAGPU_OK;
    }
    return run_sweeps(ctx, FilterJob{src, first, count, fb, {out_keys, out_seq, out_pos}, cap, out_on_device}, n_out);
    });
}

// ------------------------------------------------------------------------------------------------
// the operator over a batch of keys
extern "C" int dnagpu_kmer_match(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, int k,
                                 const dnagpu_filter *filter, uint8_t *flags, int on_device)
{
    return guarded([&]() -> int {
    if (!ctx || (n && (!keys || !flags)))
        return DNAGPU_ERR_BAD_ARG;
    if (k <= 0 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    FilterDev fd;
    int op_error = DNAGPU_OK;
    RC_TRY(build_filter(filter, k, &fd, &op_error));
    if (n == 0)
        return DNAGPU_OK;
    RC_TRY(op_error);
    HIP_TRY(hipSetDevice(ctx->device));
    if (on_device) {
        HIP_TRY(launch_match_batch(keys, n, fd, flags, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DNAGPU_OK;
    }
    PoolScope ps(ctx);
    u64 *dk = nullptr;
    uint8_t *df = nullptr;
    RC_TRY(ps.alloc((size_t)n, &dk));
    RC_TRY(ps.alloc((size_t)n, &df));
    HIP_TRY(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_match_batch(dk, n, fd, df, ctx->stream));
    HIP_TRY(hipMemcpyAsync(flags, df, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}
