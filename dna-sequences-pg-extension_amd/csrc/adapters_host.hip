// adapters_host.hip -- dnagpu_dna_adapters of include/dnagpu.h: the 3' adapter cut of the segments of a packed stream, with
// mismatches and IUPAC letters (adapters_kernels.hip).  The argument rules, the descriptors of the adapters,
// the order of the stages, the one read-back, the report.
#include "adapters_math.hpp"
#include "host_common.hpp"

using namespace dnagpu;

namespace {

struct AdaptersCaller {
    const u64 *seg_seq, *seg_first, *seg_len;    // seg_first / seg_len: both or none
    u64 n;
    int on_device;
    u64 *out_len, *out_adapter, *out_mismatch;   // per segment; any may be null
    u64 *pass_seq, *pass_first, *pass_len;       // pass_cap entries each; any may be null
    u64 pass_cap;
    int out_on_device;
};

int cut_segments(dnagpu_ctx *ctx, const dnagpu_dna *src, const std::vector<AdapterDesc> &ads, u64 min_bases, u32 flags,
                 const AdaptersCaller &c, dnagpu_adapters_report *report)
{
    const u64 n = c.n;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    prof_begin(ctx);
    prof_mark(ctx, "adapters_lists");
    AdapterSegs g = {nullptr, nullptr, src->seq_starts, n};
    const u64 *dseq = nullptr;
    RC_TRY(device_list(ctx, ps, c.seg_first, n, c.on_device, &g.first));
    RC_TRY(device_list(ctx, ps, c.seg_len, n, c.on_device, &g.len));
    RC_TRY(device_list(ctx, ps, c.seg_seq, n, c.on_device, &dseq));
    AdapterDesc *dads = nullptr;
    u64 *keys = nullptr;
    u32 *lists = nullptr, *counts = nullptr, *pass = nullptr, *rank = nullptr, *scan_tmp = nullptr;
    unsigned long long *res = nullptr;
    RC_TRY(ps.alloc(ads.size(), &dads));
    RC_TRY(ps.alloc((size_t)n, &keys));
    RC_TRY(ps.alloc((size_t)2 * n, &lists));
    RC_TRY(ps.alloc(2, &counts));
    RC_TRY(ps.alloc((size_t)n, &pass));
    RC_TRY(ps.alloc((size_t)n, &rank));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n), &scan_tmp));
    RC_TRY(ps.alloc(ADAPTERS_R_WORDS, &res));
    HIP_TRY(hipMemcpyAsync(dads, ads.data(), ads.size() * sizeof(AdapterDesc), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(res, 0, ADAPTERS_R_WORDS * sizeof *res, st));
    if (g.first)                                     // a caller's lists: every entry inside the stream (rank: scratch here)
        HIP_TRY(launch_take_segments(nullptr, nullptr, 0, g.first, g.len, src->n_bases, n, nullptr, rank, res, st));
    const unsigned long long *bad = res + ADAPTERS_R_BAD;
    const u64 cap = std::min(c.pass_cap, n);
    OutCols<3> cols, segs;
    RC_TRY(cols.init(ctx, ps, {c.out_len, c.out_adapter, c.out_mismatch}, n, c.out_on_device));
    RC_TRY(segs.init(ctx, ps, {c.pass_seq, c.pass_first, c.pass_len}, cap, c.out_on_device));
    prof_mark(ctx, "adapters_find");
    HIP_TRY(launch_adapters_find(src->words, g, dads, (u32)ads.size(), bad, keys, lists, counts, st));
    prof_mark(ctx, "adapters_verdict");
    HIP_TRY(launch_adapters_verdict(g, keys, min_bases, flags, cols.dev(0), cols.dev(1), cols.dev(2), pass, res, st));
    if (cap) {
        prof_mark(ctx, "adapters_segments");
        HIP_TRY(launch_scan_u32(pass, rank, n, scan_tmp, nullptr, st));
        HIP_TRY(launch_adapters_pass(g, dseq, keys, pass, rank, cap, bad, segs.dev(0), segs.dev(1), segs.dev(2), st));
    }
    prof_mark(ctx, "end");
    u64 got[ADAPTERS_R_WORDS] = {};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (the one read-back: the report; waits for the stream)
    prof_end(ctx);
    if (got[ADAPTERS_R_BAD]) {
        set_err("adapters: a segment leaves the stream of %llu bases", (unsigned long long)src->n_bases);
        return DNAGPU_ERR_BAD_ARG;
    }
    RC_TRY(cols.finish());
    RC_TRY(segs.finish(std::min(got[ADAPTERS_R_PASSED], cap)));
    if (report) {
        report->segments = n;
        report->passed = got[ADAPTERS_R_PASSED];
        report->trimmed = got[ADAPTERS_R_TRIMMED];
        report->bases_in = got[ADAPTERS_R_BASES_IN];
        report->bases_kept = got[ADAPTERS_R_BASES_KEPT];
        report->bases_cut = got[ADAPTERS_R_BASES_IN] - got[ADAPTERS_R_BASES_KEPT];
        report->failed_short = got[ADAPTERS_R_SHORT];
        report->failed_discarded = got[ADAPTERS_R_DISCARDED];
        for (u32 a = 0; a < ADAPTERS_MAX; a++)
            report->per_adapter[a] = got[ADAPTERS_R_ADAPTER + a];
    }
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_dna_adapters(dnagpu_ctx *ctx, const dnagpu_dna *src, const char *const *adapters, uint32_t n_adapters,
                                   const dnagpu_adapters_options *opt, const uint64_t *seg_seq, const uint64_t *seg_first,
                                   const uint64_t *seg_len, uint64_t n_segs, int on_device, uint64_t *out_len, uint64_t *out_adapter,
                                   uint64_t *out_mismatch, uint64_t *pass_seq, uint64_t *pass_first, uint64_t *pass_len,
                                   uint64_t pass_cap, int out_on_device, dnagpu_adapters_report *report)
{
    return guarded([&]() -> int {
    if (report)
        memset(report, 0, sizeof *report);
    if (!ctx || !src || !opt || !adapters)
        return DNAGPU_ERR_BAD_ARG;
    if (n_adapters < 1 || n_adapters > ADAPTERS_MAX)
        return DNAGPU_ERR_BAD_ARG;
    size_t len[ADAPTERS_MAX];
    for (u32 a = 0; a < n_adapters; a++) {
        if (!adapters[a])
            return DNAGPU_ERR_BAD_ARG;
        len[a] = strnlen(adapters[a], ADAPTERS_MAX + 1);
        if (len[a] < 1 || len[a] > ADAPTERS_MAX)
            return DNAGPU_ERR_BAD_ARG;
    }
    const u32 both = DNAGPU_ADAPTERS_DISCARD_UNTRIMMED | DNAGPU_ADAPTERS_DISCARD_TRIMMED;
    if (opt->err_den < 1 || opt->err_num > opt->err_den || opt->min_overlap < 1 || opt->min_overlap > ADAPTERS_MAX ||
        (opt->flags & ~both) || (opt->flags & both) == both || opt->reserved)
        return DNAGPU_ERR_BAD_ARG;
    std::vector<AdapterDesc> ads(n_adapters);
    for (u32 a = 0; a < n_adapters; a++) {
        int sets[ADAPTERS_MAX];
        for (size_t j = 0; j < len[a]; j++)
            if ((sets[j] = iupac_set(adapters[a][j])) < 0) {
                set_err("adapters: adapter %u holds a letter outside the qkmer alphabet", a);
                return DNAGPU_ERR_QKMER_INVALID;
            }
        adapter_build(sets, (u32)len[a], opt->err_num, opt->err_den, opt->min_overlap, &ads[a]);
    }
    if ((seg_first == nullptr) != (seg_len == nullptr))
        return DNAGPU_ERR_BAD_ARG;
    if (!seg_first && (table_without_set(src) || n_segs > src->n_seqs))
        return DNAGPU_ERR_BAD_ARG;                   // (segment i is sequence i of the set)
    if (n_segs > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    if (n_segs == 0)
        return DNAGPU_OK;
    static_assert(DNAGPU_ADAPTERS_DISCARD_UNTRIMMED == ADAPTERS_FLAG_UNTRIMMED && DNAGPU_ADAPTERS_DISCARD_TRIMMED == ADAPTERS_FLAG_TRIMMED,
                  "the flags of the header are the verdict's");
    const AdaptersCaller c = {seg_seq, seg_first, seg_len, n_segs, on_device, out_len, out_adapter, out_mismatch,
                              pass_seq, pass_first, pass_len, pass_cap, out_on_device};
    return cut_segments(ctx, src, ads, opt->min_bases, opt->flags, c, report);
    });
}

extern "C" int dnagpu_adapters_geometry(uint64_t *group_bases, uint64_t *wave_bases, uint64_t *tile_bases)
{
    if (!group_bases || !wave_bases || !tile_bases)
        return DNAGPU_ERR_BAD_ARG;
    *group_bases = ADAPTERS_GROUP_BASES;
    *wave_bases = ADAPTERS_WAVE_BASES;
    *tile_bases = ADAPTERS_TILE_BASES;
    return DNAGPU_OK;
}
