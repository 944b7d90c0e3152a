// host_common.hpp -- what the host files of the C-ABI (dnagpu_api.hip, count_host.hip, sk_host.hip, multi_host.hip, query_host.hip,
// filter_host.hip, index_host.hip, join_host.hip, hits_host.hip, take_host.hip, profile_host.hip, seqeq_host.hip, text_host.hip, reads_host.hip, export_host.hip, quals_host.hip, names_host.hip, adapters_host.hip, host_steps.hip, table_steps.hip) share
// (internal, like kernels.hpp): the error macros, the context / dna / histogram objects, the buffer pool, and the few
// functions one of the files calls in another.  Declarations only, plus the templates and macros that must be visible;
// the definitions are in dnagpu_api.hip unless a section says otherwise.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>
#include <vector>

#include "../../include/dnagpu.h"
#include "kernels.hpp"

namespace dnagpu {
void set_err(const char *fmt, ...);

#ifdef DNAGPU_STAMPS
inline const char *diag_env(const char *name) { return getenv(name); }
#else
inline const char *diag_env(const char *) { return nullptr; }
#endif

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return e_ == hipErrorOutOfMemory ? DNAGPU_ERR_OOM : DNAGPU_ERR_HIP;              \
        }                                                                                    \
    } while (0)

#define RC_TRY(expr)           \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != DNAGPU_OK)  \
            return rc_;        \
    } while (0)

// No C++ exception may cross the C-ABI (a PostgreSQL backend would die in std::terminate): every
// extern "C" entry point that can allocate on the host (pool bookkeeping, event lists, node lists) runs its
// body inside this guard.
template <typename F>
int guarded(F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        set_err("host allocation failed");
        return DNAGPU_ERR_OOM;
    } catch (...) {
        set_err("unexpected C++ exception");
        return DNAGPU_ERR_INTERNAL;
    }
}

// ---------------------------------------------------------------- context + device buffer pool
struct PoolBlock {
    void *ptr;
    size_t size;
    bool in_use;
    size_t guard_at = 0;      // DNAGPU_DEBUG_GUARD_POOL: offset of the block's guard band (0 = none)
};
constexpr size_t POOL_GUARD = 256;               // bytes of 0xA5 behind the bytes a caller asked for

constexpr size_t MAILBOX_BYTES = (size_t)1 << 20;

}  // namespace dnagpu
using dnagpu::u32;
using dnagpu::u64;

struct dnagpu_ctx {
    int device;
    hipStream_t stream;
    std::vector<dnagpu::PoolBlock> pool;
    bool profiling;
    dnagpu_phase_times last_times;
    // per-call event list (profiling)
    std::vector<hipEvent_t> ev;
    std::vector<const char *> ev_names;
    // pinned, device-visible host words: small results (totals, per-group counts) land here without a
    // staging copy; read after hipStreamSynchronize
    u64 *mailbox;
    u64 mailbox_seq = 0;      // sequence number of the last flagged read-back (read_back)
    unsigned debug_flags;     // DNAGPU_DEBUG_*
    // A second stream of the context, for work that runs beside the main stream's inside ONE call (the record count:
    // level 1 beside level 0), and the events the two order themselves with.  Made on first use (side_stream), kept for
    // the life of the context.  Pool memory the side stream touches stays allocated until `stream` has waited for it.
    hipStream_t stream2 = nullptr;
    std::vector<hipEvent_t> sync_ev;
};

struct dnagpu_dna {
    u64 *words;
    u64 n_words;
    u64 n_bases;
    bool owned;
    // a TABLE of sequences (dnagpu_dna_set_sequences): where every sequence starts, resident beside the packed stream
    u64 *seq_starts = nullptr;    // n_seqs + 1 offsets (pool memory)
    u32 *seq_marks = nullptr;     // one bit per base, set where a sequence starts (pool memory)
    u64 n_seqs = 0, n_mark_words = 0;
};

struct dnagpu_hist {
    u64 *keys = nullptr;        // n_distinct groups, dense; stored leaf by leaf in completion order
    u32 *counts = nullptr;      // a count never exceeds the 2^32 - 1 rows of one call: 4 bytes in HBM, widened on download
    u64 n_distinct = 0;
    u64 total = 0;
    // segment directory: leaf l (leaves are in ascending key order) = seg_cnt[l] groups at seg_off[l]
    u64 *seg_off = nullptr;
    u32 *seg_cnt = nullptr;
    u32 *seg_pre = nullptr;     // exclusive scan of seg_cnt, built on first ordered download
    u32 n_segs = 0;
    bool sorted = true;         // the segments are consecutive key ranges (true unless the super-k-mer engine made them)
    u64 extent = 0;             // slots of keys / counts in use: n_distinct, or more when an unordered histogram holds count-0 padding
                                // between segments (0 = n_distinct)
    // A histogram made of several (dnagpu_hist_parts): the pipelined record exchange counts an owner's buckets group by
    // group, each group into arrays of its own.  The head then owns no arrays (keys == nullptr); n_distinct / total /
    // extent are the sums over the parts, the groups of part i come before those of part i + 1 in every ordered read.
    std::vector<dnagpu_hist *> parts;
    int k = 0;        // the k the rows were counted with (0 = unknown): dnagpu_hist_merge refuses two different ones
};
using HistPtr = std::unique_ptr<dnagpu_hist>;

namespace dnagpu {
// Up to 32 bytes from the host into device memory as a kernel argument: see Poke32 (dnagpu_api.hip)
hipError_t poke(void *dst, const void *src, size_t bytes, hipStream_t st);
// `bytes` of device memory to the host through the pinned mailbox; waits for the stream (dnagpu_api.hip: mailbox_kernel)
int read_back(dnagpu_ctx *ctx, void *host, const void *dev, size_t bytes);

int pool_alloc(dnagpu_ctx *ctx, size_t bytes, void **out);
// Buffers go back to the pool while kernels that use them may still be queued: every later user is
// queued on the same stream, behind them.
void pool_free(dnagpu_ctx *ctx, void *p);
// ctx->stream2 and at least n_events untimed events in ctx->sync_ev: created once per context, on first use
int side_stream(dnagpu_ctx *ctx, size_t n_events);

template <typename T>
int pool_alloc_t(dnagpu_ctx *ctx, size_t n, T **out)
{
    void *p = nullptr;
    int rc = pool_alloc(ctx, n * sizeof(T), &p);
    *out = static_cast<T *>(p);
    return rc;
}

// frees a set of pool buffers at scope exit
struct PoolScope {
    dnagpu_ctx *ctx;
    std::vector<void *> ptrs;
    explicit PoolScope(dnagpu_ctx *c) : ctx(c) {}
    ~PoolScope()
    {
        for (void *p : ptrs)
            pool_free(ctx, p);
    }
    template <typename T>
    int alloc(size_t n, T **out)
    {
        int rc = pool_alloc_t(ctx, n, out);
        if (rc == DNAGPU_OK)
            ptrs.push_back(*out);
        return rc;
    }
    void release(void *p)   // hand ownership to the caller
    {
        ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), p), ptrs.end());
    }
    void free_now(void *p)
    {
        release(p);
        pool_free(ctx, p);
    }
};

// An empty histogram of `total` rows, owned by the caller until it hands it out (release()); null when the host is out
// of memory.
HistPtr hist_new(u64 total, bool sorted = true);
// h takes the groups and their segment directory over from the scope that allocated them.
void hist_adopt(PoolScope &ps, dnagpu_hist *h, u64 *keys, u32 *counts, u64 *seg_off, u32 *seg_cnt, u32 n_segs, u64 n_distinct,
                bool sorted, u64 extent);
// hist_adopt for n_groups groups that are ONE segment: seg_off[0] = 0 and seg_cnt[0] = n_groups, twelve bytes of one pool
// block written by one poke.  (seg_cnt points into the block of seg_off: freeing it finds no block of its own and does
// nothing.)  Waits for the stream.
int hist_adopt_one_segment(dnagpu_ctx *ctx, PoolScope &ps, dnagpu_hist *h, u64 *keys, u32 *counts, u64 n_groups, bool sorted);

// ---------------------------------------------------------------- profiling helpers
void prof_begin(dnagpu_ctx *ctx);
void prof_mark(dnagpu_ctx *ctx, const char *name);
void prof_end(dnagpu_ctx *ctx);      // names[i] labels the interval [mark i, mark i+1)

// ---------------------------------------------------------------- dna
inline u64 words_for(u64 n_bases) { return (n_bases + 31) / 32; }
// the words of seq_marks over a stream of n_bases bases: what every reader of the marks is handed as n_mark_words
inline u64 table_mark_words(u64 n_bases) { return n_bases / 32 + 3; }
// bases but no set: no dnagpu_dna_set_sequences before.  (An empty stream without a set is a table of no sequence.)
inline bool table_without_set(const dnagpu_dna *dna) { return dna->n_seqs == 0 && dna->n_bases != 0; }
// validates [first, first+count) against the row count of generate_kmers(dna, k)
int check_range(const dnagpu_dna *dna, int k, u64 first, u64 count);

// ---------------------------------------------------------------- host_steps.hip
// The host-side steps that several features drive the same way: the LSD pair sort, the scan with its total, the count half
// of a stable select, the hand-out of u64 columns, a caller's list as device memory.  (Hidden: steps of the host files, not
// symbols of the library.)
#pragma GCC visibility push(hidden)
constexpr u64 U32_MAX64 = 0xFFFFFFFFull;

// `count` entries of a caller's list as device memory: the list itself (null stays null), or a copy in pool memory of ps
template <typename T>
int device_list(dnagpu_ctx *ctx, PoolScope &ps, const T *list, u64 count, int on_device, const T **dev)
{
    *dev = list;
    if (!list || on_device)
        return DNAGPU_OK;
    T *copy = nullptr;
    RC_TRY(ps.alloc((size_t)count, &copy));
    HIP_TRY(hipMemcpyAsync(copy, list, (size_t)count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *dev = copy;
    return DNAGPU_OK;
}

// The stable LSD radix sort of n >= 1 (key, value) pairs by `passes` 8-bit digits of the key, ping-pong between the caller's
// buffer pairs (key[b], val[b]), n entries each.  src = what the first pass reads: the caller's keys (src.keys != null: no
// pair exists yet, the first scatter forms them in pair 0), or the pairs in pair 0.  A pass whose digit takes one value
// moves nothing and is skipped -- but the last pass runs if nothing has formed the pairs yet (a column of one key).
// *sorted = the pair that holds the result.  One 4-byte read-back per pass; every pass is labelled `mark` unless it is null
// (the caller has called prof_begin).  The histogram and its scratch are gone when this returns.
int lsd_sort_pairs(dnagpu_ctx *ctx, IndexSortSrc src, u64 n, int passes, u64 *const key[2], u32 *const val[2], const char *mark,
                   int *sorted);

// arr[0 .. n) scanned in place (exclusive), the sum in arr[n] and, read back, in *total.  Waits.
int scan_total(dnagpu_ctx *ctx, u32 *arr, u64 n, u32 *scan_tmp, u32 *total);

// The count half of a stable select over nt tiles: *tiles (nt + 1 words of ps) = what count_launch(tiles) counted per tile,
// scanned into every tile's first output slot; *total = how many are selected.  Waits.
template <typename F>
int select_tiles(dnagpu_ctx *ctx, PoolScope &ps, u32 nt, F &&count_launch, u32 **tiles, u32 *total)
{
    u32 *scan_tmp = nullptr;
    RC_TRY(ps.alloc((size_t)nt + 1, tiles));               // (the last word: the total)
    RC_TRY(ps.alloc((size_t)scan_tmp_words(nt), &scan_tmp));
    HIP_TRY(count_launch(*tiles));
    return scan_total(ctx, *tiles, nt, scan_tmp, total);
}

// n words of every device array to its `out` (null: not wanted), host memory or device memory; waits for the stream
struct ColCopy {
    const u64 *dev;
    u64 *out;
};
int copy_cols(dnagpu_ctx *ctx, const ColCopy *cols, int n_cols, u64 n, int out_on_device);
inline int copy_cols(dnagpu_ctx *ctx, std::initializer_list<ColCopy> cols, u64 n, int out_on_device)
{
    return copy_cols(ctx, cols.begin(), (int)cols.size(), n, out_on_device);
}

// N optional u64 output columns of n_write entries each: the caller's arrays (null: not wanted) in host memory, or in
// device memory when out_on_device.  dev(i) = where a kernel writes column i: the caller's pointer, or a staging buffer of
// ps (null stays null).  finish() copies the staged columns to the host and waits for the stream.
template <int N>
struct OutCols {
    dnagpu_ctx *ctx = nullptr;
    u64 n_write = 0;
    u64 *out[N] = {}, *col[N] = {};
    int on_device = 0;

    int init(dnagpu_ctx *c, PoolScope &ps, std::initializer_list<u64 *> outs, u64 n, int out_on_device)
    {
        ctx = c;
        n_write = n;
        on_device = out_on_device;
        std::copy(outs.begin(), outs.end(), out);
        for (int i = 0; i < N; i++) {
            col[i] = on_device ? out[i] : nullptr;
            if (!on_device && out[i] && n)
                RC_TRY(ps.alloc((size_t)n, &col[i]));
        }
        return DNAGPU_OK;
    }
    u64 *dev(int i) const { return col[i]; }
    int finish(u64 n) const                                // (the first n <= n_write entries)
    {
        ColCopy c[N];
        for (int i = 0; i < N; i++)
            c[i] = ColCopy{col[i], on_device ? nullptr : out[i]};
        return copy_cols(ctx, c, N, n, 0);
    }
    int finish() const { return finish(n_write); }
};

// n entries of a u32 device array widened to u64 at `out` (host memory, or device memory; null: nothing).  Queued only.
int widen_out(dnagpu_ctx *ctx, PoolScope &ps, const u32 *src, u64 n, u64 *out, int out_on_device);
#pragma GCC visibility pop

// ---------------------------------------------------------------- table_steps.hip
// The host-side steps that the calls which make a resident table, or a column beside one, drive the same way: the hand-over
// of a new table, the starts and marks of a caller's boundaries, the segment plan of take / gather, and the front end of the
// text loaders.  (Hidden, like the steps above.)
#pragma GCC visibility push(hidden)
// A table being made.  It owns the scope of the call that makes it: everything allocated from ps goes back to the pool when
// the call returns, except what hand_over (or empty) has passed to the caller.
struct NewTable {
    PoolScope ps;
    std::unique_ptr<dnagpu_dna> h;
    explicit NewTable(dnagpu_ctx *ctx) : ps(ctx) {}
    // *out = a valid table of 0 bases with no set (one word): what dnagpu_dna_upload makes of 0 bases
    int empty(dnagpu_dna **out);
    // n_seqs + 1 starts, the marks and max(words, 1) stream words of n_bases bases, allocated in that order; a block that the
    // caller already has in ps (starts, words) is adopted instead.  Nothing of it is assumed zero.
    int alloc(u64 n_seqs, u64 n_bases, u64 *starts = nullptr, u64 *words = nullptr);
    int queue_marks(hipStream_t st);                 // launch_batch_marks over h->seq_starts; queued only
    void hand_over(dnagpu_dna **out);                // the three blocks leave ps; the caller has waited for the stream
};

// n_seqs + 1 starts from the host into ps memory and the marks of a stream of n_bases bases beside them.  Waits (the
// caller's array is not kept behind the call).
int starts_and_marks(dnagpu_ctx *ctx, PoolScope &ps, const u64 *host_starts, u64 n_seqs, u64 n_bases, u64 **starts, u32 **marks,
                     u64 *n_mark_words);

// The two faces of take / gather.  ids != nullptr: take (segment i = sequence ids[i] of the source's set); else gather
// (first / len).  All the lists are host memory, or device memory when on_device.
struct TakeLists {
    const u64 *ids;
    const u64 *first, *len;
    const uint8_t *flip;              // may be null
    u64 n;
    int on_device;
};
// What the copy kernel of a take reads, in memory of ps: where every segment begins in the source, the flips (null: none),
// the n + 1 starts of the result, and its bases.
struct TakePlan {
    const u64 *seg_first;
    const uint8_t *flip;
    u64 *starts;                      // written by queue_starts
    u64 total;
    u32 *len32, *scan_tmp;            // the lengths of the n segments, and the scratch of their scan
    u64 n;
    int queue_starts(dnagpu_ctx *ctx) const;         // phase "take_starts": the scan and the starts; queued only
};
// The plan of in.n >= 1 segments over a source of n_seqs sequences (seq_starts; take only) and stream_bases bases: the lists
// on the device, validated and summed in one pass (one read-back: it waits, the caller's host lists have been read).
// BAD_ARG with its text for an id >= n_seqs or a segment that leaves the stream, TOO_LARGE for more than 2^32 - 1 bases.
// Phases: lists_mark, "take_segments" (the caller has called prof_begin).  The caller allocates its result, then queues the
// starts.
int take_plan(dnagpu_ctx *ctx, PoolScope &ps, const TakeLists &in, const u64 *seq_starts, u64 n_seqs, u64 stream_bases,
              const char *lists_mark, TakePlan *plan);

// A report of a text loader as it is before anything is known
template <typename R>
void report_clear(R *r)
{
    if (!r)
        return;
    memset(r, 0, sizeof *r);
    r->bad_pos = ~(u64)0;
    r->bad_record = ~(u64)0;
}

// FASTA: the state every tile begins in, and the per-tile words that launch_text_finish reads.  The caller sets sw.text,
// sw.lim, sw.n_tiles and sw.res.  before_sweep (phase "text_heads"): the eight per-tile arrays, launch_text_heads and its two
// maximum scans; the caller's sweep then writes sw.last_seq, sw.first_header and sw.seq_before.  after_sweep: the maximum
// scan of last_seq and launch_text_finish.
struct FastaTiles {
    TextSweep sw = {};
    u32 *last_header = nullptr, *seq_before_t = nullptr;
    int before_sweep(dnagpu_ctx *ctx, PoolScope &ps);
    int after_sweep(hipStream_t st) const;
};

// Where an error word points, for the launch that ranks its byte: rec_t = the scanned records per tile (LINES, FASTA),
// nl_base = the '\n' before every tile (FASTQ)
struct TextErrorIn {
    const unsigned char *text;
    u64 n;
    const u64 *lim;
    int format;                       // TEXT_FORMAT_*
    const u32 *rec_t, *nl_base;
};
// who = {the record of the byte at pos, the byte, FASTQ: the role of its line}.  One launch, one read-back.
int text_error_rank(dnagpu_ctx *ctx, PoolScope &ps, const TextErrorIn &in, u64 pos, u64 who[3]);
struct TextBad {
    u64 pos, record;
    char byte;                        // 0 unless the error is an invalid character
    int code;
};
// after the error word `word` of a sweep: where it is, dnagpu_last_error() and the code (the reference's three messages;
// FASTQ: the truncated record, the missing '@' and '+')
int text_error_find(dnagpu_ctx *ctx, PoolScope &ps, const TextErrorIn &in, u64 word, TextBad *bad);
template <typename R>
int text_input_error(dnagpu_ctx *ctx, PoolScope &ps, const TextErrorIn &in, u64 word, R *report)
{
    TextBad bad = {};
    RC_TRY(text_error_find(ctx, ps, in, word, &bad));
    if (report) {
        report->bad_pos = bad.pos;
        report->bad_record = bad.record;
        report->bad_char = bad.byte;
    }
    return bad.code;
}
#pragma GCC visibility pop

// ---------------------------------------------------------------- filter_host.hip
// A WHERE operator as per-position sets, with the argument checks and the reference's ERRORs of every entry point that
// takes a dnagpu_filter (the fused extractions, the index scan of index_host.hip).  Returns the error of a malformed filter.
// *op_error: the operator's own ERROR, which the reference raises only when a row reaches the operator; *none: no row can
// match.
int build_filter_bits(const dnagpu_filter *f, int k, FilterBits *out, bool *none, int *op_error);
// a letter of the qkmer alphabet as a 4-bit mask over the codes (bit0 = A, bit1 = T, bit2 = C, bit3 = G; 'U': 0), else -1:
// the one routine that `@>` and the adapters of dnagpu_dna_adapters are validated by
int iupac_set(char c);

// ---------------------------------------------------------------- count_host.hip
struct TreeResult {
    Node *nodes;      // final node list (leaves, or the children of a forced level)
    u32 n_nodes;
    u32 n_big;        // leaves that sort more than LEAF_CAP_SMALL keys among them
    u32 n_small;      // leaves that sort up to LEAF_CAP_SMALL keys
    u32 n_tiny;       // leaves that sort at most LEAF_CAP_TINY keys (the rest: single-key or empty nodes)
    u64 n_keys;       // keys in the tree (== n unless an owner filter dropped some at the dna root)
    u64 *buf0;
    u64 *buf1;        // may be null if never needed
};

// Runs levels until every node is a leaf (force_bits == 0), or exactly one forced level of
// `force_bits` bits on the root (force_bits > 0).  dna != null: root over the packed sequence
// (keys land in buf0, allocated here); else root over keys_in (used as buf0).
// init_nodes != null: the levels start at `start_level` from that node list over keys_in (pool memory of `ps`; the
// nodes' key ranges need not share key bits: the super-k-mer engine enters here with its bucket nodes)
int run_tree(dnagpu_ctx *ctx, PoolScope &ps, const dnagpu_dna *dna, u64 first, u64 n, int k,
             u64 *keys_in, int force_bits, TreeResult *res, int fixed_bits = 0, u64 fixed_prefix = 0,
             bool single_level = true, u32 flt_lo = 0, u32 flt_span = ~0u, u32 flt_tb = 0,
             Node *init_nodes = nullptr, u32 init_n = 0, int start_level = 0);
// short k-mers (2k <= dense_max_bits()) of enough rows to pay for the table passes and for compacting the table: no tree
bool dense_pays(u64 n, int k);

// ---------------------------------------------------------------- sk_host.hip
// The record count.  What it shares with the other host files is below; its state (SkParts) and its stages -- level 0,
// the sk_l1_* stages of level 1, sk_level2, the sk_tail_* stages -- are local to sk_host.hip.
// DNAGPU_SK_SKEWED (from the census of level 1, sk_l1_census; nothing has moved yet): the set is too heavy for the record
// path (low-complexity input): count_sk hands it up and the caller counts with the ordinary tree instead, which has the
// skew paths; count_sk_received expands everything to keys.
constexpr int DNAGPU_SK_SKEWED = -1;
// geometry of a count of n rows: final buckets of ~SK_LEAF_MEAN k-mers = 16 per mid bucket; mid buckets = c0n coarse x 2^b1.
// A multi-GPU count derives it from the GLOBAL row count on every rank (the digits are part of the records).
struct SkGeom {
    int b1, r0bits;
    u32 c0n;
    u64 mid_limit;
};
SkGeom sk_geometry(const dnagpu_ctx *ctx, u64 n, int k);

// The rows a record count sweeps: [first, first + n) of dna's generate_kmers rows.  marks != null: a count over a TABLE
// of sequences -- one bit per base of the packed stream, set where a sequence starts (n_mark_words words, device memory);
// level 0 makes no record of rows that reach across a mark.
struct SkRows {
    const dnagpu_dna *dna;
    u64 first, n;
    const u32 *marks;
    u64 n_mark_words;
};

// rows.n = rows swept; n_kmers_expected = the k-mers they hold (fewer over a table of sequences: rows.marks)
int count_sk(dnagpu_ctx *ctx, const SkRows &rows, int k, dnagpu_hist *h, u64 n_kmers_expected);
// the records a landing buffer of the buckets blen[] should have room for, so that level 1 can run without its histogram
u64 sk_received_cap(const std::vector<u64> &blen, u32 n_coarse, const SkGeom &g);
// rec0 (pool memory; this takes it over and returns it to the pool) = the records of the coarse buckets, bucket after
// bucket: bucket d = blen[d] records at boff[d] (n_coarse = 2^r0bits entries).  Everything queued on ctx->stream
// behind whatever filled rec0.
int count_sk_received(dnagpu_ctx *ctx, void *rec0, const std::vector<u64> &boff, const std::vector<u64> &blen, const SkGeom &g,
                      int k, dnagpu_hist *h, u64 rec0_cap = 0);
}  // namespace dnagpu

// the k-mer accumulator (dnagpu_api.hip: dnagpu_acc_*; query_host.hip and join_host.hip read the table)
namespace dnagpu {
struct AccTable {
    u64 *table = nullptr;     // 2^pbits * ACC_SLOTS * {key, count}
    u32 *occ = nullptr;       // 2^pbits occupied-slot counts
    int pbits = 0;            // 0: no table yet
};
}  // namespace dnagpu

struct dnagpu_acc {
    int k;
    dnagpu::AccTable t;
    u64 distinct = 0, total = 0;
    std::vector<u64> pre;     // groups before each partition (+ the total): the download order, built after an add
    u64 *dev_pre = nullptr;
};

// per-sequence hits of a window of a table (hits_host.hip): a snapshot that depends on neither of its sources
struct dnagpu_seq_hits {
    u64 n = 0, first = 0;       // sequences of the window, and the first of them
    int k = 0;
    u32 *rows = nullptr;        // pool memory, n entries each (null when n == 0)
    u32 *hits = nullptr;
    u64 tot_rows = 0, tot_hits = 0, tot_seqs_hit = 0;
};

// the classes of equal sequences of a table (seqeq_host.hip).  It BORROWS the table: dnagpu_table_match compares against its bases.
struct dnagpu_seq_classes {
    const dnagpu_dna *table = nullptr;
    u64 n = 0, distinct = 0;    // sequences, classes
    u32 rounds = 0;             // verify rounds of the build
    u32 *rep = nullptr;         // pool memory, n entries each (null when n == 0): the smallest id of s's class, its size
    u32 *copies = nullptr;
    u64 *sfp = nullptr;         // the (fingerprint, id) pairs sorted by fingerprint, ids ascending inside a run
    u32 *sid = nullptr;
};

// the quality column of a table (quals_host.hip): one Phred+33 byte per base of the table's stream.  It holds no boundaries.
struct dnagpu_quals {
    unsigned char *bytes = nullptr;     // pool memory: whole 16-byte chunks, at least one
    u64 n = 0;
};

// the names column of a table (names_host.hip): one string per sequence, none of its bytes '\n' or '\r'
struct dnagpu_names {
    unsigned char *bytes = nullptr;     // pool memory: names_alloc_bytes(total) bytes
    u64 *off = nullptr;                 // pool memory: n + 1 offsets, off[0] = 0, off[n] = total
    u64 n = 0, total = 0;
};

struct dnagpu_records {
    void *recs = nullptr;       // pool memory: 16 bytes per record, bucket after bucket
    std::vector<u64> off;       // n_buckets + 1 offsets (records)
};
