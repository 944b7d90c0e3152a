// kernels.hpp -- host-callable launchers of the gfx950 kernels (internal; the public surface is
// include/dnagpu.h).  Every launcher enqueues on `stream` and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "export_math.hpp"
#include "kmer_device.hpp"

namespace dnagpu {

// ---------------------------------------------------------------- extract_kernels.hip
// words[w] of the synthetic sequence of n_bases bases for w in [w_begin, w_end) (words = the sequence's word 0)
hipError_t launch_synth(u64 *words, u64 w_begin, u64 w_end, u64 n_bases, u64 seed, u64 motif_len, hipStream_t s);
hipError_t launch_extract(const u64 *words, u64 n_words, u64 first, u64 count, int k, u64 *out_keys,
                          hipStream_t s);

// position-ordered filtered extraction (filter_kernels.hip), two sweeps over the (tiny) packed input:
//   count sweep -> rows of the result per workgroup range (filter_bits_geometry groups, group_counts[g]);
//   write sweep -> every group sums the counts before it, then writes the rows whose output index is < cap;
//   *total_out (may be null, may be host-mapped memory) receives the number of rows of the result
// One sequence (marks == nullptr): the rows that match, each with its key and its position (out_seq must be null).
// A TABLE of sequences (marks / seq_starts: what dnagpu_dna_set_sequences keeps resident): only stream rows that lie
// inside one sequence, in ascending stream position, each with its key, its sequence (0-based) and its ordinal inside
// that sequence.  Any of the arrays may be null.  k = fb.k.
constexpr int FILTER_MAX_GROUPS = 8192;
struct FilterSource {
    const u64 *words;
    u64 n_words;
    const u32 *marks;
    u64 n_mark_words;
    const u64 *seq_starts;
    u64 n_seqs;
};
void filter_bits_geometry(u64 count, u32 *n_groups, u32 *tiles_per_group);
hipError_t launch_filter_bits_count(const FilterSource &src, u64 first, u64 count, const FilterBits &fb, u32 *group_counts,
                                    hipStream_t s);
hipError_t launch_filter_bits_write(const FilterSource &src, u64 first, u64 count, const FilterBits &fb,
                                    const u32 *group_counts, u64 *out_keys, u64 *out_seq, u64 *out_pos, u64 cap,
                                    u64 *total_out, hipStream_t s);

hipError_t launch_hash_batch(const u64 *keys, u64 n, u32 *out, hipStream_t s);
hipError_t launch_match_batch(const u64 *keys, u64 n, const FilterDev &f, uint8_t *flags, hipStream_t s);
// result[0] += sum(count), result[1] += #(count == 1), result[2] += sum(pair_mix); zero it first
hipError_t launch_hist_summary(const u64 *keys, const u32 *counts, u64 n, u64 *result3, hipStream_t s);

// text <-> packed forms.  *bad_pos must hold ~0 before launch_pack; afterwards the position of the first
// character that is not A/T/C/G (or still ~0)
hipError_t launch_pack(const unsigned char *text, u64 n_bases, u64 *words, u64 *bad_pos, hipStream_t s);
hipError_t launch_unpack(const u64 *words, u64 first, u64 count, unsigned char *text, hipStream_t s);
hipError_t launch_kmers_to_text(const u64 *keys, u64 n, int k, unsigned char *text, hipStream_t s);
// dst[i] = bswap64(src[i]); the last word is ANDed with last_mask (wire <-> packed words)
hipError_t launch_wire_swap(const u64 *src, u64 *dst, u64 n_words, u64 last_mask, hipStream_t s);

// ---------------------------------------------------------------- strand_kernels.hip
// out[0 .. ceil(count / 32)) = bases [first, first + count) of words, reverse-complemented; bits behind the last base zero;
// no word outside [first / 32, ceil((first + count) / 32)) is read
hipError_t launch_dna_revcomp(const u64 *words, u64 first, u64 count, u64 *out, hipStream_t s);
// out[i] = rc(keys[i]) (canonical == 0) or the canonical form of keys[i], bits above 2k dropped; flipped (may be null):
// flipped[i] = out[i] != the masked key.  out == keys allowed.
hipError_t launch_kmer_strand(const u64 *keys, u64 n, int k, int canonical, u64 *out, uint8_t *flipped, hipStream_t s);

// exclusive scan of n u32 values (in != out allowed, in == out allowed); *total receives the sum.
// tmp must hold scan_tmp_words(n) u32 values.
u64 scan_tmp_words(u64 n);
// up to six exclusive scans of the same length n in three launches: in[a] -> out[a] (in == out allowed), *total[a] = the
// sum (may be null); tmp holds n_arrays x scan_tmp_words(n) words
constexpr int SCAN_SET_MAX = 6;
struct ScanSet {
    const u32 *in[SCAN_SET_MAX];
    u32 *out[SCAN_SET_MAX];
    u32 *total[SCAN_SET_MAX];
    u32 *tmp;
};
hipError_t launch_scan_u32_multi(const ScanSet &set, int n_arrays, u64 n, hipStream_t s);
hipError_t launch_scan_u32(const u32 *in, u32 *out, u64 n, u32 *tmp, u32 *total, hipStream_t s);

// ---------------------------------------------------------------- count_kernels.hip
// MSD radix tree over the keys (DESIGN.md "count"): every level splits the oversize nodes on their
// next most significant bits; leaves (<= LEAF_CAP keys, or no bits left) are sorted and run-length
// encoded in LDS, in key order, with a chained scan giving each leaf its output offset.
constexpr int LEAF_CAP = 6144;        // max keys a leaf workgroup sorts in LDS (48 KB of keys, six per thread)
constexpr int LEAF_CAP_TINY = 1024;   // leaves up to here take 256-thread workgroups (eight per CU)
constexpr int LEAF_CAP_SMALL = 4096;  // leaves up to here take the four-keys-per-thread kernel
constexpr int LEAF_TARGET = 5800;     // planned leaf size: a split aims at means in (2900, 5800]; a leaf that still exceeds LEAF_CAP is halved by one more level
constexpr int MAX_SPLIT_BITS = 10;    // widest digit of one level (1024 children)
constexpr int ROW_STRIDE = 1 << MAX_SPLIT_BITS;

struct Node {           // 32 bytes
    u32 start;          // index of the node's first key in its buffer (root over dna: 0)
    u32 len;            // keys in the node
    u32 meta;           // bits 0-7: remaining (not yet fixed) key bits; bit 8: buffer; bit 9: terminal
    u32 split;          // plan: digit width this level (0 = leaf)
    u64 prefix;         // the fixed high bits of every key in the node (low `rem` bits zero)
    u32 child_base;     // plan: index of the first child (or of the node itself) in the next list
    u32 chunk_base;     // plan: index of the node's first chunk
};
constexpr u32 NODE_BUF = 1u << 8;
constexpr u32 NODE_TERMINAL = 1u << 9;
constexpr u32 NODE_SKIP = 1u << 10;     // this level only: all keys share the digit, the scatter leaves the node where it is
constexpr u32 NODE_PEEL = 1u << 11;     // this level only: the node is split three ways around its dominant first key
// per node and key-source level (level_hist -> level_children -> peel_scatter): varying low bits, keys equal
// to the node's first key, cursors of the two moved parts of a peeled node
constexpr int NODE_STAT_WORDS = 8;

struct Chunk {          // 16 bytes: a contiguous piece of one node, the unit of work of a level
    u32 node;
    u32 off;            // offset inside the node
    u32 len;
    u32 pad;
};

struct LevelCounters {  // read back by the host once per level
    u32 n_next;         // nodes in the next list
    u32 n_chunks;
    u32 n_split;        // nodes being split this level
    u32 n_scatter;      // of which non-terminal (their keys move)
    u32 max_bits;       // widest split of this level
    u32 n_big;          // unsplit nodes that sort more than LEAF_CAP_SMALL keys (the six-keys-per-thread leaves kernel)
    u32 n_small;        // unsplit nodes that sort LEAF_CAP_TINY < keys <= LEAF_CAP_SMALL
    u32 n_tiny;         // unsplit nodes that sort at most LEAF_CAP_TINY keys; the rest are single-key or empty nodes
    u32 n_over;         // (levels >= 2) nodes over the leaf capacity, counted before the plan
};

hipError_t launch_plan(Node *nodes, u32 n_nodes, int level, u32 chunk_len, u32 *outc, u32 *nch,
                       LevelCounters *ctr, hipStream_t s, int skew_from = 2);
// plan + both scans + counters of a level (one launch for levels of at most 1024 nodes)
// skew_from: the first level at which an oversize node means skew and is fanned out wider than its size asks
hipError_t launch_plan_level(Node *nodes, u32 n_nodes, int level, u32 chunk_len, u32 *outc, u32 *nch, u32 *scan_tmp,
                             LevelCounters *ctr, hipStream_t s, int skew_from = 2);
hipError_t launch_fill_chunks(const Node *nodes, u32 n_nodes, u32 chunk_len, const u32 *child_base,
                              const u32 *chunk_base, Node *nodes_rw, Chunk *chunks, hipStream_t s);
// src_dna != 0: the (single) node being split is the root over the packed sequence; flt_lo/flt_span:
// owner filter on the root's digits ((d - lo) < span keeps a key; span = ~0 keeps all; tb > 0: lo/span are an
// aligned power-of-two range and only the digit's top tb bits need testing)
hipError_t launch_level_hist(const Node *nodes, const Chunk *chunks, u32 n_chunks, int src_dna,
                             const u64 *words, u64 n_words, u64 first, int k, const u64 *buf0,
                             const u64 *buf1, u32 *hist, u32 flt_lo, u32 flt_span, u32 flt_tb, u32 *vary, int multi_ref,
                             u32 stat_min_len, hipStream_t s);
// per split node and 64-digit group: chunk rows -> exclusive prefixes over chunks; per-digit totals
// into tot[row of the node's first chunk]
hipError_t launch_level_prefix(const Node *nodes, const Chunk *chunks, u32 n_chunks, u32 n_split_nodes, u32 chunk_len,
                               u32 *hist, u32 *tot, hipStream_t s, u32 n_nodes = 0);
// per node: leaf -> copied to the next list; split -> totals scanned over digits, children appended
// in digit (= key) order, tot row overwritten with each digit's absolute base
// vary (may be null): per node NODE_STAT_WORDS words -- the number of low key bits that vary inside it, keys below /
// equal to its first key -- as level_hist found (key-source levels); a node whose keys all share this level's digit is flagged NODE_SKIP and stays where it is
// (stat_min_len: the statistics exist for nodes of at least that many keys only)
hipError_t launch_level_children(Node *nodes, u32 n_nodes, u32 *tot, Node *next, u32 *vary, const u64 *buf0,
                                 const u64 *buf1, u32 stat_min_len, hipStream_t s);
// the chunks of nodes that level_children flagged NODE_PEEL (stat = the NODE_STAT_WORDS-per-node table)
hipError_t launch_peel_scatter(const Node *nodes, u32 n_nodes, const Chunk *chunks, u32 n_chunks, Node *next, u64 *buf0,
                               u64 *buf1, u32 *stat, hipStream_t s);
hipError_t launch_level_scatter(const Node *nodes, const Chunk *chunks, u32 n_chunks, int src_dna,
                                const u64 *words, u64 n_words, u64 first, int k, u64 *buf0, u64 *buf1,
                                const u32 *hist, const u32 *tot, u32 flt_lo, u32 flt_span, u32 flt_tb, u32 max_bits,
                                hipStream_t s);
// leaves -> (key, count) groups appended densely to out_keys/out_counts at offsets taken from *cursor
// (zeroed; holds the group count afterwards); seg_off/seg_cnt[l] = where leaf l landed.
// hashed: the groups of a leaf need no order -- leaves of at most LEAF_CAP_SMALL keys are counted in an LDS hash table
// (flags / scan_tmp / list are then always needed).
// n_tiny / n_small / n_big: leaves per sorting class; the other leaves hold one distinct key (or none) and are emitted
// in bulk; flags / scan_tmp / list (n_leaves + 1, scan_tmp_words(n_leaves) and n_leaves u32) are needed unless all
// nodes are sorting leaves of one class
hipError_t launch_leaves(const Node *leaves, u32 n_leaves, u32 n_tiny, u32 n_small, u32 n_big, const u64 *buf0, const u64 *buf1,
                         u64 *cursor, u64 *seg_off, u32 *seg_cnt, u64 *out_keys, u32 *out_counts, u32 *flags,
                         u32 *scan_tmp, u32 *list, hipStream_t s, bool hashed = false, u64 out_base = 0);
// (out_base: the value *cursor holds at the call -- the first output slot these leaves may use)
// dense count of short k-mers straight from the packed sequence (2k = bits <= dense_max_bits()): table must hold
// 2^bits u32 counters, out_keys/out_counts 2^bits entries; *n_out = distinct keys; results ascending
int dense_max_bits();
hipError_t launch_dense_count(const u64 *words, u64 n_words, u64 first, u64 count, int bits, u32 *table, u64 *out_keys,
                              u32 *out_counts, u64 *n_out, hipStream_t s);
// the two halves of it (a multi-GPU dense count sums the ranks' tables in between), and dst[i] += src[i]
hipError_t launch_dense_table(const u64 *words, u64 n_words, u64 first, u64 count, int bits, u32 *table, hipStream_t s);
hipError_t launch_dense_compact(const u32 *table, int bits, u64 *out_keys, u32 *out_counts, u64 *n_out, hipStream_t s);
hipError_t launch_table_add(u32 *dst, const u32 *src, u32 n, hipStream_t s);
// groups [first, first+count) of the ascending-key view -> dst arrays
hipError_t launch_gather_sorted(const u64 *seg_off, const u32 *seg_cnt, const u32 *seg_pre, u32 n_leaves,
                                u64 first, u64 count, const u64 *keys, const u32 *counts, u64 *dst_keys,
                                u64 *dst_counts, hipStream_t s);

// ---- dnagpu_hist_merge (extract_kernels.hip): groups (key, count; count 0 = padding) added into an open-addressing table of
// t_slots (a power of two) 8-byte keys (all ones = free) + 32-bit counts; the all-ones key's count goes to *ones.  Then the
// table's groups dense, in table order; *cursor (zeroed by the caller) ends as their number.
hipError_t launch_merge_insert(const u64 *keys, const u32 *counts, u64 n, u64 *tkeys, u32 *tcnt, u64 t_slots,
                               unsigned long long *ones, hipStream_t s);
hipError_t launch_merge_compact(const u64 *tkeys, const u32 *tcnt, u64 t_slots, u64 *out_keys, u32 *out_counts,
                                unsigned long long *cursor, hipStream_t s);

// ---- the k-mer accumulator (acc_kernels.hip): P = 2^pbits partitions of ACC_SLOTS 16-byte {key, u64 count} slots (count 0 =
// empty), occ[p] = occupied slots of partition p.  bin: every group of a histogram (count-0 padding skipped) into bins[p] of
// bin_cap 16-byte entries, cursor[p] (zeroed by the caller) = arrivals (entries past bin_cap are dropped, counted).
// bin_stats: stats[0] = max(occ + cursor), stats[1] = max(cursor) (stats zeroed by the caller).  merge: one workgroup per
// partition with arrivals; commit = 0 only counts the new keys (stats[0] = max(occ + new), stats[2..3] = sum of new as
// u64), commit = 1 adds the bins in LDS and writes the partitions back (stats[2..3] = new keys; stats[1] != 0: a partition
// ran full).  split: the table of 2^old_bits partitions into one of 2^new_bits.  gather: groups [first, first + count) of
// the partition-order view (pre[p] = groups before partition p) of partitions p_lo .. p_lo + n_parts - 1.
// The canonical add: canon_k != 0 makes bin store the canonical form of every key (strand_math.hpp, k =
// canon_k), in the partition of that form, with bit 63 of the entry's count word set when the key was flipped; merge with
// canonical != 0 takes such bins -- a key may then arrive twice, once from either strand -- and counts a pair that is new
// as ONE new key, in the dry run too.
constexpr int ACC_SLOTS = 4096;
hipError_t launch_acc_bin(const u64 *keys, const u32 *counts, u64 n, int pbits, u32 *cursor, u64 *bins, u32 bin_cap, int canon_k,
                          hipStream_t s);
hipError_t launch_acc_bin_stats(const u32 *occ, const u32 *cursor, u64 P, u32 *stats, hipStream_t s);
hipError_t launch_acc_merge(u64 *table, u32 *occ, u64 P, const u32 *cursor, const u64 *bins, u32 bin_cap, int commit, int canonical,
                            u32 *stats, hipStream_t s);
hipError_t launch_acc_split(const u64 *old_table, const u32 *old_occ, int old_bits, u64 *new_table, u32 *new_occ, int new_bits,
                            u32 *stats, hipStream_t s);
// res3[0] += sum(count), res3[1] += #(count == 1), res3[2] += sum(pair_mix(key, count)); zero it first
hipError_t launch_acc_summary(const u64 *table, const u32 *occ, u64 P, u64 *res3, hipStream_t s);
hipError_t launch_acc_gather(const u64 *table, const u32 *occ, const u64 *pre, u64 p_lo, u64 n_parts, u64 first, u64 count,
                             u64 *out_keys, u64 *out_counts, hipStream_t s);

// ---- the join of two accumulators (join_kernels.hip).  For every group of the left table (2^s partitions)
// the count of its key in the right table (2^t partitions; r_table == nullptr: right holds no table, t = 0, every row is a
// miss) decides whether it is a result row of `kind`.  Result rows are ranked by one returning atomic per workgroup on
// res[0]; row `at` is stored at out_*[at - out_base] when at < cap (any array may be null; out_base = what res[0] held
// when the launch was queued: the host reads a result larger than its staging buffers chunk by chunk).  res[0] += the result
// rows; res[1 ..] += sum_left, sum_right, sum_min, checksum_left, checksum_right over them (dnagpu_join_stats).
// Both launchers cover left's partitions [p_lo, p_lo + n_parts):
//   partition: one workgroup per partition of the finer side; right's partition in LDS, left's streamed past it
//   direct:    one workgroup per 2048 slots of left; every group probes right's table in global memory
constexpr int JOIN_KIND_INNER = 0, JOIN_KIND_ANTI = 1, JOIN_KIND_LEFT = 2;    // DNAGPU_JOIN_*
constexpr int JOIN_RES_WORDS = 6;
struct JoinArgs {
    const u64 *l_table;
    const u32 *l_occ;
    int s;
    const u64 *r_table;
    const u32 *r_occ;
    int t;
    int kind;
    u64 *out_keys, *out_left, *out_right;
    u64 cap, out_base;
    unsigned long long *res;
};
hipError_t launch_join_partition(const JoinArgs &a, u64 p_lo, u64 n_parts, hipStream_t st);
hipError_t launch_join_direct(const JoinArgs &a, u64 p_lo, u64 n_parts, hipStream_t st);

// ---- per-sequence hits of a table's k-mers in an accumulator (hits_kernels.hip; the layout of the scratch
// arrays is hits_math.hpp's).  The window is the stream bases [a0, a0 + n), n <= 2^32 - 1; row r is the k-mer at a0 + r.
struct HitsWindow {
    const u64 *words;
    u64 n_words;
    const u32 *marks;
    u64 n_mark_words;
    u64 a0, n;
    int k;
    int canonical;                    // probe with the canonical form of the row's key (strand_math.hpp)
};
struct HitsSet {                      // the accumulator's table (it must hold one) and the count bounds, lo >= 1
    const u64 *table;
    const u32 *occ;
    int pbits;
    u64 lo, hi;
    const u64 *idle;                  // 16 readable, 16-byte aligned bytes of no meaning: what a row that is not probed loads
};
struct HitsPredicate {
    u64 min_hits, max_hits, frac_num, frac_den;
};
// sweep: mask / word_pre (hits_mask_words(n) words each) and tile_tot (hits_tiles(n) words); a row that reaches across a mark
// is not probed and has no bit.  The caller scans tile_tot into tile_base (launch_scan_u32).
hipError_t launch_hits_sweep(const HitsWindow &w, const HitsSet &set, u32 *mask, u32 *word_pre, u32 *tile_tot, hipStream_t s);
// out2[0] = seq_starts[seq_first], out2[1] = seq_starts[seq_first + seq_count]
hipError_t launch_hits_bounds(const u64 *seq_starts, u64 seq_first, u64 seq_count, u64 *out2, hipStream_t s);
// starts = seq_starts + seq_first; out_rows / out_hits[i] for the window's sequence i; totals3 (zeroed by the caller) += the
// sums of rows, of hits, and the sequences with a hit.  mask == nullptr: nothing was swept, every sequence has 0 hits.
hipError_t launch_hits_gather(const u64 *starts, u64 seq_count, u64 a0, int k, const u32 *mask, const u32 *word_pre,
                              const u32 *tile_base, u32 *out_rows, u32 *out_hits, unsigned long long *totals3, hipStream_t s);
// the stable selection of the sequences that pass p (hits_math.hpp: hits_selected): count -> tile_counts[tile]
// (hits_select_tiles(n) tiles); write (tile_offsets = their exclusive scan) -> the matches in ascending sequence order,
// entries from cap on not stored, any array may be null; out_seq = seq_first + index
u32 hits_select_tiles(u64 n);
hipError_t launch_hits_select_count(const u32 *rows, const u32 *hits, u64 n, const HitsPredicate &p, u32 *tile_counts, hipStream_t s);
hipError_t launch_hits_select_write(const u32 *rows, const u32 *hits, u64 n, const HitsPredicate &p, const u32 *tile_offsets,
                                    u64 seq_first, u64 *out_seq, u64 *out_rows, u64 *out_hits, u64 cap, hipStream_t s);
hipError_t launch_hits_widen(const u32 *in, u64 *out, u64 n, hipStream_t s);

// ---- the k-mer profile of every sequence of a window of a table (profile_kernels.hip; classes and items are
// profile_math.hpp's).  starts = seq_starts + seq_first (seq_count + 1 entries), k in 1 .. 6, out = seq_count rows of 4^k u32.
// plan: out_rows[i] (may be null) = the rows of sequence i, items[i] = its item count (0: the wave class)
hipError_t launch_profile_plan(const u64 *starts, u64 seq_count, int k, u64 *out_rows, u32 *items, hipStream_t s);
// wave: writes every cell of every row of out -- the profile of a wave-class sequence, zeros for a tiled one
hipError_t launch_profile_wave(const u64 *words, u64 n_words, const u64 *starts, u64 seq_count, int k, int canonical, u32 *out,
                               hipStream_t s);
// tile (behind wave on the same stream): off = the exclusive scan of items[], n_items = its total; adds the counts of every
// item into its sequence's row
hipError_t launch_profile_tile(const u64 *words, u64 n_words, const u64 *starts, u64 seq_count, const u32 *off, u32 n_items, int k,
                               int canonical, u32 *out, hipStream_t s);

// ---- the gather of segments of a packed stream into a new one (take_kernels.hip; the piece arithmetic is
// take_math.hpp's).  segments: the list of n entries built and validated in one pass -- ids != nullptr: entry i is sequence
// ids[i] of the table (seq_starts, n_seqs), its first base goes to seg_first[i]; else entry i is (in_first[i], in_len[i]) of
// a stream of n_bases bases and seg_first is not written.  len32[i] = the entry's length, res2[0] = the sum of the lengths
// in 64 bits (each counted as at most 2^32), res2[1] != 0: an id >= n_seqs or a segment that leaves the stream (res2 is
// zeroed here).
hipError_t launch_take_segments(const u64 *ids, const u64 *seq_starts, u64 n_seqs, const u64 *in_first, const u64 *in_len,
                                u64 n_bases, u64 n, u64 *seg_first, u32 *len32, unsigned long long *res2, hipStream_t s);
// out_starts[0 .. n] from the exclusive scan of the lengths (n entries) and their total
hipError_t launch_take_starts(const u32 *scan, u64 n, u64 total, u64 *out_starts, hipStream_t s);
// the sweep: out[0 .. ceil(total / 32)) = the segments back to back, segment i = the out_starts[i + 1] - out_starts[i] bases at
// base seg_first[i] of src, reverse-complemented where seg_flip[i] != 0 (seg_flip may be null).  Every output word is
// stored once, whole; bits behind the last base are zero; no word of src is read that holds no base of a segment.
hipError_t launch_take_copy(const u64 *src, const u64 *seg_first, const uint8_t *seg_flip, const u64 *out_starts, u64 n, u64 total,
                            u64 *out, hipStream_t s);

// ---- a text file of sequences into a resident table (text_kernels.hip; the masks of a lane's bytes, the
// error word and the cut are text_math.hpp's).  All per-tile arrays have n_tiles = text_tiles(n_bytes) entries and are
// written whole; offsets stored per tile are offset + 1, 0 = none.
// *cut = where a chunk that more text follows is cut (text_is_cut): LINES one past the last '\n' or 0, FASTA the last
// header's '>' or n
hipError_t launch_text_cut(const unsigned char *text, u64 n, int format, u64 *cut, hipStream_t s);
// FASTA: per tile the last line start ((tile + 1) << 1 | it begins a header) and the last header
hipError_t launch_text_heads(const unsigned char *text, const u64 *lim, u32 n_tiles, u32 *last_start, u32 *last_header, hipStream_t s);
// out[i] = max(in[0 .. i)), out[0] = 0; n <= 2^19 + 1; in != out
hipError_t launch_text_max_scan(const u32 *in, u32 *out, u32 n, hipStream_t s);
struct TextSweep {
    const unsigned char *text;
    const u64 *lim;               // device: the bytes of text that count (res + 3)
    int format;                   // TEXT_FORMAT_*
    u32 n_tiles;
    const u32 *in_state;          // FASTA: max scan of last_start
    const u32 *header_before;     // FASTA: max scan of last_header
    u32 *keep_t, *rec_t;          // bases kept / records begun per tile; scanned in place before launch_text_pack
    u32 *last_seq, *first_header, *seq_before;      // FASTA, for launch_text_finish
    u64 *res;                     // res[0]: the minimum error word (text_error_key), TEXT_NO_ERROR before the launch
};
hipError_t launch_text_sweep(const TextSweep &a, hipStream_t s);
// FASTA: records without sequence whose two headers lie in different tiles, or that the end of the text closes
// (seq_before_t: max scan of a.last_seq)
hipError_t launch_text_finish(const TextSweep &a, const u32 *last_header, const u32 *seq_before_t, hipStream_t s);
// out2[0] = the record the byte at e belongs to (~0: before the first), out2[1] = the byte; rec_base = the scanned rec_t
hipError_t launch_text_rank(const unsigned char *text, const u64 *lim, int format, const u32 *rec_base, u64 e, u64 *out2, hipStream_t s);
// words[0 .. ceil(n_bases / 32)) (cleared here), starts[0 .. n_records], record_pos[0 .. min(n_records, record_cap)) (null:
// not wanted) from the scanned tile counts
hipError_t launch_text_pack(const TextSweep &a, u64 n_bases, u64 n_records, u64 *words, u64 *starts, u64 *record_pos, u64 record_cap,
                            hipStream_t s);

// ---- FASTQ and real FASTA into a resident table (reads_kernels.hip).  The per-tile arrays are as above;
// the stages in order: FASTQ launch_reads_newlines -> launch_scan_u32 -> launch_reads_fastq_cut (LINES / FASTA:
// launch_text_cut, launch_text_heads and its two maximum scans) -> launch_reads_sweep -> FASTA launch_text_finish, SPLIT the
// maximum scans of last_keep / last_brk and launch_reads_finish -> the additive scans, in place -> launch_reads_pack.
struct ReadsSweep {
    const unsigned char *text;
    const u64 *lim;               // device: the bytes of text that count (res + 3)
    int format;                   // TEXT_FORMAT_*
    int ambiguous;                // READS_AMBIG_*
    int fold;                     // DNAGPU_READS_FOLD_CASE
    u32 n_tiles;
    const u32 *in_state, *header_before;            // FASTA: as TextSweep's
    const u32 *line_base;                           // FASTQ: the '\n' before every tile
    u32 *keep_t, *rec_t;          // bases kept / records begun per tile
    u32 *last_seq, *first_header, *seq_before;      // FASTA, for launch_text_finish
    u32 *piece_t, *sc_t;          // SPLIT: piece starts / sequence characters per tile
    u32 *last_keep, *last_brk, *undecided;          // SPLIT: for launch_reads_finish
    const u32 *keep_before_t, *brk_before_t;        // SPLIT: the maximum scans of last_keep / last_brk
    u64 *res;                     // res[0]: the minimum error word, res[4]: += the ambiguity letters of sequence lines
};
struct ReadsPack {
    u64 n_bases, n_seqs, n_records;
    u64 *words, *starts;          // ceil(n_bases / 32) words (cleared by the launcher), n_seqs + 1 starts
    u64 *record_pos;              // null: not wanted
    u64 record_cap;
    u32 *rec_amb;                 // DROP: ambiguity letters per record, zero before the launch; else null
    u32 *rec_sc;                  // SPLIT: per record
    u64 *src_record, *src_offset; // SPLIT: per sequence
};
hipError_t launch_reads_newlines(const unsigned char *text, u64 n, u32 n_tiles, u32 *nl_t, hipStream_t s);
// *lim = the cut (more), or res[0] takes the truncated record's error word (not more, lines no multiple of four)
hipError_t launch_reads_fastq_cut(const unsigned char *text, u64 n, u32 n_tiles, const u32 *nl_t, const u32 *nl_base, const u32 *total,
                                  bool more, u64 *lim, u64 *res, hipStream_t s);
// out3 = {record of the byte at e, the byte, the role of its line}
hipError_t launch_reads_fastq_rank(const unsigned char *text, u64 n, const u32 *nl_base, u64 e, u64 *out3, hipStream_t s);
hipError_t launch_reads_sweep(const ReadsSweep &a, hipStream_t s);
hipError_t launch_reads_finish(const ReadsSweep &a, hipStream_t s);
hipError_t launch_reads_pack(const ReadsSweep &a, const ReadsPack &p, hipStream_t s);
hipError_t launch_reads_offsets(const u64 *src_record, u64 *src_offset, const u32 *rec_sc, u64 n, hipStream_t s);
hipError_t launch_reads_identity(u64 *src_record, u64 *src_offset, u64 n, hipStream_t s);
// flags[i] = sequence i stays; res2[0] += dropped for an ambiguity letter, res2[1] += shorter than min_bases
hipError_t launch_reads_select(const u64 *starts, const u32 *rec_amb, u64 n, u64 min_bases, u32 *flags, u64 *res2, hipStream_t s);
// rank: the scanned flags; len32: zero before the launch
hipError_t launch_reads_move(const u64 *starts, const u64 *src_record, const u64 *src_offset, const u32 *flags, const u32 *rank, u64 n,
                             u64 *seg_first, u32 *len32, u64 *src_record_out, u64 *src_offset_out, hipStream_t s);

// ---- a resident table as text (export_kernels.hip; the record arithmetic is export_math.hpp's).
// the plan: ex32[s] = the bytes of record s that are no bases of a sequence line (clamped to 2^32 - 1), res2[0] = their sum
// in 64 bits, res2[1] = the sequences of 0 bases (res2 is zeroed here).  numbers may be null: the number of s is name_base + s
hipError_t launch_export_plan(const u64 *starts, u64 n, const u64 *numbers, u64 name_base, const ExportFmt &f, u32 *ex32,
                              unsigned long long *res2, hipStream_t s);
// pos[0 .. n] = where every record begins, from the exclusive scan of ex32 and its total; pos[n] = the image's bytes
hipError_t launch_export_pos(const u64 *starts, const u32 *scan, u64 n, u64 total, u64 *pos, hipStream_t s);
// the sweep: dst[0 .. count) = bytes [first_byte, first_byte + count) of the image; dst at any byte alignment; no byte of
// dst outside them is written or read; no word of words at or beyond n_words is read
struct ExportRead {
    const u64 *words;
    u64 n_words, n_bases;
    const u64 *starts, *pos, *numbers;       // n + 1, n + 1, n (or null) entries
    const unsigned char *prefix;             // fmt.prefix_len bytes of device memory
    u64 n, name_base;
    ExportFmt fmt;
    u64 first_byte, count;
    unsigned char *dst;
};
hipError_t launch_export_read(const ExportRead &a, hipStream_t s);
// the named image (dnagpu_table_to_text_named): the header of record s is its marker and bytes [off[s],
// off[s + 1]) of a names column, whose allocation reaches NAMES_SLACK bytes behind its last byte.  The plan and the sweep are
// the bodies of the two above; a.numbers, a.prefix and a.name_base are not looked at.
struct ExportNames {
    const unsigned char *bytes;
    const u64 *off;                          // n + 1 entries
};
hipError_t launch_export_plan_named(const u64 *starts, u64 n, const u64 *name_off, const ExportFmt &f, u32 *ex32,
                                    unsigned long long *res2, hipStream_t s);
hipError_t launch_export_read_named(const ExportRead &a, const ExportNames &names, hipStream_t s);

// ---- the names column of a table (names_kernels.hip; the arithmetic is names_math.hpp's).
// the sweep over a text: mask[c] = the bytes of chunk c (TEXT_CHUNK bytes) that end a name -- '\n', and with first_word
// blank and tab --, tile_first[t] = the offset of the first of them in tile t (NAMES_NONE: none); res[NAMES_R_LONE_CR] |= 1
// where a '\r' is not followed by '\n'
hipError_t launch_names_ends(const unsigned char *text, u64 n, u32 n_tiles, bool first_word, u32 *mask, u32 *tile_first,
                             unsigned long long *res, hipStream_t s);
// the suffix minimum of tile_first in groups of NAMES_GROUP_TILES tiles: local[t] = the minimum over tile t and the tiles
// behind it in its group, after[g] = the minimum over the groups behind group g.  group_min: names_groups(n_tiles) words.
hipError_t launch_names_suffix_min(const u32 *tile_first, u32 n_tiles, u32 *local, u32 *group_min, u32 *after, hipStream_t s);
// one thread per sequence: first[s] / len32[s] = where its name lies in the text; res[NAMES_R_TOTAL] += the lengths,
// res[NAMES_R_BAD] |= 1 for a record_pos that is not the marker's inside the text or a src_record >= n_records (null:
// sequence s is record s)
struct NamesSpans {
    const unsigned char *text;
    u64 n;
    u32 n_tiles;
    u32 marker;
    const u32 *mask, *local, *after;
    const u64 *record_pos, *src_record;
    u64 n_records, n_seqs;
    u64 *first;
    u32 *len32;
    unsigned long long *res;
};
hipError_t launch_names_spans(const NamesSpans &a, hipStream_t s);
// a caller's n + 1 offsets: res[NAMES_R_BAD] |= 1 unless off[0] == 0 and no pair decreases, res[NAMES_R_TOTAL] = off[n]
hipError_t launch_names_offsets_check(const u64 *off, u64 n, unsigned long long *res, hipStream_t s);
// res[0] takes the minimum offset of a '\n' or '\r' in the total bytes at col (NAMES_NO_ERROR before the launch: none)
hipError_t launch_names_validate(const unsigned char *col, u64 total, unsigned long long *res, hipStream_t s);
// out3 = {the sequence whose name holds column byte pos, first[s] + its offset inside the name, src_record[s] (or s)}
hipError_t launch_names_locate(const u64 *off, u64 n, u64 pos, const u64 *first, const u64 *src_record, u64 *out3, hipStream_t s);

// ---- the quality column of a table (quals_kernels.hip; the byte arithmetic is quals_math.hpp's).
// col: a caller's n bytes in a column's allocation (whole 16-byte chunks); res[0] takes the minimum of the error words
hipError_t launch_quals_validate(unsigned char *col, u64 n, unsigned long long *res, hipStream_t s);
// FASTQ: rec[4 r ..] = start and end of the sequence line and of the quality line of every whole record (nl_base: the
// scanned launch_reads_newlines counts, *total their sum); res[0] takes the error words of the quality lines' bytes, and
// launch_quals_lengths adds those of the lengths, one thread per record of the records_cap that rec has room for
hipError_t launch_quals_lines(const unsigned char *text, u64 n, u32 n_tiles, const u32 *nl_base, const u32 *total, u32 *rec,
                              unsigned long long *res, hipStream_t s);
hipError_t launch_quals_lengths(const unsigned char *text, u64 n, const u32 *total, const u32 *rec, u64 records_cap,
                                unsigned long long *res, hipStream_t s);
// src_at[s] = the text's byte where the qualities of sequence s begin; res[1] = the records, res[2] |= 1 on a bad source
hipError_t launch_quals_sources(const unsigned char *text, u64 n, const u32 *total, const u32 *rec, const u64 *starts, u64 n_seqs,
                                const u64 *src_record, const u64 *src_offset, u64 *src_at, unsigned long long *res, hipStream_t s);
// out[0 .. total) = segment i's bytes src[src_at[i] ..) (backwards where seg_flip[i]) at out_starts[i]; out holds whole
// 16-byte chunks; no byte of src outside [0, src_n) is read
hipError_t launch_quals_copy(const unsigned char *src, u64 src_n, const u64 *src_at, const uint8_t *seg_flip, const u64 *out_starts,
                             u64 n, u64 total, unsigned char *out, hipStream_t s);
// dst[0 .. count) = bytes [first, first + count) of a FASTQ image as launch_export_read left them: the bytes of quality
// lines become the column's; dst at any byte alignment; no byte of dst outside them is written or read
hipError_t launch_quals_overlay(const unsigned char *quals, const u64 *starts, const u64 *pos, u64 n, u32 term, u64 first,
                                u64 count, unsigned char *dst, hipStream_t s);
// the trim: first / len / qsum / low[s] (none null) = the kept range of every sequence as a stream coordinate and a length,
// the sum of its Phred values and its bases below low_q.  lists: 2 n_seqs words, counts2: 2 words (scratch: the longer
// sequences by class).  Three launches: groups of lanes, waves, workgroups.
struct QualsTrimOpt;
hipError_t launch_quals_trim(const unsigned char *col, const u64 *starts, u64 n_seqs, const QualsTrimOpt &o, u64 *first, u64 *len,
                             u64 *qsum, u64 *low, u32 *lists, u32 *counts2, hipStream_t s);
// flags[s] = sequence s passes; res7 = {passed, bases kept, cut in front, cut at the tail, failed short, mean, low} (zeroed here)
hipError_t launch_quals_verdict(const u64 *starts, u64 n_seqs, const QualsTrimOpt &o, const u64 *first, const u64 *len, const u64 *qsum,
                                const u64 *low, u32 *flags, unsigned long long *res7, hipStream_t s);
// rank: the scanned flags; the passing sequences in table order, at most cap of them; any list may be null
hipError_t launch_quals_segments(const u32 *flags, const u32 *rank, const u64 *first, const u64 *len, u64 n_seqs, u64 cap, u64 *seg_seq,
                                 u64 *seg_first, u64 *seg_len, hipStream_t s);

// ---- the 3' adapter cut of the segments of a stream (adapters_kernels.hip; the window arithmetic and the
// hit key are adapters_math.hpp's).  The segments: (first[i], len[i]), or with first == null sequence i of starts.
struct AdapterDesc;
struct AdapterSegs {
    const u64 *first, *len, *starts;
    u64 n;
};
// the words of res: launch_take_segments' two (the second: a segment leaves the stream), the report's sums, and the segments
// cut by each adapter.  The launches below do nothing once res[ADAPTERS_R_BAD] is set.
enum {
    ADAPTERS_R_SUM, ADAPTERS_R_BAD, ADAPTERS_R_PASSED, ADAPTERS_R_TRIMMED, ADAPTERS_R_BASES_IN, ADAPTERS_R_BASES_KEPT, ADAPTERS_R_SHORT,
    ADAPTERS_R_DISCARDED, ADAPTERS_R_ADAPTER, ADAPTERS_R_WORDS = ADAPTERS_R_ADAPTER + 32
};
// keys[i] = the hit key of segment i's cut, or ADAPTERS_NONE.  lists: 2 n words, counts2: 2 words (scratch: the longer segments
// by class).  Three launches: groups of lanes, waves, workgroups.
hipError_t launch_adapters_find(const u64 *words, const AdapterSegs &g, const AdapterDesc *ads, u32 n_ads, const unsigned long long *bad,
                                u64 *keys, u32 *lists, u32 *counts2, hipStream_t s);
// out_len / out_adapter / out_mismatch (any may be null) and pass_flags[i] = segment i passes; res += the sums (zeroed by the caller)
hipError_t launch_adapters_verdict(const AdapterSegs &g, const u64 *keys, u64 min_bases, u32 flags, u64 *out_len, u64 *out_adapter,
                                   u64 *out_mismatch, u32 *pass_flags, unsigned long long *res, hipStream_t s);
// rank: the scanned flags; the passing segments in input order, at most cap of them, seg_seq (null: i) carried through
hipError_t launch_adapters_pass(const AdapterSegs &g, const u64 *seg_seq, const u64 *keys, const u32 *pass_flags, const u32 *rank, u64 cap,
                                const unsigned long long *bad, u64 *pass_seq, u64 *pass_first, u64 *pass_len, hipStream_t s);

// ---- equal sequences (seqeq_kernels.hip; classes, items, realigned word and fingerprint are
// seqeq_math.hpp's).  A table, or a window of one: starts = seq_starts + seq_first, n + 1 entries.
struct SeqTable {
    const u64 *words;
    u64 n_words;
    const u64 *starts;
};
// the fingerprint sweep: fp_short writes fp[i] of every short sequence and the length's part of every long one, ids[i] = i and
// items[i] = the sequence's item count (either may be null); fp_long (off = the exclusive scan of items, n_items its total)
// adds every item's partial sum; weaken keeps SEQEQ_WEAK_MASK of every fingerprint (DNAGPU_DEBUG_WEAK_FINGERPRINT)
hipError_t launch_seqeq_fp_short(const SeqTable &t, u64 n, u64 *fp, u32 *ids, u32 *items, hipStream_t s);
hipError_t launch_seqeq_fp_long(const SeqTable &t, u64 n, const u32 *off, u32 n_items, u64 *fp, hipStream_t s);
hipError_t launch_seqeq_weaken(u64 *fp, u64 n, hipStream_t s);
// One verify round over the fingerprint-sorted list (lfp, lid)[0 .. m), ids ascending inside a run.  head_flags: head[i] = 1
// where a run starts; the caller scans head into run; head_slots: slot[r] = the slot of the head of run r.  verify: hidx[i]
// = the slot of the head of entry i's run, eq[i] = 1 for the head and for an entry equal to it, items[i] = the item count of
// a long pair of equal lengths (eq = 1 until pair_items clears it), else 0.  apply (pre = the exclusive scan of eq): equal
// entries take the head's id as rep, copies[head id] = the run's equal entries, the n_out others move in order to
// (out_fp, out_id).
hipError_t launch_seqeq_head_flags(const u64 *lfp, u64 m, u32 *head, hipStream_t s);
hipError_t launch_seqeq_head_slots(const u32 *head, const u32 *run, u64 m, u32 *slot, hipStream_t s);
hipError_t launch_seqeq_verify(const SeqTable &t, const u32 *lid, u64 m, const u32 *head, const u32 *run, const u32 *slot, u32 *hidx,
                               u32 *eq, u32 *items, hipStream_t s);
// long pairs by items: pair p = sequence (ia ? ia[p] : p) of a against sequence ib[ib_slot[p]] of b, of equal lengths; off =
// the exclusive scan of the pairs' item counts; an item that differs stores 0 into flag[p]
hipError_t launch_seqeq_pair_items(const SeqTable &a, const u32 *ia, const SeqTable &b, const u32 *ib, const u32 *ib_slot,
                                   u64 n_pairs, const u32 *off, u32 n_items, u32 *flag, hipStream_t s);
hipError_t launch_seqeq_apply(const u64 *lfp, const u32 *lid, u64 m, const u32 *hidx, const u32 *eq, const u32 *pre, u32 *rep,
                              u32 *copies, u64 *out_fp, u32 *out_id, u64 n_out, hipStream_t s);
// copies[s] = copies[rep[s]] for every s; *distinct (zeroed by the caller) += the representatives
hipError_t launch_seqeq_spread(const u32 *rep, u32 *copies, u64 n, u64 *distinct, hipStream_t s);
// The match of np probe sequences (fingerprints pfp) against a built side (bt, its sorted list (sfp, sid)[0 .. nb), rep).
// walk, first != 0: every probe walks the representatives of its fingerprint's run: match[p] = the id of the first equal
// one or 0xFFFFFFFF, items[p] = 0; a probe that meets a long candidate of its length parks there instead: cur[p] = the slot,
// flag[p] = 1, items[p] = the pair's item count.  The caller scans items, runs pair_items (ia = null, ib = sid, ib_slot =
// cur) and calls walk with first == 0, which settles or moves on the parked probes only -- until no items are left.
hipError_t launch_seqeq_match_walk(const SeqTable &pt, u64 np, const u64 *pfp, const SeqTable &bt, const u64 *sfp, const u32 *sid,
                                   u64 nb, const u32 *rep, int first, u32 *cur, u32 *flag, u32 *items, u32 *match, hipStream_t s);
// out_match[p] = match32[p] widened (all-ones for none; match32 == null: no probe matches), out_copies[p] = the match's class
// size or 0 (either may be null); *n_matched (zeroed by the caller) += the probes with a match
hipError_t launch_seqeq_match_out(const u32 *match32, const u32 *copies, u64 n, u64 *out_match, u64 *out_copies, u64 *n_matched,
                                  hipStream_t s);
// the stable selects, count -> tile_counts[tile] (seqeq_select_tiles(n) tiles), write (tile_offsets = their exclusive scan) ->
// the matches in ascending id, entries from cap on not stored, either array may be null.  members == 0: the representatives
// with lo <= copies <= hi; members != 0: every sequence whose rep is target.
struct SeqSelect {
    int members;
    u32 target;
    u64 lo, hi;
};
u32 seqeq_select_tiles(u64 n);
hipError_t launch_seqeq_select_count(const u32 *rep, const u32 *copies, u64 n, const SeqSelect &q, u32 *tile_counts, hipStream_t s);
hipError_t launch_seqeq_select_write(const u32 *rep, const u32 *copies, u64 n, const SeqSelect &q, const u32 *tile_offsets,
                                     u64 *out_seq, u64 *out_copies, u64 cap, hipStream_t s);
// two whole values of n_bases bases each: a word that differs stores 0 into *flag, which the caller has set non-zero
hipError_t launch_seqeq_whole(const u64 *a, u64 a_words, const u64 *b, u64 b_words, u64 n_bases, u32 *flag, hipStream_t s);

// ---- queries over counted groups (query_kernels.hip).  A group source is a histogram part (n slots of
// keys / 32-bit counts, count 0 = padding) or the accumulator's table (n = P * ACC_SLOTS 16-byte slots, occ[p] == 0: the
// partition is not read); both are cut into tiles of Q_TILE slots.
constexpr int Q_TILE = 2048;
constexpr int Q_DIGITS = 2048;        // bins of one radix-select pass: 11-bit digits of the count
constexpr u32 Q_LDS_BINS = 8192;      // most bins a workgroup privatises in LDS
struct QHistSrc {
    const u64 *keys;
    const u32 *counts;
    u64 n;
};
struct QAccSrc {
    const u64 *table;
    const u32 *occ;
    u64 n;
};
struct QDenseSrc {                    // dense rows with 64-bit counts (the tail of a ranking): a third, trivial source
    const u64 *keys;
    const u64 *counts;
    u64 n;
};
// which bin a group's count c goes to: spectrum != 0: min(c, n_bins) - 1; else the digit (c >> shift) & (Q_DIGITS - 1) of
// the groups with c >> prefix_shift == prefix (has_prefix != 0; prefix_shift < 64).  lds_bins: 4 .. Q_LDS_BINS.
struct QDigit {
    int spectrum;
    u64 n_bins;
    int shift;
    int has_prefix;
    int prefix_shift;
    u64 prefix;
    u32 lds_bins;
    int want_max;
};
// bins[b] += the groups of bin b (bins: at least max(lds_bins, n_bins) words, zeroed by the caller; several sources add
// into the same bins); want_max: *maxc = max(*maxc, largest count)
hipError_t launch_query_digits(const QHistSrc &s, const QDigit &a, u64 *bins, u64 *maxc, hipStream_t st);
hipError_t launch_query_digits(const QAccSrc &s, const QDigit &a, u64 *bins, u64 *maxc, hipStream_t st);
// the groups with lo <= count <= hi (lo >= 1) to out_keys / out_counts (either may be null) at *cursor + their rank, rows
// from `cap` on not stored; *cursor += all matches (so several sources, or several ranges, append to one output)
hipError_t launch_query_select(const QHistSrc &s, u64 lo, u64 hi, u64 *out_keys, u64 *out_counts, u64 cap, u64 *cursor,
                               hipStream_t st);
hipError_t launch_query_select(const QAccSrc &s, u64 lo, u64 hi, u64 *out_keys, u64 *out_counts, u64 cap, u64 *cursor,
                               hipStream_t st);
hipError_t launch_query_digits(const QDenseSrc &s, const QDigit &a, u64 *bins, u64 *maxc, hipStream_t st);
hipError_t launch_query_select(const QDenseSrc &s, u64 lo, u64 hi, u64 *out_keys, u64 *out_counts, u64 cap, u64 *cursor,
                               hipStream_t st);
// m = 2^x >= 2 rows sorted by (count descending, key ascending)
hipError_t launch_query_sort(u64 *keys, u64 *counts, u32 m, hipStream_t st);
// rank (dnagpu_*_rank): a counting sort by count class.  A group of count c belongs to class min(c, n_classes); cursors[cls]
// (n_classes + 1 words, [0] unused) holds the next free row of class cls -- the caller sets them to the classes' first rows.
// Every tile takes one returning atomic per class it holds rows of and stores (key, 64-bit count) at the rows it got; rows
// from `rows` on are never stored.  3 <= n_classes <= Q_DIGITS.  Several sources go on from the same cursors.
hipError_t launch_query_rank_scatter(const QHistSrc &s, u32 n_classes, u64 *cursors, u64 *out_keys, u64 *out_counts, u64 rows,
                                     hipStream_t st);
hipError_t launch_query_rank_scatter(const QAccSrc &s, u32 n_classes, u64 *cursors, u64 *out_keys, u64 *out_counts, u64 rows,
                                     hipStream_t st);
// rows [0, n) of the two arrays reversed in place
hipError_t launch_query_reverse(u64 *keys, u64 *counts, u64 n, hipStream_t st);

// ---- a table of sequences in one packed stream (extract_kernels.hip)
// marks: bit b set where a sequence starts at base b (starts[1 .. n_seqs - 1]; the buffer is zeroed here)
hipError_t launch_batch_marks(const u64 *starts, u64 n_seqs, u32 *marks, u64 n_mark_words, hipStream_t s);
// *rows = sum over the sequences of max(0, length - k + 1)
hipError_t launch_batch_rows(const u64 *starts, u64 n_seqs, int k, u64 *rows, hipStream_t s);
// the keys of the rows of the table -- windows [p, p + k) of rows [0, n_rows) that reach across no mark -- in no
// particular order; *cursor (zeroed here) ends as their number
hipError_t launch_batch_keys(const u64 *words, u64 n_words, const u32 *marks, u64 n_mark_words, u64 n_rows, int k, u64 *out_keys,
                             unsigned long long *cursor, hipStream_t s);

// ---------------------------------------------------------------- index_kernels.hip
// The index over a stored kmer column: n (r, row) pairs sorted by r = the base-reversed key
// (index_math.hpp), a stable LSD radix sort by 8-bit digits.  One pass = launch_index_hist (hist[d * tiles + tile], tiles =
// index_sort_tiles(n)) -> launch_scan_u32 over the 256 * tiles words -> launch_index_scatter; launch_index_digit_bins tells
// from the scanned matrix how many digits occur at all (one: the scatter would move nothing).
constexpr int INDEX_SORT_TILE = 2048;     // keys per workgroup of the sort: 256 threads x 8, each wave a contiguous quarter
constexpr int INDEX_SCAN_TILE = 2048;     // candidates per workgroup of the scan's sweeps
struct IndexSortSrc {                     // what a pass reads: the caller's keys (r is formed on the fly, row = position) while
    const u64 *keys;                      // nothing has moved yet (keys != null), else the pairs of the pass before
    const u64 *r;
    const u32 *row;
    int k;
    u32 row_base;                         // keys != null: row = row_base + position (the build: 0; an appended batch: next_row)
};
u32 index_sort_tiles(u64 n);
hipError_t launch_index_hist(const IndexSortSrc &src, u64 n, int shift, u32 *hist, hipStream_t s);
hipError_t launch_index_digit_bins(const u32 *off, u64 n, u32 *nonempty, hipStream_t s);
hipError_t launch_index_scatter(const IndexSortSrc &src, u64 n, int shift, const u32 *off, u64 *out_r, u32 *out_row, hipStream_t s);
// *distinct (zeroed by the caller) += the keys of the sorted r[0 .. n) that differ from their predecessor
hipError_t launch_index_distinct(const u64 *r, u64 n, u64 *distinct, hipStream_t s);
// The scan.  ranges: the R <= 1024 concrete prefixes of p bases that fb admits (index_prune_depth), in ascending order, each
// looked up in r: beg[j] = first slot, off[0 .. R] = exclusive scan of the lengths, *visited = off[R] = the candidates C.
hipError_t launch_index_ranges(const u64 *r, u64 n, const FilterBits &fb, int p, u32 R, u32 *off, u32 *beg, u64 *visited,
                               hipStream_t s);
// sweeps over the C candidates in tiles of INDEX_SCAN_TILE (index_scan_tiles(C) tiles): test != 0: a candidate matches when
// its key passes fd (the positions behind the prune depth); count -> tile_counts[tile]; write (tile_offsets = their
// exclusive scan; unused when test == 0) -> the matches in index order, row ids widened to u64 and keys un-reversed, rows
// from cap on not stored; either array may be null.
struct IndexScanArgs {
    const u64 *r;
    const u32 *row;
    const u32 *off;
    const u32 *beg;
    u32 R;
    u32 C;
    int k;
    int test;
    FilterDev fd;
};
u32 index_scan_tiles(u64 C);
hipError_t launch_index_sweep_count(const IndexScanArgs &a, u32 *tile_counts, hipStream_t s);
hipError_t launch_index_sweep_write(const IndexScanArgs &a, const u32 *tile_offsets, u64 *out_rows, u64 *out_keys, u64 cap,
                                    hipStream_t s);
// out_first[j], out_count[j] = the window of the index that holds keys[j] (count 0: absent, or bits above 2k set)
hipError_t launch_index_lookup(const u64 *r, u64 n, int k, const u64 *keys, u64 m, u64 *out_first, u64 *out_count, hipStream_t s);
// entries [first, first + count) as u64 row ids and un-reversed keys (either may be null)
hipError_t launch_index_read(const u64 *r, const u32 *row, int k, u64 first, u64 count, u64 *out_rows, u64 *out_keys, hipStream_t s);
// The append: the stable merge of the sorted runs A = (ar, arow)[0 .. na) and B = (br, brow)[0 .. nb) into (out_r, out_row)
// [0 .. na + nb), an A entry before a B entry of the same r (index_math.hpp: index_merge_split).  Two launches: the
// partition -- part[t] = the entries of A among the first min(t * INDEX_SORT_TILE, na + nb) outputs, t = 0 ..
// index_sort_tiles(na + nb), by binary search in global memory -- and the merge, one workgroup per tile of INDEX_SORT_TILE
// outputs.  na + nb <= 2^32 - 1.
hipError_t launch_index_merge_partition(const u64 *ar, u64 na, const u64 *br, u64 nb, u32 *part, hipStream_t s);
hipError_t launch_index_merge(const u64 *ar, const u32 *arow, u64 na, const u64 *br, const u32 *brow, u64 nb, const u32 *part,
                              u64 *out_r, u32 *out_row, hipStream_t s);
// The delete.  mark: bit ids[j] of bitmap (index_bitmap_words(n_bits) zeroed words) is set for every j < m with ids[j] <
// n_bits.  The stable compaction of the entries whose row's bit is clear, in tiles of INDEX_SORT_TILE entries: count ->
// tile_counts[tile]; write (tile_offsets = their exclusive scan) -> the kept entries in their order.  Every row[i] < n_bits.
u64 index_bitmap_words(u64 n_bits);
hipError_t launch_index_mark(const u64 *ids, u64 m, u64 n_bits, u32 *bitmap, hipStream_t s);
hipError_t launch_index_compact_count(const u32 *row, u64 n, const u32 *bitmap, u32 *tile_counts, hipStream_t s);
hipError_t launch_index_compact_write(const u64 *r, const u32 *row, u64 n, const u32 *bitmap, const u32 *tile_offsets, u64 *out_r,
                                      u32 *out_row, u64 n_out, hipStream_t s);

// ---------------------------------------------------------------- the super-k-mer engine (sk_device.hpp), three files
// super-k-mer (minimizer) partitioning for long k-mers: the dna sweeps (level 0: records per coarse digit of every
// chunk of rows / records scattered into the coarse buckets), the record level (level 1: d1), and the expansion of
// mid buckets into key nodes.  k in [sk_min_k(), 32]; c0n = coarse buckets, b1bits = bits of d1, r0bits = split
// bits of the root (2^r0bits >= c0n); records are 16 bytes each.
// ---------------------------------------------------------------- sk_level0_kernels.hip
int sk_min_k();
int sk_minimizer_len(int k);          // m: 15 for k >= 23, 13 for k = 21, 22, 12 for k = 20
int sk_tile_rows();
int sk_max_c0();          // most coarse buckets the level-0 sweeps support
// aux: the histogram sweep adds its chunks' counts into ONE row aux[0 .. 2^r0bits) instead of hist rows (a sampled
// histogram); the scatter sweep takes aux as its slab table (sk_slab_words() words, launch_sk_slab_init): level 0 WITHOUT
// the histogram sweep -- every chunk reserves sk_slab_cap(est ...) slots of every digit's region, unused slots become NULL
// records (bit 63 of the second word; level 1 skips them), aux[17 * sk_max_c0() + d] = records stored per digit,
// aux[18 * sk_max_c0()] = 1 if a chunk ran out of slots, aux[18 * sk_max_c0() + 1] = slots of all regions.
// marks (or null): one bit per base of the packed stream, set where a sequence of a TABLE of sequences starts
// (dnagpu_count_kmers_batch): rows whose k-mer reaches across a start are rows of no sequence and make no record.
hipError_t launch_sk_level0(bool scatter, const Chunk *chunks, u32 n_chunks, const u64 *words, u64 n_words, u64 first, int k,
                            u32 c0n, u32 b1bits, u32 r0bits, u32 *hist, const u32 *tot, void *recs, hipStream_t s,
                            u32 *aux = nullptr, const u32 *marks = nullptr, u64 n_mark_words = 0);
hipError_t launch_sk_sample_chunks(Chunk *chunks, u32 n_chunks, u32 stride, u32 len, u32 n, hipStream_t s);
int sk_slab_words();
u32 sk_slab_cap(u32 est, u64 chunk_rows, u64 sampled);
hipError_t launch_sk_slab_init(const u32 *est, u32 r0bits, u32 chunk_rows, u32 sampled, u32 n_chunks, u32 *slab, Node *nodes,
                               hipStream_t s);
// (a stage of the tail that is compiled in sk_level0_kernels.hip: see the head of that file)
// long buckets of few distinct keys (repeats): one workgroup per bucket, one LDS table for the whole bucket; status[i] = 1
// where the distinct keys outgrew the table (the bucket's range is then all padding)
// slices of SKB records per big bucket: nsl[p] = its slices, msl[p] = the same if more than one (else 0); after exclusive
// scans: sl_bucket / sl_idx[first slice of p + j] = (p, j).  Partial areas of sk_big_partial_slots() groups each, one per
// slice of a sliced bucket (mfirst = scan of msl); part_n[area] = its groups (~0: the slice gave up).
hipError_t launch_sk_node_lens(const Node *nodes, u32 n, u32 *lens, hipStream_t s);
u32 sk_big_slice_records();
u64 sk_big_partial_slots();
hipError_t launch_sk_big_slices(const Node *fin, const u32 *list, u32 n_list, u32 *nsl, u32 *msl, hipStream_t s);
hipError_t launch_sk_big_slice_fill(const u32 *nsl_raw, const u32 *sfirst, u32 n_list, u32 *sl_bucket, u32 *sl_idx, hipStream_t s);
hipError_t launch_sk_count_big(const Node *fin, const u32 *list, const u32 *list_off, const u32 *nsl, const u32 *mfirst,
                               const u32 *sl_bucket, const u32 *sl_idx, u32 n_slices, u32 n_list, const void *recs, int k,
                               u64 *n_groups, u64 *seg_off, u32 *seg_cnt, u64 *out_keys, u32 *out_counts, u32 *status, u64 *part_keys,
                               u32 *part_cnts, u32 *part_n, bool any_sliced, hipStream_t s);

// ---------------------------------------------------------------- sk_level1_kernels.hip
hipError_t launch_sk_hist1(const Node *nodes, const Chunk *chunks, u32 n_chunks, const void *recs, u32 *hist, u32 *kcount,
                           hipStream_t s, bool by_d2 = false);
hipError_t launch_sk_scatter1(const Node *nodes, const Chunk *chunks, u32 n_chunks, const void *src, void *dst, const u32 *hist,
                              const u32 *tot, hipStream_t s, bool by_d2 = false, u32 *gcur = nullptr);
// (by_d2: the same kernels on the 4-bit digit d2 -- the heavy mid buckets' split into final buckets)
// Level 1 WITHOUT its histogram (speculative): every mid bucket is a region of the destination buffer, sk_spec_span(len, bits)
// slots for a node of len records (host and device share the formula); spec = 2 words per node, out = 3 words (slots of all
// regions; 1 if they pass 2^32; the sweep's overflow flag), gcur = rows of ROW_STRIDE cursors (row = the node's first chunk).
// The sweep counts the k-mers per mid bucket into kcount; launch_sk_spec_nodes writes the mid nodes and raises *over too.
u64 sk_spec_span(u32 len, int bits);
// Over UNEVEN coarse buckets (repeats) the regions come from a sampled histogram instead: one piece of sk_sample1_len()
// records in every sk_sample1_every() pieces of a node's records (the host lists the pieces as chunks), rcap / rstart per mid
// bucket (launch_sk_sampled_regions), handed to the three launchers above as rstart / rcap.
hipError_t launch_sk_spec_regions(const Node *nodes, u32 n_nodes, u32 *spec, u32 *out, u32 *gcur, hipStream_t s,
                                  const u32 *rstart = nullptr);
hipError_t launch_sk_scatter1_spec(const Node *nodes, const Chunk *chunks, u32 n_chunks, const void *src, void *dst, u32 *gcur,
                                   const u32 *spec, u32 *kcount, u32 *over, hipStream_t s, const u32 *rstart = nullptr,
                                   const u32 *rcap = nullptr);
hipError_t launch_sk_spec_nodes(const Node *nodes, u32 n_nodes, const u32 *spec, const u32 *gcur, Node *next, u32 *over,
                                hipStream_t s, const u32 *rstart = nullptr, const u32 *rcap = nullptr);
u32 sk_sample1_len();
u32 sk_sample1_every();
hipError_t launch_sk_sampled_regions(const Node *nodes, const Chunk *samples, u32 n_samples, const void *recs, u32 n_mid, u32 *est,
                                     u32 *rcap, u32 *rstart, u32 *scan_tmp, u32 *total, hipStream_t s);
// every mid bucket's records regrouped by d2 from src into the same range of dst; out_nodes[16 i + j] = final bucket:
// start / len in records, child_base = its k-mers
int sk_regroup_tile();   // records one workgroup regroups in one go; longer mid buckets need any_long (a second kernel)
// gate != null: a workgroup of the one-tile kernel returns at once unless *gate == 0 (the launch went out before the host
// had seen level 1's verdict: launch_sk_l1_gate)
hipError_t launch_sk_regroup(const Node *mids, u32 n_mids, const void *src, void *dst, Node *out_nodes, bool any_long, hipStream_t s,
                             const u32 *gate = nullptr);
// The gate of an early level 2: *gate = 0 exactly when the one-tile regroup is all that level 2 has to do, else the reasons
// why not.  Host and device judge a mid bucket with the one function; the host recomputes the word from what it read back.
enum : u32 {
    SK_GATE_SPEC = 1,       // the speculative sweep's status words: a wrong span, regions past 2^32, a region overflowed
    SK_GATE_SLAB = 2,       // level 0's slab status words: a chunk ran out of slots, or a wrong span
    SK_GATE_LONG = 4,       // a mid bucket of more than one regroup tile
    SK_GATE_HEAVY = 8,      // a heavy mid bucket (k-mers over mid_limit, records over rec_limit)
    SK_GATE_KMERS = 16,     // the k-mers found are not the expected ones, or pass 2^32
};
struct SkGateIn {
    const u32 *lens, *kcount;   // records and k-mers per mid bucket (n_mid each)
    u32 n_mid;
    const u32 *status1;         // the sweep's three status words
    u32 span1, sampled;         // the slots its regions must span (not checked for sampled regions)
    const u32 *status0;         // level 0's two slab status words, or null
    u32 span0;
    u64 mid_limit, n_expected;  // (n_expected 0: not known)
    u32 rec_limit, tile;
};
__host__ __device__ inline u32 sk_gate_bucket(u32 len, u32 kmers, u64 mid_limit, u32 rec_limit, u32 tile)
{
    return (len > tile ? (u32)SK_GATE_LONG : 0u) | ((kmers > mid_limit || len > rec_limit) ? (u32)SK_GATE_HEAVY : 0u);
}
__host__ __device__ inline u32 sk_gate_status(const u32 *st1, u32 span1, u32 sampled, const u32 *st0, u32 span0)
{
    u32 g = 0;
    if ((!sampled && (st1[0] != span1 || st1[1])) || st1[2])
        g |= SK_GATE_SPEC;
    if (st0 && (st0[0] || st0[1] != span0))
        g |= SK_GATE_SLAB;
    return g;
}
hipError_t launch_sk_l1_gate(const SkGateIn &in, u32 *gate, hipStream_t s);

// ---------------------------------------------------------------- sk_tail_kernels.hip
int sk_count_cap();       // most k-mers a final bucket may hold to be counted from its records
// (f_over3 / k_over3: flag and k-mers of the buckets of class "over", which are all of the expansion's when none is big)
hipError_t launch_sk_select_flags(const Node *fin, u32 n_fin, u32 cap, u32 big_limit, u32 *f_small, u32 *f_big, u32 *k_range,
                                  u32 *k_big, u32 *f_over3, u32 *k_over3, hipStream_t s);
hipError_t launch_sk_select_lists(const Node *fin, u32 n_fin, u32 cap, u32 big_limit, const u32 *p_small, const u32 *p_big,
                                  const u32 *kb_range, u32 *list_small, u32 *off_small, u32 *list_big, u32 *off_big, hipStream_t s);
// buckets that go through the expansion: too many k-mers for sk_count_big, or given up by it (big_status[p] != 0)
hipError_t launch_sk_over_flags(const Node *fin, u32 n_fin, u32 cap, u32 big_limit, const u32 *p_big, const u32 *big_status,
                                u32 *f_over, u32 *k_over, hipStream_t s);
hipError_t launch_sk_over_list(const Node *fin, u32 n_fin, const u32 *f_raw, const u32 *p_over, const u32 *kb_over, Node *over_nodes,
                               u32 *over_kbase, hipStream_t s);
// final buckets list[0..n_list) (indices into fin) counted from their records in an LDS hash table; groups appended
// at *cursor, seg_off / seg_cnt[bucket] = where they went
// list_off[i] = first output slot of bucket list[i] (its range is as long as its k-mers; slots past its distinct keys are
// count-0 padding); *n_groups += the groups written
// (left: 2 n_list + 1 words of work memory -- the buckets the record test leaves to the k-mer table kernel)
hipError_t launch_sk_count(const Node *fin, const u32 *list, const u32 *list_off, u32 n_list, const void *recs, int k, u64 *n_groups,
                           u64 *seg_off, u32 *seg_cnt, u64 *out_keys, u32 *out_counts, u32 *left, hipStream_t s);
// buckets sk_count does not take, expanded to keys in record order (no host step): slices of sk_flat_slice() records
// per bucket (n_slices[i], then after an exclusive scan slice_first[i]; slice_rec0 = first record, slice_nrec = records),
// k-mers per slice, after a scan the keys of slice s at key_base + slice_koff[s] and one key node per bucket
int sk_flat_slice();
// out[j] = mids[idx[j]] with child_base = kcount[idx[j]]; mids[idx[j]].len = 0
hipError_t launch_sk_take_heavy(Node *mids, const u32 *idx, u32 n_heavy, const u32 *kcount, Node *out, hipStream_t s);
hipError_t launch_sk_slice_count(const Node *buckets, u32 nb, u32 *n_slices, hipStream_t s);
hipError_t launch_sk_slice_fill(const Node *buckets, u32 nb, const u32 *slice_first, u32 *slice_rec0, u32 *slice_nrec, hipStream_t s);
hipError_t launch_sk_slice_kmers(const void *recs, const u32 *slice_rec0, const u32 *slice_nrec, u32 n_slices, u32 *slice_km,
                                 hipStream_t s);
hipError_t launch_sk_slice_nodes(const Node *buckets, u32 nb, const u32 *slice_first, const u32 *slice_koff, u32 n_slices,
                                 const u32 *total_keys, u32 key_base, int k, bool check_kmers, Node *out, u64 *n_bad, hipStream_t s);
// keys[first .. *end): key_unmix (the groups of the tree over the expansion's mixed keys; at most max_groups of them)
hipError_t launch_sk_unmix(u64 *keys, u64 first, const u64 *end, u64 max_groups, int k, hipStream_t s);
hipError_t launch_sk_expand_flat(const void *recs, const u32 *slice_rec0, const u32 *slice_nrec, const u32 *slice_koff, u32 key_base,
                                 u32 n_slices, int k, u64 *keys, hipStream_t s);
hipError_t launch_sk_heavy_finals(const Node *kids, u32 n, const u32 *kcount, Node *out, hipStream_t s);

// ---------------------------------------------------------------- count_kernels.hip, continued
// scatter-only microbenchmark entry (bench tooling): one level over a key array
int scatter_tile_keys();
int scatter_threads();

}  // namespace dnagpu
