/*
 * dnagpu.h -- C-ABI of the MI355X (gfx950) k-mer back-end.
 *
 * This is the drop-in boundary for the k-mer generation / filtering / counting path of the
 * PostgreSQL extension sid2364/dna-sequences-pg-extension.  The extension's fmgr glue (dna.c)
 * stays as it is; where its functions loop over bases on the CPU they call these entry points
 * instead (INTEGRATION.md shows the glue).  Plain C: pointers, sizes, status codes.  No
 * exceptions and no longjmp ever cross this boundary; no PostgreSQL, torch or C++ types appear.
 *
 * Data formats are the reference's own:
 *   packed dna   uint64 words, base i in word i/32 at bits (2i mod 64)..+1, LSB first,
 *                A=00 T=01 C=10 G=11, tail bits zero        (dna.c:42-47, 114-128)
 *   kmer key     uint64, base i of the k-mer at bits 2i..2i+1 (dna.c:61-65, 397-420); the k-mer
 *                at position p is bits [2p, 2p+2k) of the packed stream
 *   qkmer        NUL-terminated IUPAC text, <= 32 chars      (dna.c:81-84, 876-900)
 *
 * Threading / process model: one context per process and device, created lazily AFTER fork (a
 * PostgreSQL backend must not inherit a HIP runtime from the postmaster); calls on one context
 * are synchronous with respect to the caller unless documented otherwise and not re-entrant.
 * Every pointer named dev_* is device memory on the context's GPU; every other pointer is host
 * memory owned by the caller.  The library never keeps a caller pointer after the call returns,
 * except dnagpu_dna_wrap and dnagpu_table_classes (documented there).
 */
#ifndef DNAGPU_H
#define DNAGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: histograms of several parts (dnagpu_hist_parts: what dnagpu_count_multi_unordered returns with its default of three
 * bucket groups per owner -- dnagpu_hist_device_keys / _counts are NULL for those), the dnagpu_multi_* options, the
 * table-of-sequences count (dnagpu_count_kmers_batch, dnagpu_dna_set_sequences + dnagpu_count_kmers_table,
 * dnagpu_hist_merge), the rows of a table of sequences with the fused WHERE forms (dnagpu_generate_kmers_table), the index
 * over a stored kmer column (dnagpu_kmer_index_*) and its updates (dnagpu_kmer_index_append / _delete / _next_row), the
 * join of two accumulators (dnagpu_acc_join, dnagpu_acc_partitions), the strand-neutral forms (dnagpu_dna_revcomp,
 * dnagpu_kmer_strand, dnagpu_acc_add_canonical), the per-sequence hits of a table in a counted set (dnagpu_table_hits,
 * dnagpu_seq_hits_*), sequences by id and stream segments as a new resident table (dnagpu_dna_take, dnagpu_dna_gather,
 * dnagpu_dna_sequence_starts), the k-mer profile of every sequence of a table (dnagpu_table_profile), equal sequences
 * (dnagpu_dna_equals, dnagpu_table_classes, dnagpu_seq_classes_*, dnagpu_table_match): additions only, so the number stays */
#define DNAGPU_ABI_VERSION 2

/* ---- status codes ------------------------------------------------------------------------
 * 1..3 are the reference's own ERROR conditions on this path; dnagpu_strerror() returns the
 * reference's exact message text for them so the glue can ereport() it unchanged. */
#define DNAGPU_OK                       0
#define DNAGPU_ERR_INVALID_K            1   /* dna.c:772-773 "Invalid k value: must be between 1 and 32" */
#define DNAGPU_ERR_QKMER_LEN_MISMATCH   2   /* dna.c:1106-1108 "Qkmer pattern and kmer lengths do not match" */
#define DNAGPU_ERR_PREFIX_TOO_LONG      3   /* dna.c:854-856 "Prefix length cannot exceed kmer length" */
#define DNAGPU_ERR_QKMER_INVALID        4   /* dna.c:876-900 pattern empty / > 32 / non-IUPAC character */
#define DNAGPU_ERR_BAD_ARG              5   /* NULL pointer, range outside the sequence, bad filter kind */
#define DNAGPU_ERR_TOO_LARGE            6   /* more than 2^32 - 1 k-mers in one call */
#define DNAGPU_ERR_NO_DEVICE            7   /* no usable gfx950 device / HIP runtime unavailable */
#define DNAGPU_ERR_OOM                  8   /* device or host allocation failed */
#define DNAGPU_ERR_HIP                  9   /* a HIP call or kernel failed; see dnagpu_last_error() */
#define DNAGPU_ERR_INTERNAL             10
#define DNAGPU_ERR_DNA_EMPTY            11  /* dna.c:160-161 "DNA sequence cannot be empty" */
#define DNAGPU_ERR_DNA_INVALID_CHAR     12  /* dna.c:165-166 "Invalid character in DNA sequence: %c" */

const char *dnagpu_strerror(int status);
/* detail text of the most recent failing call on the calling thread (HIP error string, etc.) */
const char *dnagpu_last_error(void);
int dnagpu_abi_version(void);
/* Number of HIP devices this process can use (0 when there is none or the runtime cannot start).  Does not create a
 * context. */
int dnagpu_device_count(void);

/* ---- context ------------------------------------------------------------------------------ */
typedef struct dnagpu_ctx dnagpu_ctx;

/* Creates a context on HIP device `device` (0-based).  Lazy, post-fork.  Owns one HIP stream and
 * a pool of device work buffers that are recycled between calls. */
int dnagpu_init(int device, dnagpu_ctx **out_ctx);
void dnagpu_destroy(dnagpu_ctx *ctx);
/* Blocks until all work queued on the context's stream has finished. */
int dnagpu_synchronize(dnagpu_ctx *ctx);
/* The context's hipStream_t (as void*), for callers that enqueue their own HIP work around it. */
void *dnagpu_stream(dnagpu_ctx *ctx);
/* Releases every pooled device buffer that is not in use. */
int dnagpu_trim(dnagpu_ctx *ctx);
/* Bytes of device memory currently held by the context (in use + pooled). */
uint64_t dnagpu_device_bytes(dnagpu_ctx *ctx);

/* ---- device-resident dna (the detoasted Dna* of dna.c:768, moved to HBM once) --------------- */
typedef struct dnagpu_dna dnagpu_dna;

/* Copies ceil(n_bases/32) packed words host -> device.  Replaces nothing in the reference by
 * itself: it is the hand-off of dna->bit_sequence / dna->length (dna.c:45-46). */
int dnagpu_dna_upload(dnagpu_ctx *ctx, const uint64_t *words, uint64_t n_bases, dnagpu_dna **out);
/* Wraps n_words packed words already in device memory (no copy; the caller keeps them alive and
 * unchanged until dnagpu_dna_free, which does not release them).  n_words >= ceil(n_bases/32).  The view may lie in the
 * middle of the caller's own data: results never depend on the bits behind base n_bases - 1 (the rest of the last word,
 * words [ceil(n_bases/32), n_words)) -- dnagpu_dna_to_wire clears them in the image -- and no word from n_words on is
 * read. */
int dnagpu_dna_wrap(dnagpu_ctx *ctx, const uint64_t *dev_words, uint64_t n_words, uint64_t n_bases,
                    dnagpu_dna **out);
/* Synthetic sequence generated on the device: word w = splitmix64(seed + w) (i.i.d. uniform bases,
 * the distribution of data/create_dna.py:27-33), tail bits zero.  motif_len > 0 gives the
 * repeat-rich variant: the second half of the sequence tiles the first motif_len bases. */
int dnagpu_dna_synth(dnagpu_ctx *ctx, uint64_t seed, uint64_t n_bases, uint64_t motif_len,
                     dnagpu_dna **out);
int dnagpu_dna_download(dnagpu_ctx *ctx, const dnagpu_dna *dna, uint64_t *words);
uint64_t dnagpu_dna_length(const dnagpu_dna *dna);
const uint64_t *dnagpu_dna_device_words(const dnagpu_dna *dna);
void dnagpu_dna_free(dnagpu_ctx *ctx, dnagpu_dna *dna);

/* ---- text <-> packed forms on the device (the steps either side of the path) ----------------
 * dna_in's work, validate_dna_sequence + encode_dna (dna.c:159-171, 114-128): n_bases characters
 * (host memory, or device memory when text_on_device != 0; no terminating NUL needed) become a
 * device-resident dna.  An empty text is DNAGPU_ERR_DNA_EMPTY; a character other than A/T/C/G is
 * DNAGPU_ERR_DNA_INVALID_CHAR with *bad_pos / *bad_char (either may be NULL) = the FIRST offending
 * character, the one the reference's message names. */
int dnagpu_dna_pack(dnagpu_ctx *ctx, const char *text, uint64_t n_bases, int text_on_device,
                    dnagpu_dna **out, uint64_t *bad_pos, char *bad_char);
/* decode_dna (dna.c:135-152): bases [first, first+count) as `count` characters (no NUL). */
int dnagpu_dna_unpack(dnagpu_ctx *ctx, const dnagpu_dna *dna, uint64_t first, uint64_t count,
                      char *out_text, int out_on_device);
/* bases [first, first+count) of dna, reverse-complemented, as a new device-resident dna (a sequence set is not carried):
 * base j of the result is the complement (A <-> T, C <-> G: code ^ 1) of base first + count - 1 - j.  The window follows
 * dnagpu_dna_unpack's range rule: one that leaves the sequence is DNAGPU_ERR_BAD_ARG; count == 0 is DNAGPU_ERR_DNA_EMPTY,
 * because the type has no empty value.  The bits behind the result's last base are zero (dnagpu_dna_upload's rule); no word
 * of dna outside [first/32, ceil((first+count)/32)) is read and the result never depends on bits behind dna's last base
 * (dnagpu_dna_wrap's rule).  Free the result with dnagpu_dna_free. */
int dnagpu_dna_revcomp(dnagpu_ctx *ctx, const dnagpu_dna *dna, uint64_t first, uint64_t count, dnagpu_dna **out);
/* ---- binary wire image: dna_recv / dna_send (dna.c:244-268, 270-291) ---------------------------
 * Wire image of a dna: int64 length in bases, then ceil(length/32) packed words, every field in
 * network byte order (what pq_sendint64 writes and pq_getmsgint64 reads).  The reference moves its
 * length field with pq_getmsgint / pq_sendint of size 8, which PostgreSQL rejects ("unsupported
 * integer size 8"), so its binary I/O cannot work as written; this is the format it describes, with
 * a length field that does.  from_wire: wire_bytes must equal dnagpu_dna_wire_size(length) else
 * DNAGPU_ERR_BAD_ARG; length 0 is DNAGPU_ERR_DNA_EMPTY (the type has no empty value, dna.c:160-161);
 * bits behind the last base are cleared (dna.c:186).  A device-side wire buffer must be 8-byte
 * aligned. */
uint64_t dnagpu_dna_wire_size(uint64_t n_bases);
int dnagpu_dna_from_wire(dnagpu_ctx *ctx, const void *wire, uint64_t wire_bytes, int wire_on_device,
                         dnagpu_dna **out);
int dnagpu_dna_to_wire(dnagpu_ctx *ctx, const dnagpu_dna *dna, void *wire, uint64_t wire_cap,
                       int wire_on_device);

/* decode_kmer / kmer_out (dna.c:428-452, 538-546) for n keys of k bases: n records of k characters
 * followed by a NUL (record stride k+1).  keys and out_text both host, or both device. */
int dnagpu_kmers_to_text(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, int k, char *out_text,
                         int on_device);

/* ---- generate_kmers(dna, k)  (dna.c:743-837, dna--1.0.sql:188-191) -------------------------- */

/* Row count of generate_kmers: n_bases - k + 1 (dna.c:781), 0 when n_bases < k (the reference
 * underflows there).  DNAGPU_ERR_INVALID_K unless 1 <= k <= 32 (dna.c:771-773). */
int dnagpu_kmer_count(uint64_t n_bases, int k, uint64_t *n_kmers);

/* Writes the keys of rows [first, first+count) of generate_kmers(dna, k), in position order,
 * duplicates kept, to out_keys (host memory, or device memory when out_on_device != 0).
 * Replaces the per-row body dna.c:803-825 (decode to text, kmer_make, encode). */
int dnagpu_generate_kmers(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k,
                          uint64_t first, uint64_t count, uint64_t *out_keys, int out_on_device);

/* ---- generate_kmers fused with a WHERE operator --------------------------------------------- */
#define DNAGPU_FILTER_EQUALS       1   /* kmer = q         kmer_eq,     dna.c:655-668, 686-696 */
#define DNAGPU_FILTER_STARTS_WITH  2   /* kmer ^@ prefix   starts_with, dna.c:842-866           */
#define DNAGPU_FILTER_CONTAINS     3   /* qkmer @> kmer    contains,    dna.c:1064-1135         */

typedef struct dnagpu_filter {
    int32_t  kind;          /* DNAGPU_FILTER_*                                                   */
    int32_t  length;        /* EQUALS / STARTS_WITH: length (bases) of the right-hand kmer       */
    uint64_t bits;          /* EQUALS / STARTS_WITH: its bit_sequence                            */
    char     pattern[36];   /* CONTAINS: the qkmer text, NUL-terminated                          */
    int32_t  reserved;
} dnagpu_filter;

/* Rows of generate_kmers(dna,k) restricted to [first, first+count) that satisfy `filter`, in
 * position order (the reference's row order, test.sql:86-92).  Keys go to out_keys and their
 * positions to out_pos (either may be NULL), at most `cap` of each; *n_out receives the total
 * number of matching rows even when it exceeds cap.  Errors exactly where the reference's operator
 * raises them on the first row: CONTAINS with strlen(pattern) != k -> QKMER_LEN_MISMATCH,
 * STARTS_WITH with length > k -> PREFIX_TOO_LONG (only when there is at least one row).  An EQUALS
 * filter of another length matches nothing.  A 32-base prefix compares all 64 bits (the
 * reference's shift-by-64 at dna.c:862 is undefined behaviour). */
int dnagpu_generate_kmers_filtered(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k,
                                   const dnagpu_filter *filter, uint64_t first, uint64_t count,
                                   uint64_t *out_keys, uint64_t *out_pos, uint64_t cap,
                                   uint64_t *n_out, int out_on_device);

/* ---- GROUP BY kmer, count(*)  (kmer_hash dna.c:722-735 + kmer_eq dna.c:686-696 drive
 * PostgreSQL's HashAggregate in the reference; test.sql:95-119) ------------------------------ */
typedef struct dnagpu_hist dnagpu_hist;

/* Groups rows [first, first+count) of generate_kmers(dna,k) by key.  The result lives in device
 * memory: n_distinct (key, count) pairs in two dense arrays (uint64 keys, uint32 counts).  Group order in those arrays is
 * unspecified, as it is in PostgreSQL (the arrays hold key-range segments in the order the GPU
 * finished them, keys ascending inside a segment); dnagpu_hist_download serves the groups in
 * ascending key order through the segment directory.  At most 2^32-1 rows per call. */
int dnagpu_count_kmers(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k,
                       uint64_t first, uint64_t count, dnagpu_hist **out);
/* The same groups when the caller does not need them in key order -- PostgreSQL's own GROUP BY order is
 * unspecified (test.sql:95-104), so this is what the SQL entry point calls.  Long k-mers (k >= 20) of long
 * sequences (2^25 rows or more; k = 20, 21 and 22: where that is the faster engine, up to 2^28 / 2^29 / 2^31 rows) are then
 * partitioned as super-k-mers (runs of consecutive k-mers sharing a minimizer, 16 bytes per
 * ~9 k-mers) instead of 8-byte keys: less than a third of the partition traffic.  dnagpu_hist_download and
 * dnagpu_hist_sorted_view then serve the groups bucket by bucket (keys ascending inside a bucket only);
 * dnagpu_hist_is_sorted tells which kind a histogram is. */
int dnagpu_count_kmers_unordered(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k,
                                 uint64_t first, uint64_t count, dnagpu_hist **out);
int dnagpu_hist_is_sorted(const dnagpu_hist *h);
/* GROUP BY kmer, count(*) over a TABLE of sequences -- the reference's second counting shape,
 *   SELECT k.kmer, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, K) AS k(kmer) GROUP BY k.kmer
 * (test.sql:140-150: one generate_kmers call per row of the table, dna.c:743-837; data/create_dna.py:36-49 writes such
 * tables of read-like rows).  The table travels as ONE packed stream `dna` (the sequences' bases back to back, no
 * padding) and seq_starts[0 .. n_seqs] (host memory): the first base of every sequence, seq_starts[0] = 0,
 * seq_starts[n_seqs] = dnagpu_dna_length(dna), ascending (equal neighbours: an empty sequence).  The rows are those of
 * every sequence's own generate_kmers: no k-mer spans two sequences, a sequence shorter than k has none (the 64-bit
 * restatement of dna.c:781).  Same result object as dnagpu_count_kmers_unordered (group order unspecified;
 * dnagpu_hist_is_sorted tells); dnagpu_hist_total = the rows of the table.  At most 2^32 - 1 bases per call: callers
 * that stream larger tables count batch by batch and add the histograms up (dnagpu_acc_add: 64-bit counts, no total limit). */
int dnagpu_count_kmers_batch(dnagpu_ctx *ctx, const dnagpu_dna *dna, const uint64_t *seq_starts, uint64_t n_seqs,
                             int k, dnagpu_hist **out);
/* The same table kept RESIDENT: dnagpu_dna_set_sequences validates seq_starts (as above), uploads them and builds the
 * boundary marks once, beside the packed stream (replacing an earlier set; n_seqs = 0 over an empty stream clears it;
 * released with dnagpu_dna_free); dnagpu_count_kmers_table then counts the table for any k with nothing crossing the bus
 * -- a glue that caches the packed table across queries pays the boundaries' upload (8 bytes per sequence: 80 MB and
 * 5.8 ms of a 14.4 ms call at 10^7 reads) once instead of per query.  dnagpu_dna_sequences: the sequences set, 0 if none.
 * dnagpu_count_kmers_table without a set (and a non-empty stream): DNAGPU_ERR_BAD_ARG. */
int dnagpu_dna_set_sequences(dnagpu_ctx *ctx, dnagpu_dna *dna, const uint64_t *seq_starts, uint64_t n_seqs);
uint64_t dnagpu_dna_sequences(const dnagpu_dna *dna);
int dnagpu_count_kmers_table(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, dnagpu_hist **out);
/* The ROWS of the same table -- FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) [WHERE <op>]: the
 * k-mers of every sequence, each with the sequence it came from (what test.sql:172-176 inserts into kmer_data_t), and the
 * three WHERE forms over them (test.sql:187-262 asks them of that stored column, whose row ids are this order).
 * Input: a table made resident with dnagpu_dna_set_sequences; a non-empty stream without a set is DNAGPU_ERR_BAD_ARG
 *   (dnagpu_count_kmers_table's rule).
 * Window: [first, first + count) are rows of the STREAM, under dnagpu_generate_kmers_filtered's range rule: stream row p is
 *   the window of k bases at base p of the packed stream.  More than 2^32 - 1 stream rows in one call: DNAGPU_ERR_TOO_LARGE.
 *   A caller with buffers of cap rows pages with windows of cap stream rows (a window never holds more table rows than
 *   stream rows).
 * Table rows: stream row p is a table row when it lies inside one sequence: with s the sequence for which
 *   seq_starts[s] <= p < seq_starts[s+1], p + k <= seq_starts[s+1].  These are exactly the rows of every sequence's own
 *   generate_kmers (dna.c:781, in 64 bits): a sequence shorter than k has none; empty sequences, runs of them included, have
 *   none and are never an s.
 * Output: the table rows of the window that satisfy `filter`, in ascending p -- table order: sequence by sequence, position
 *   order inside a sequence (test.sql:86-92 per sequence).  out_keys[i] = the key, out_seq[i] = s (0-based, global, not
 *   relative to the window), out_pos[i] = p - seq_starts[s] (the row's ordinal inside its sequence's generate_kmers).  Any
 *   of the three arrays may be NULL; at most cap rows go to each; *n_out = all matching rows, even beyond cap.  The arrays
 *   are host memory, or device memory when out_on_device != 0 (8-byte aligned, at any parity relative to each other).
 * Filter: NULL = no WHERE, every table row matches.  Otherwise the operators of dnagpu_generate_kmers_filtered with its
 *   rules (EQUALS of another length matches nothing, a 32-base prefix compares 64 bits, 'U' matches nothing, a malformed
 *   filter -- bad kind, invalid qkmer text -- is always an error), except that the two operator ERRORs,
 *   DNAGPU_ERR_QKMER_LEN_MISMATCH (dna.c:1106-1108) and DNAGPU_ERR_PREFIX_TOO_LONG (dna.c:854-856), are raised exactly when
 *   the window holds at least one TABLE row: the reference raises them when the operator is first evaluated, and a window
 *   whose stream rows all span boundaries evaluates nothing (0 rows, DNAGPU_OK).
 * Checks, in order: NULL ctx / dna / n_out (DNAGPU_ERR_BAD_ARG), k (DNAGPU_ERR_INVALID_K, dna.c:772-773), the range, the
 *   missing set, the filter.  count == 0: *n_out = 0, DNAGPU_OK.  The table, its sequence set and the stream are untouched. */
int dnagpu_generate_kmers_table(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, const dnagpu_filter *filter,
                                uint64_t first, uint64_t count,
                                uint64_t *out_keys, uint64_t *out_seq, uint64_t *out_pos,
                                uint64_t cap, uint64_t *n_out, int out_on_device);
/* ---- sequences by id, and segments of a stream, as a new resident table ("give me those reads": what follows a
 * dnagpu_seq_hits_select, as input to the next count, hit or join) ----
 * dnagpu_dna_gather: segment i is bases [seg_first[i], seg_first[i] + seg_len[i]) of src's stream.  Any order; segments may
 *   overlap, repeat or be empty.  src needs no sequence set, and one it has is ignored: a segment may span boundaries.
 *   seg_flip may be NULL (no segment is flipped); a non-zero seg_flip[i] puts the reverse complement of segment i into the
 *   result, under dnagpu_dna_revcomp's definition: the complement is code ^ 1, base j comes from base seg_len[i] - 1 - j.
 * dnagpu_dna_take: the same where segment i is sequence seq_ids[i] of a table made resident with dnagpu_dna_set_sequences.
 *   Ids are global and 0-based, may repeat and come in any order; they are uint64 because that is what
 *   dnagpu_seq_hits_select writes to out_seq -- with on_device != 0 that buffer is passed straight in.
 * The lists are host memory, or device memory when on_device != 0 (all of them alike).
 * Result of both: a new owned dnagpu_dna (dnagpu_dna_free).  Its stream is the segments back to back in list order,
 *   ceil(total / 32) words, the bits behind the last base zero (dnagpu_dna_upload's rule).  It holds a resident sequence set
 *   of n sequences (the marks and n + 1 starts): segment i is sequence i, an empty segment an empty sequence, so every entry
 *   point that takes a resident table takes it.  n == 0 gives a valid dna of 0 bases with no set; n > 0 with a total of 0
 *   gives 0 bases and n empty sequences.  The result does not depend on src afterwards; src, its set and its words are only
 *   read, no word of src at or beyond its n_words is read and the result never depends on bits behind src's last base
 *   (dnagpu_dna_wrap's rule).  The call waits for its work.
 * Checks, in order: a NULL ctx, src / table or out, or a NULL seg_first / seg_len / seq_ids with n > 0, is
 *   DNAGPU_ERR_BAD_ARG; take on a non-empty stream without a sequence set is DNAGPU_ERR_BAD_ARG (dnagpu_count_kmers_table's
 *   rule); n > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE; a segment that leaves the stream (seg_first > length or seg_len > length -
 *   seg_first) or an id >= the table's sequences is DNAGPU_ERR_BAD_ARG -- found on the device, over all entries, before the
 *   result is allocated; a total above 2^32 - 1 bases is DNAGPU_ERR_TOO_LARGE (dnagpu_dna_set_sequences' own limit for a
 *   resident table, judged in 64 bits; callers page by id window, and windows tile); an allocation failure is
 *   DNAGPU_ERR_OOM.  On every error *out is left as it was and nothing stays allocated.
 * dnagpu_dna_sequence_starts: entries [first, first + count) of the n_seqs + 1 starts of dna's sequence set (a dna without a
 *   set has 0 entries), to host memory, or to device memory when out_on_device != 0, by dnagpu_ranking_read's window rule:
 *   first > entries or count > entries - first is DNAGPU_ERR_BAD_ARG; count == 0 is DNAGPU_OK.  A NULL ctx or dna, or a NULL
 *   out_starts with count > 0, is DNAGPU_ERR_BAD_ARG.  Waits for the copy. */
int dnagpu_dna_gather(dnagpu_ctx *ctx, const dnagpu_dna *src,
                      const uint64_t *seg_first, const uint64_t *seg_len, const uint8_t *seg_flip,
                      uint64_t n_segs, int on_device, dnagpu_dna **out);
int dnagpu_dna_take(dnagpu_ctx *ctx, const dnagpu_dna *table,
                    const uint64_t *seq_ids, const uint8_t *seq_flip,
                    uint64_t n_ids, int on_device, dnagpu_dna **out);
int dnagpu_dna_sequence_starts(dnagpu_ctx *ctx, const dnagpu_dna *dna, uint64_t first, uint64_t count,
                               uint64_t *out_starts, int out_on_device);
/* ---- a text file of sequences as a resident table (COPY dna_sequences (sequence) FROM '...' WITH (FORMAT text),
 * test.sql:128-130) ----
 * dnagpu_table_from_text: the raw bytes of a file -- DNAGPU_TEXT_LINES: one sequence per line; DNAGPU_TEXT_FASTA: '>' header
 *   lines open records -- are split, validated and packed on the device.  text is host memory, or device memory at any
 *   byte alignment when text_on_device != 0; no byte at or beyond text + n_bytes is read.
 * Result: a new owned dnagpu_dna (dnagpu_dna_free), exactly what dnagpu_dna_take returns.  Its stream is the records' bases
 *   back to back, ceil(bases / 32) words, the bits behind the last base zero.  It holds a resident sequence set of `records`
 *   sequences (the marks and records + 1 starts), so every entry point that takes a resident table takes it.  records == 0
 *   -- empty text, or with DNAGPU_TEXT_MORE a chunk that holds no finished record -- gives 0 bases and no set.
 * Characters: only A T C G are bases (validate_dna_sequence, dna.c:159-171).  A lower-case letter, N, a space, a tab, a
 *   backslash, and a '\r' that is not directly followed by '\n' are invalid characters.  A line ends at '\n'; a '\r'
 *   directly before that '\n' belongs to the terminator.
 * LINES: every line is a record; a last line without a terminator is a record, and text that ends in '\n' has no extra
 *   empty record.  An empty line is the reference's "DNA sequence cannot be empty" (dna.c:160-161): DNAGPU_ERR_DNA_EMPTY,
 *   reported at the offset of the line's first byte, which is its terminator.
 * FASTA: a line whose first byte is '>' is a header; the whole line is ignored and no byte of it is validated.  A header
 *   opens a record; the bases of the non-header lines that follow are joined into it; blank lines are ignored.  A record
 *   with no base is DNAGPU_ERR_DNA_EMPTY, reported at its '>'.  A base or an invalid character before the
 *   first header is DNAGPU_ERR_BAD_ARG at that byte ("sequence data before the first header").
 * Errors: every input error has a byte offset, and the one with the lowest offset wins (COPY stops at the first bad row).
 *   report (may be NULL) gets bad_pos, bad_record and bad_char; dnagpu_last_error() is the reference's message verbatim,
 *   "Invalid character in DNA sequence: %c" or "DNA sequence cannot be empty".  On every error *out is left as it was and
 *   nothing stays allocated; out_record_pos may then hold anything, and records / bases / consumed of the report are 0.
 * DNAGPU_TEXT_MORE: text is a chunk of a longer file, and its unfinished last record is held back.  LINES: only lines that
 *   end in '\n' are records, and consumed is one past the last '\n' (0: there is none).  FASTA: the record that the last
 *   header opens is held back, and consumed is the offset of that header's '>'; a chunk with no header and no sequence byte
 *   has consumed = n_bytes.  Bytes at or beyond consumed raise no error.  The caller prepends text[consumed ..] to the next
 *   chunk, and passes the file's last chunk without the flag.  consumed == 0 over a full chunk means that the record is longer
 *   than the chunk: the caller enlarges the chunk (to at most 2^32 - 1 bytes) and calls again.
 * out_record_pos (may be NULL with record_cap == 0): entry r is the byte offset of record r's first byte -- in FASTA its '>',
 *   so the caller reads the name from its own text.  At most record_cap entries are written.  It is host memory, or device
 *   memory when text_on_device != 0.
 * Checks, in order: a NULL ctx or out, a NULL text with n_bytes > 0, or a NULL out_record_pos with record_cap > 0, is
 *   DNAGPU_ERR_BAD_ARG; a format other than 1 or 2, or flags other than 0 or 1, is DNAGPU_ERR_BAD_ARG; n_bytes > 2^32 - 1 is
 *   DNAGPU_ERR_TOO_LARGE (the scans are 32-bit and a resident table holds at most 2^32 - 1 bases: larger files go chunk by
 *   chunk with DNAGPU_TEXT_MORE).  These need no device.  Then the input errors above, then DNAGPU_ERR_OOM.  The call
 *   waits for its work.
 * dnagpu_text_geometry: *tile_bytes = the bytes one workgroup sweeps (the edge shapes of the tests); needs no device. */
#define DNAGPU_TEXT_LINES 1   /* one sequence per line: COPY ... WITH (FORMAT text), test.sql:128-130 */
#define DNAGPU_TEXT_FASTA 2   /* '>' header lines open records; the sequence lines of a record are joined */
#define DNAGPU_TEXT_MORE  1u  /* flags: text is a chunk of a longer file; the unfinished last record is held back */
typedef struct dnagpu_text_report {
    uint64_t records;     /* sequences in the result */
    uint64_t bases;       /* bases in the result */
    uint64_t consumed;    /* bytes of text the result accounts for (== n_bytes without MORE) */
    uint64_t bad_pos;     /* on an input error: byte offset it is reported at, else ~0 */
    uint64_t bad_record;  /* on an input error: 0-based record it belongs to (~0: before the first record), else ~0 */
    char     bad_char;    /* DNAGPU_ERR_DNA_INVALID_CHAR: the character, else 0 */
    char     reserved[7];
} dnagpu_text_report;
int dnagpu_table_from_text(dnagpu_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device,
                           int format, unsigned flags, dnagpu_dna **out,
                           uint64_t *out_record_pos, uint64_t record_cap,
                           dnagpu_text_report *report);
int dnagpu_text_geometry(uint64_t *tile_bytes);
/* ---- FASTQ and real FASTA as a resident table (COPY reads (record, start, sequence) FROM 'x.fastq') ----
 * dnagpu_reads_from_text: dnagpu_table_from_text for the files that real data comes in: FASTQ records, IUPAC ambiguity
 *   letters under a policy, lower-case (soft-masked) bases, a minimal length, and for every sequence of the result where in
 *   the source it came from.  text, *out and the result are dnagpu_table_from_text's: an owned dnagpu_dna with a resident
 *   sequence set, exactly what dnagpu_dna_take returns; sequences == 0 gives a valid dna of 0 bases with no set.
 * 1. Byte classes in a sequence line.  Base: A T C G, and with DNAGPU_READS_FOLD_CASE also a t c g.  Ambiguity letter:
 *   N R Y K M S W B D H V, and with FOLD_CASE their lower case.  Terminator: '\n', and a '\r' directly before it.  Invalid:
 *   everything else -- U, X, '-', '*', digits, blanks, lower case without FOLD_CASE -- and DNAGPU_ERR_DNA_INVALID_CHAR under
 *   every policy.
 * 2. LINES and FASTA delimit records exactly as dnagpu_table_from_text does (header lines unvalidated, blank lines in FASTA
 *   ignored, data before the first header DNAGPU_ERR_BAD_ARG).  With ambiguous == DNAGPU_AMBIG_ERROR, flags & ~MORE == 0 and
 *   min_bases <= 1 the result is bit-identical to dnagpu_table_from_text's on the same bytes -- stream, starts, record_pos,
 *   report -- and so is every error: code, offset, record, character and dnagpu_last_error().
 * 3. FASTQ: strict four-line records.  Lines are numbered from 0 and end at '\n'; a last line without a terminator is a
 *   line, text that ends in '\n' has no extra one.  Line i belongs to record i / 4 and has role i % 4.  Role 0 must begin
 *   with '@', else DNAGPU_ERR_BAD_ARG at the line's first byte, "FASTQ record does not begin with '@'" (a blank line there
 *   is this error); the rest of the line is ignored.  Role 1 is the sequence line, classified as in 1; an empty one is
 *   DNAGPU_ERR_DNA_EMPTY at the line's first byte, as for LINES.  Role 2 must begin with '+', else DNAGPU_ERR_BAD_ARG at its
 *   first byte, "FASTQ separator line does not begin with '+'"; the rest is ignored.  Role 3 is the quality line: it is
 *   ignored whole, no byte of it is validated, and its length is NOT compared with the sequence's (that check would need the
 *   last four newline positions across tiles; it is left out on purpose).  Multi-line FASTQ is not supported.  Without
 *   MORE a line count that is no multiple of 4 is DNAGPU_ERR_BAD_ARG, "truncated FASTQ record", at the first byte of the
 *   unfinished record.  With MORE consumed is one past the '\n' that ends the last complete record (0: there is none), and
 *   nothing at or beyond it raises an error.  record_pos[r] is the offset of record r's '@'.
 * 4. Policies, over a record's sequence text S (its sequence bytes joined, terminators removed).  DNAGPU_AMBIG_ERROR: an
 *   ambiguity letter is DNAGPU_ERR_DNA_INVALID_CHAR with that letter.  DNAGPU_AMBIG_DROP: a record whose S holds an
 *   ambiguity letter contributes nothing and counts in dropped; every other record is one sequence with src_offset 0.
 *   DNAGPU_AMBIG_SPLIT: every maximal run of bases in S is one sequence, in order; src_offset is the index in S of the run's
 *   first base (the coordinate in the original sequence, ambiguity letters counted); a non-empty S with no base contributes
 *   nothing and is no error.  Under every policy an S with no byte at all is DNAGPU_ERR_DNA_EMPTY; a sequence shorter than
 *   min_bases is left out and counts in short_out; src_record is the 0-based source record, the index into record_pos.
 *   Deleting the ambiguity letters and joining the flanks is deliberately not offered: it invents k-mers.
 * 5. Errors: every input error has a byte offset, and the lowest offset wins; at equal offsets a bad '@' or '+' comes before
 *   empty, before invalid character, before truncated.  report gets bad_pos, bad_record and bad_char as dnagpu_text_report.
 *   On every error *out is left as it was and nothing stays allocated; the output arrays may then hold anything.
 * 6. out_record_pos: per SOURCE record, at most record_cap entries.  out_src_record / out_src_offset: per sequence of the
 *   RESULT, at most seq_cap entries each.  All three are host memory, or device memory when text_on_device != 0.
 * 7. Checks, in order, none needs a device: a NULL ctx, opt or out; a NULL text with n_bytes > 0; a NULL array with a
 *   non-zero cap; only one of the two src arrays given with seq_cap > 0 -- all DNAGPU_ERR_BAD_ARG; then a format, ambiguous,
 *   flags or reserved out of range, DNAGPU_ERR_BAD_ARG; then n_bytes > 2^32 - 1, DNAGPU_ERR_TOO_LARGE.  Then the input
 *   errors, then DNAGPU_ERR_OOM.  The call waits for its work.  The success path reads back once; a second read-back (the
 *   counts of what stays) happens only where DROP met an ambiguity letter or min_bases > 1. */
#define DNAGPU_TEXT_FASTQ 3            /* strict four-line records: @name / sequence / +[name] / quality */

#define DNAGPU_AMBIG_ERROR 0           /* an IUPAC ambiguity letter is an invalid character (dnagpu_table_from_text's rule) */
#define DNAGPU_AMBIG_DROP  1           /* a record that holds one is left out of the result */
#define DNAGPU_AMBIG_SPLIT 2           /* a record is cut at every run of them: each maximal run of bases is a sequence */

#define DNAGPU_READS_MORE      1u      /* == DNAGPU_TEXT_MORE */
#define DNAGPU_READS_FOLD_CASE 2u      /* a c g t are bases; lower-case ambiguity letters are ambiguity letters */

typedef struct dnagpu_reads_options {
    int      format;      /* DNAGPU_TEXT_LINES, _FASTA or _FASTQ */
    int      ambiguous;   /* DNAGPU_AMBIG_* */
    unsigned flags;       /* DNAGPU_READS_* */
    unsigned reserved;    /* must be 0 */
    uint64_t min_bases;   /* sequences of the result shorter than this are left out (0 and 1: none is) */
} dnagpu_reads_options;

typedef struct dnagpu_reads_report {
    uint64_t records;     /* source records accounted for (finished records of text[0 .. consumed)) */
    uint64_t sequences;   /* sequences in the result */
    uint64_t bases;       /* bases in the result */
    uint64_t consumed;    /* bytes of text the result accounts for (== n_bytes without MORE) */
    uint64_t ambiguous;   /* ambiguity letters met in sequence lines */
    uint64_t dropped;     /* DROP: records left out for an ambiguity letter */
    uint64_t short_out;   /* sequences left out by min_bases */
    uint64_t bad_pos, bad_record;   /* as dnagpu_text_report */
    char     bad_char, reserved[7];
} dnagpu_reads_report;

int dnagpu_reads_from_text(dnagpu_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device,
                           const dnagpu_reads_options *opt, dnagpu_dna **out,
                           uint64_t *out_record_pos, uint64_t record_cap,      /* per SOURCE record: offset of its first byte */
                           uint64_t *out_src_record, uint64_t *out_src_offset, uint64_t seq_cap,   /* per RESULT sequence */
                           dnagpu_reads_report *report);
/* ---- a resident table as text, FASTA or FASTQ (COPY dna_sequences (sequence) TO '...'; dna_out -> decode_dna, dna.c:135-152,
 * 230-239, once per row) ----
 * The text image of a table is the file that the loaders above would read back into the same table.  dnagpu_table_to_text
 *   plans it -- it is never materialised --, dnagpu_text_image_read forms any byte window of it on the device, and
 *   dnagpu_text_image_free releases the plan (dnagpu_ranking's shape).
 * The image is record after record, in table order.  T is the terminator ("\n", or "\r\n" with DNAGPU_TEXT_OUT_CRLF), len
 *   the sequence's bases, name = name_prefix followed by the record's number in decimal without padding (1 .. 20 digits); the
 *   number of sequence s is numbers[s], or name_base + s (mod 2^64) when numbers is NULL.  Codes 0 .. 3 are A T C G.
 *   LINES: the bases, T (prefix, base and numbers are ignored).
 *   FASTA: '>' name T, then the bases in lines of line_width bases, each followed by T; the last line may be shorter, there is
 *     never an empty line, and line_width == 0 or >= len gives one line.
 *   FASTQ: '@' name T, the bases, T, '+' T, the quality byte len times, T.
 * A sequence of 0 bases (dnagpu_dna_take can return such tables) is written as what it is -- LINES a bare T, FASTA a header
 *   with no sequence line, FASTQ four lines of which two are empty -- and counted in dnagpu_text_image_empty: the loaders
 *   refuse such records, the caller is told, nothing is invented.
 * Round trip: for a table without empty sequences the whole image, given to dnagpu_table_from_text (LINES, FASTA) or
 *   dnagpu_reads_from_text (FASTQ), yields bit-identical words and starts, and the loader's record_pos equals
 *   dnagpu_text_image_record_pos.
 * Lifetime: the image holds copies of the options, the prefix and the numbers, and one offset per sequence in pool memory;
 *   it BORROWS the table, whose stream and sequence set are read by every dnagpu_text_image_read -- the caller keeps the
 *   table alive and its set unchanged until dnagpu_text_image_free (dnagpu_table_classes' rule).  The table is only read: no
 *   word at or beyond its n_words, and no byte of the image depends on bits behind the last base (dnagpu_dna_wrap's rule).
 *   A table of 0 sequences gives an image of 0 bytes that holds no device memory.
 * Checks of dnagpu_table_to_text, in order (the first three need no device): a NULL ctx, table, opt or out is
 *   DNAGPU_ERR_BAD_ARG; a format outside 1 .. 3, flags other than 0 or 1, non-zero reserved bytes, prefix_len > 64, a NULL
 *   prefix with prefix_len > 0, a '\n' or '\r' in the prefix, a quality byte outside 33 .. 126 (0 means 'I'), or line_width
 *   != 0 with LINES or FASTQ, is DNAGPU_ERR_BAD_ARG; a non-empty stream without a sequence set is DNAGPU_ERR_BAD_ARG
 *   (dnagpu_count_kmers_table's rule); more than 2^32 - 1 bytes of the image that are no bases of a sequence line (headers,
 *   terminators, '+' and quality lines; summed in 64 bits on the device before anything is scanned) is DNAGPU_ERR_TOO_LARGE
 *   -- callers split such tables with dnagpu_dna_take; an allocation failure is DNAGPU_ERR_OOM with nothing leaked.  On every
 *   error *out is left as it was.  The call waits for its work and reads back once.
 * dnagpu_text_image_read: bytes [first_byte, first_byte + count) of the image to out_text -- host memory, or device memory
 *   at any byte alignment when out_on_device != 0.  Exactly count bytes are written, no NUL, and no byte of the destination
 *   outside them is written or read.  dnagpu_ranking_read's window rule: first_byte > bytes or count > bytes - first_byte is
 *   DNAGPU_ERR_BAD_ARG; count == 0 is DNAGPU_OK; count > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE (callers page).  Windows tile: the
 *   concatenation of any partition of [0, bytes) is the image.  Offsets are 64-bit throughout.  Waits for its work.
 * dnagpu_text_image_record_pos: entry s = the offset of record s's first byte; sequences + 1 entries, the last = bytes (an
 *   image of 0 sequences has 0 entries); dnagpu_dna_sequence_starts' window rule.
 * dnagpu_text_out_geometry: *tile_bytes = the bytes one workgroup forms (the edge shapes of the tests); needs no device. */
typedef struct dnagpu_text_image dnagpu_text_image;

#define DNAGPU_TEXT_OUT_CRLF 1u            /* every terminator is "\r\n" instead of "\n" */

typedef struct dnagpu_text_out_options {
    int         format;        /* DNAGPU_TEXT_LINES, DNAGPU_TEXT_FASTA or DNAGPU_TEXT_FASTQ (the loaders' constants) */
    unsigned    flags;         /* DNAGPU_TEXT_OUT_* */
    uint32_t    line_width;    /* FASTA: bases per sequence line; 0 = the whole sequence on one line.  Must be 0 for LINES / FASTQ */
    uint32_t    prefix_len;    /* bytes of name_prefix, <= 64 */
    const char *name_prefix;   /* host memory; copied; no '\n' or '\r' in it; may be NULL when prefix_len == 0 */
    uint64_t    name_base;     /* the number in sequence s's header is name_base + s (mod 2^64) ... */
    const uint64_t *numbers;   /* ... or numbers[s] when this is not NULL: n_seqs entries, copied by the call */
    int         numbers_on_device;
    char        quality;       /* FASTQ: the byte that fills every quality line, 33..126; 0 means 'I' */
    char        reserved[3];   /* must be 0 */
} dnagpu_text_out_options;

int      dnagpu_table_to_text(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_text_out_options *opt, dnagpu_text_image **out);
uint64_t dnagpu_text_image_bytes(const dnagpu_text_image *img);       /* size of the whole image; 0 for NULL */
uint64_t dnagpu_text_image_sequences(const dnagpu_text_image *img);
uint64_t dnagpu_text_image_empty(const dnagpu_text_image *img);       /* sequences of 0 bases in it */
int      dnagpu_text_image_read(dnagpu_ctx *ctx, const dnagpu_text_image *img, uint64_t first_byte, uint64_t count,
                                char *out_text, int out_on_device);
int      dnagpu_text_image_record_pos(dnagpu_ctx *ctx, const dnagpu_text_image *img, uint64_t first_seq, uint64_t count,
                                      uint64_t *out_pos, int out_on_device);
void     dnagpu_text_image_free(dnagpu_ctx *ctx, dnagpu_text_image *img);
int      dnagpu_text_out_geometry(uint64_t *tile_bytes);              /* bytes one workgroup forms; needs no device */

/* ---- The quality column of a table of reads: dnagpu_quals.
 *
 * A column is an owned object (dnagpu_quals_free) of n bytes in device memory: byte b is the raw Phred+33 character of
 *   base b of a table's stream.  It holds no boundaries of its own: every call that needs them takes the table too, and
 *   answers DNAGPU_ERR_BAD_ARG when dnagpu_dna_length(table) != dnagpu_quals_bases(q).  Every byte of a column is in 33 ..
 *   126; that is checked wherever a column is made, so no later call has an error path for it.
 * dnagpu_quals_upload: a column from the caller's n bytes (host memory, or device memory when on_device != 0).  A byte
 *   outside 33 .. 126 is DNAGPU_ERR_BAD_ARG, "invalid FASTQ quality character"; the lowest offset is found on the device
 *   and reported with the character in report->bad_pos / bad_char (report may be NULL).  A NULL ctx or out, or NULL bytes
 *   with n > 0, is DNAGPU_ERR_BAD_ARG; n > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE (a resident table's limit).  n == 0 gives a
 *   valid column of 0 bytes.
 * dnagpu_quals_bases: n (0 for NULL).  dnagpu_quals_read: bytes [first, first + count) to out (host memory, or device
 *   memory when out_on_device != 0) by dnagpu_ranking_read's window rule: first > n or count > n - first is
 *   DNAGPU_ERR_BAD_ARG; count == 0 is DNAGPU_OK; a NULL ctx or q, or a NULL out with count > 0, is DNAGPU_ERR_BAD_ARG.
 *
 * dnagpu_quals_from_fastq: the column of the table that dnagpu_reads_from_text made from the same bytes.
 *   text[0 .. n_bytes) is whole FASTQ records (with DNAGPU_READS_MORE the caller passes the loader's `consumed`);
 *   src_record / src_offset are the arrays the loader wrote, one entry per sequence of the table (device memory iff
 *   text_on_device; both NULL: sequence s is record s at offset 0).  The qualities of sequence s, of len_s bases, are bytes
 *   [src_offset[s], src_offset[s] + len_s) of the quality line of record src_record[s]; they are placed at the sequence's
 *   place in the stream.  DROP, SPLIT and min_bases are covered by this with no policy here.
 *   Input errors carry a byte offset (report->bad_pos, and the record in bad_record); the lowest offset wins, and at one
 *   offset a length error comes before a character error.  A line count that is no multiple of 4 is DNAGPU_ERR_BAD_ARG,
 *   "truncated FASTQ record", at the first byte of the unfinished record.  A quality line whose length differs from its
 *   sequence line's is DNAGPU_ERR_BAD_ARG, "FASTQ quality line length differs from the sequence's", at the quality line's
 *   first byte; lengths are taken without the terminator, and a '\r' directly before '\n' belongs to the terminator (the
 *   check dnagpu_reads_from_text leaves out).  A byte outside 33 .. 126 in a quality line is the error of
 *   dnagpu_quals_upload at that byte.  '@' and '+' are not looked at again: the loader owns that check.
 *   Checks, in order: a NULL ctx, table or out, or NULL text with n_bytes > 0, is DNAGPU_ERR_BAD_ARG; only one of the two
 *   src arrays is DNAGPU_ERR_BAD_ARG; a non-empty stream without a sequence set is DNAGPU_ERR_BAD_ARG; n_bytes > 2^32 - 1 is
 *   DNAGPU_ERR_TOO_LARGE.  These need no device.  Then the input errors; then the sources: src_record[s] >= the text's
 *   records, or src_offset[s] + len_s beyond that record's quality line, is DNAGPU_ERR_BAD_ARG with no offset.  On every
 *   error *out is left as it was and nothing stays allocated.  The call waits for its work.
 *
 * dnagpu_quals_gather / dnagpu_quals_take: the arguments, the checks in their order and the limits of dnagpu_dna_gather /
 *   dnagpu_dna_take, over the column (gather: segments of src's bytes; take: sequences of `table`, whose column `quals`
 *   is -- a column of another length is DNAGPU_ERR_BAD_ARG, checked after the missing sequence set).  Given the same lists,
 *   the result is the column of the table those two return.  A flipped segment is reversed: qualities have no complement.
 *
 * dnagpu_text_image_read_quals: dnagpu_text_image_read with every quality line of the image taken from the column -- the
 *   quality line of sequence s is the column's bytes [starts[s], starts[s + 1]) -- and dnagpu_text_out_options.quality
 *   ignored.  The image must be FASTQ and dnagpu_quals_bases(quals) the bases of the image's table, else
 *   DNAGPU_ERR_BAD_ARG (after the NULL checks, before the window's).  The window rule, the any-alignment rule and the "no
 *   byte outside the window is touched" rule are dnagpu_text_image_read's; windows tile; every byte outside a quality line
 *   is what dnagpu_text_image_read writes.
 *
 * dnagpu_quals_trim: quality trimming and quality filtering of every sequence of a table, on the device.  The Phred value
 *   of a byte is byte - 33.  For a sequence with values q[0 .. n) the cut points are cutadapt's / BWA's, each computed over
 *   the whole sequence:
 *     front (cut_front = F; F == 0: start = 0):  s = 0, best = 0, start = 0
 *         for i = 0 .. n-1:  s += F - q[i];  if s < 0: break;  if s > best: best = s, start = i + 1
 *     tail  (cut_tail = T; T == 0: stop = n):    s = 0, best = 0, stop = n
 *         for i = n-1 .. 0:  s += T - q[i];  if s < 0: break;  if s > best: best = s, stop = i
 *     if start >= stop: start = stop = 0
 *   Per sequence s, over [start, stop), all uint64: out_first[s] = starts[s] + start (a stream coordinate), out_len[s] the
 *   kept length, out_qsum[s] the sum of the values, out_low[s] the bases with a value < low_q.  With len the kept length a
 *   sequence passes iff len > 0, len >= min_bases, qsum >= min_mean_q * len and low * low_den <= low_num * len (64-bit
 *   integer comparisons; low_den == 0 switches the last test off); a failing sequence is counted under the first criterion
 *   it fails, in the order short, mean, low.  The passing sequences are written in table order as seg_seq / seg_first /
 *   seg_len, at most seg_cap of them (the report carries the full count): lists that go straight into dnagpu_dna_gather
 *   and dnagpu_quals_gather.  Every output is host memory, or device memory when out_on_device != 0; any may be NULL.
 *   The report: sequences, passed, bases_in, bases_kept, the bases cut in front (start) and at the tail (n - stop), summed
 *   over all sequences after the start >= stop rule -- a sequence cut away whole counts at the tail -- so that bases_in =
 *   bases_kept + cut_front + cut_tail, and the three failure counts.  It is the call's only read-back.
 *   Checks, in order: a NULL ctx, table, quals or opt is DNAGPU_ERR_BAD_ARG; cut_front, cut_tail, min_mean_q or low_q above
 *   255, or a non-zero reserved, is DNAGPU_ERR_BAD_ARG; a non-empty stream without a sequence set is DNAGPU_ERR_BAD_ARG; a
 *   column of another length than the table is DNAGPU_ERR_BAD_ARG.  These need no device.  The call waits for its work.
 *   dnagpu_quals_geometry names the paths by length (needs no device): a sequence of at most group_bases bases is handled
 *   by a group of 16 lanes of one wave, one of at most wave_bases by a wave, one of at most tile_bases by a workgroup in
 *   one tile, a longer one by a workgroup tile after tile. */
typedef struct dnagpu_quals dnagpu_quals;
typedef struct dnagpu_quals_trim_options {
    uint32_t cut_front;   /* F; 0: no cut in front */
    uint32_t cut_tail;    /* T; 0: no cut at the tail */
    uint32_t min_mean_q;  /* passes iff qsum >= min_mean_q * len */
    uint32_t low_q;       /* a base is low iff its value < low_q */
    uint32_t low_num;     /* passes iff low * low_den <= low_num * len; low_den == 0: no such test */
    uint32_t low_den;
    uint64_t min_bases;   /* passes iff len >= min_bases (and len > 0) */
    uint64_t reserved;    /* 0 */
} dnagpu_quals_trim_options;
typedef struct dnagpu_quals_trim_report {
    uint64_t sequences, passed, bases_in, bases_kept, cut_front, cut_tail, failed_short, failed_mean, failed_low;
} dnagpu_quals_trim_report;
int      dnagpu_quals_trim(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_quals *quals, const dnagpu_quals_trim_options *opt,
                           uint64_t *out_first, uint64_t *out_len, uint64_t *out_qsum, uint64_t *out_low, uint64_t *seg_seq,
                           uint64_t *seg_first, uint64_t *seg_len, uint64_t seg_cap, int out_on_device,
                           dnagpu_quals_trim_report *report);
int      dnagpu_quals_geometry(uint64_t *group_bases, uint64_t *wave_bases, uint64_t *tile_bases);
typedef struct dnagpu_quals_report {
    uint64_t records;     /* dnagpu_quals_from_fastq: whole records of the text (0 when the call failed before counting) */
    uint64_t bad_pos;     /* an input error: the byte offset; ~0 otherwise */
    uint64_t bad_record;  /* dnagpu_quals_from_fastq: the record bad_pos lies in; ~0 otherwise */
    char     bad_char;    /* "invalid FASTQ quality character": the character, else 0 */
    char     reserved[7];
} dnagpu_quals_report;
int      dnagpu_quals_upload(dnagpu_ctx *ctx, const char *bytes, uint64_t n, int on_device, dnagpu_quals **out,
                             dnagpu_quals_report *report);
uint64_t dnagpu_quals_bases(const dnagpu_quals *q);
int      dnagpu_quals_read(dnagpu_ctx *ctx, const dnagpu_quals *q, uint64_t first, uint64_t count, char *out, int out_on_device);
void     dnagpu_quals_free(dnagpu_ctx *ctx, dnagpu_quals *q);
int      dnagpu_quals_from_fastq(dnagpu_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device, const dnagpu_dna *table,
                                 const uint64_t *src_record, const uint64_t *src_offset, dnagpu_quals **out,
                                 dnagpu_quals_report *report);
int      dnagpu_quals_gather(dnagpu_ctx *ctx, const dnagpu_quals *src, const uint64_t *seg_first, const uint64_t *seg_len,
                             const uint8_t *seg_flip, uint64_t n_segs, int on_device, dnagpu_quals **out);
int      dnagpu_quals_take(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_quals *quals, const uint64_t *seq_ids,
                           const uint8_t *seq_flip, uint64_t n_ids, int on_device, dnagpu_quals **out);
int      dnagpu_text_image_read_quals(dnagpu_ctx *ctx, const dnagpu_text_image *img, const dnagpu_quals *quals,
                                      uint64_t first_byte, uint64_t count, char *out_text, int out_on_device);
/* bytes one lane and one workgroup of the column copy form, and the most segments of a tile it stages in LDS; needs no device.
 * It is here for the reason dnagpu_text_geometry, dnagpu_text_out_geometry and dnagpu_quals_geometry are: the copy takes another
 * path past each of these sizes, and a caller's tests can only place their cases on the edges if the library names them. */
int      dnagpu_quals_copy_geometry(uint64_t *chunk_bytes, uint64_t *tile_bytes, uint64_t *lds_segments);

/* ---- Adapter trimming: dnagpu_dna_adapters.  Segments in, segments out.
 *
 * The 3' adapter cut of every segment of a packed stream, with mismatches and IUPAC letters, on the device.
 *   Input: src, and n_segs segments of its stream: seg_first / seg_len are stream coordinates (uint64; host memory, or device
 *   memory when on_device != 0) -- exactly what dnagpu_quals_trim writes as seg_first / seg_len or as out_first / out_len.
 *   Both NULL: segment i is sequence i of the table's set (src must then have a set, and n_segs must not exceed its
 *   sequences).  seg_seq (optional, as the lists) is carried through unchanged to pass_seq; NULL: the id is i.
 *   Adapters: n_adapters (1 .. 32) NUL-terminated texts of 1 .. 32 letters of the qkmer alphabet, validated by the routine
 *   `@>` is validated by; 'U' matches no base, as it does there.  S_a[j] = the set of letter j of adapter a, L_a its length.
 *   The match rule -- Hamming distance only, no insertions or deletions.  For a segment with the bases b[0 .. n), a position
 *   p in 0 .. n-1 and an adapter a:  o = min(L_a, n - p),  m = #{ j < o : b[p + j] not in S_a[j] };  (p, a) is a hit iff
 *   o >= min(min_overlap, L_a) and m * err_den <= err_num * o (64-bit integer comparisons).  The segment's cut is the hit with
 *   the least (p, m, a) in lexicographic order: the lowest position wins (the "first position" rule of fastp and
 *   Trimmomatic), at one position the fewest mismatches, then the lowest adapter index.  With no hit nothing is cut.  No base
 *   outside [seg_first, seg_first + seg_len) is ever compared -- a partial overlap at the end of a read does not look at the
 *   head of the next one -- and words[n_words] is never read.
 *   Outputs, all uint64, host memory or device memory when out_on_device != 0; any may be NULL.  Per input segment i:
 *   out_len[i] = p of the cut, or n; out_adapter[i] = a, or ~0; out_mismatch[i] = m, or 0.  A segment passes iff its kept
 *   length is > 0 and >= min_bases and no discard flag excludes it (DISCARD_UNTRIMMED: the segments without a hit;
 *   DISCARD_TRIMMED: those with one).  The passing segments come in input order as pass_seq / pass_first / pass_len, at most
 *   pass_cap of them (the report carries the full count): lists that go straight into dnagpu_dna_gather, dnagpu_quals_gather
 *   and dnagpu_names_take.  The report (cleared on entry; its read is the call's only read-back on the success path):
 *   segments, passed, trimmed (segments with a hit), bases_in = bases_kept + bases_cut over all segments, failing ones
 *   included, failed_short and failed_discarded (in that order of precedence), and per_adapter[a] = the segments cut by
 *   adapter a.
 *   Checks, in order: a NULL ctx, src, opt or adapters (or a NULL text) is DNAGPU_ERR_BAD_ARG; an adapter count outside
 *   1 .. 32, a length outside 1 .. 32, err_den == 0, err_num > err_den, min_overlap outside 1 .. 32, unknown flags, both
 *   discard flags, or a non-zero reserved is DNAGPU_ERR_BAD_ARG; a letter outside the alphabet is DNAGPU_ERR_QKMER_INVALID;
 *   only one of seg_first / seg_len is DNAGPU_ERR_BAD_ARG; both NULL on a non-empty stream without a set, or with n_segs above
 *   the set's sequences, is DNAGPU_ERR_BAD_ARG; n_segs > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE.  These need no device.  Then, found
 *   on the device over all entries before any output is written, a segment that leaves the stream (seg_first > length or
 *   seg_len > length - seg_first) is DNAGPU_ERR_BAD_ARG.  On every error the outputs are untouched.  n_segs == 0 is DNAGPU_OK
 *   with an all-zero report.  The call waits for its work.
 *   dnagpu_adapters_geometry names the paths by segment length (needs no device): at most group_bases bases are handled by a
 *   group of 16 lanes of one wave, at most wave_bases by a wave, more by a workgroup in tiles of tile_bases positions, from
 *   the front until a tile holds a hit. */
#define DNAGPU_ADAPTERS_DISCARD_UNTRIMMED 1u
#define DNAGPU_ADAPTERS_DISCARD_TRIMMED   2u
typedef struct dnagpu_adapters_options {
    uint32_t err_num;      /* a hit has m * err_den <= err_num * o */
    uint32_t err_den;      /* >= 1, err_num <= err_den */
    uint32_t min_overlap;  /* 1 .. 32; for adapter a: min(min_overlap, L_a) */
    uint32_t flags;        /* DNAGPU_ADAPTERS_DISCARD_*; not both */
    uint64_t min_bases;    /* passes iff the kept length >= min_bases (and > 0) */
    uint64_t reserved;     /* 0 */
} dnagpu_adapters_options;
typedef struct dnagpu_adapters_report {
    uint64_t segments, passed, trimmed, bases_in, bases_kept, bases_cut, failed_short, failed_discarded;
    uint64_t per_adapter[32];
} dnagpu_adapters_report;
int      dnagpu_dna_adapters(dnagpu_ctx *ctx, const dnagpu_dna *src, const char *const *adapters, uint32_t n_adapters,
                             const dnagpu_adapters_options *opt, const uint64_t *seg_seq, const uint64_t *seg_first,
                             const uint64_t *seg_len, uint64_t n_segs, int on_device, uint64_t *out_len, uint64_t *out_adapter,
                             uint64_t *out_mismatch, uint64_t *pass_seq, uint64_t *pass_first, uint64_t *pass_len,
                             uint64_t pass_cap, int out_on_device, dnagpu_adapters_report *report);
int      dnagpu_adapters_geometry(uint64_t *group_bases, uint64_t *wave_bases, uint64_t *tile_bases);

/* ---- The names column of a table of reads: dnagpu_names.
 *
 * A column is an owned object (dnagpu_names_free) of variable-length byte strings, one per sequence of a table: n + 1
 *   uint64 offsets (offsets[0] = 0, non-decreasing) and offsets[n] bytes in device memory; string s is bytes [offsets[s],
 *   offsets[s + 1]).  No byte of a column is '\n' or '\r'; that is checked wherever a column is made, so no later call has
 *   an error path for it.  An empty string is a name ("@\n" is a header the loaders accept).  A column holds at most 2^32 - 1
 *   strings and 2^32 - 1 bytes.  On every error of every call below *out is left as it was and nothing stays allocated.
 * dnagpu_names_upload: a column from the caller's arrays (both host memory, or both device memory when on_device != 0).
 *   Checks, in order: a NULL ctx or out, or NULL offsets with n > 0, is DNAGPU_ERR_BAD_ARG; n > 2^32 - 1 is
 *   DNAGPU_ERR_TOO_LARGE; NULL bytes with offsets[n] != 0 is DNAGPU_ERR_BAD_ARG (host offsets: here; device offsets: after the
 *   total below).  These need no device.  Then, on the device over all entries: offsets[0] != 0 or a decreasing pair is
 *   DNAGPU_ERR_BAD_ARG; offsets[n] > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE; a '\n' or '\r' is DNAGPU_ERR_BAD_ARG, "invalid character
 *   in a read name": the lowest offset is found on the device and reported with the character in report->bad_pos / bad_char
 *   (report may be NULL; bad_record stays ~0).  n == 0 gives a valid empty column (offsets and bytes are not looked at).
 * dnagpu_names_sequences / dnagpu_names_bytes: n and offsets[n]; 0 for NULL; no device.
 * dnagpu_names_offsets: entries [first, first + count) of the n + 1 offsets to out (host memory, or device memory when
 *   out_on_device != 0) by dnagpu_dna_sequence_starts' window rule: first > n + 1 or count > n + 1 - first is
 *   DNAGPU_ERR_BAD_ARG; count == 0 is DNAGPU_OK; a NULL ctx or names, or NULL out with count > 0, is DNAGPU_ERR_BAD_ARG.
 * dnagpu_names_read: bytes [first_byte, first_byte + count) of the column by dnagpu_quals_read's window rule.
 *
 * dnagpu_names_from_text: the names of the table that dnagpu_reads_from_text (or dnagpu_table_from_text, FASTA) made from
 *   the same bytes.  format is DNAGPU_TEXT_FASTA or DNAGPU_TEXT_FASTQ.  record_pos is the array the loader wrote, n_records
 *   entries: the offset of each source record's '>' or '@'.  src_record is the loader's per-sequence array, n_seqs entries;
 *   NULL: sequence s is record s, and n_seqs must equal n_records.  Both are device memory iff text_on_device.  With
 *   DNAGPU_READS_MORE the caller passes the loader's `consumed` as n_bytes, or the whole chunk: a name never reaches beyond
 *   its line.
 *   The header line of record r starts at record_pos[r] and ends before the first '\n' at or after that byte, or at n_bytes
 *   if there is none; a '\r' directly before that '\n' belongs to the terminator.  The name of sequence s is that line of
 *   record src_record[s] without its first byte; with flags & DNAGPU_NAMES_FIRST_WORD it is cut before its first ' ' or
 *   '\t'.  Under SPLIT every piece of a record gets a copy of the record's name; nothing is appended or invented.
 *   Checks, in order: a NULL ctx or out, NULL text with n_bytes > 0, or NULL record_pos with n_records > 0, is
 *   DNAGPU_ERR_BAD_ARG; a format other than FASTA or FASTQ (DNAGPU_TEXT_LINES has no names) is DNAGPU_ERR_BAD_ARG; flags other
 *   than 0 or 1 are DNAGPU_ERR_BAD_ARG; NULL src_record with n_seqs != n_records is DNAGPU_ERR_BAD_ARG; n_bytes, n_records or
 *   n_seqs > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE.  These need no device.  n_seqs == 0 gives a valid empty column.  Then, found on
 *   the device over all entries: record_pos[r] >= n_bytes for a record some sequence names, a byte there that is not the
 *   format's marker, or src_record[s] >= n_records, is DNAGPU_ERR_BAD_ARG with no offset.  Then a 64-bit total of the names
 *   above 2^32 - 1 is DNAGPU_ERR_TOO_LARGE, judged before the column is allocated.  Then a '\r' that remains inside a name
 *   is DNAGPU_ERR_BAD_ARG, "invalid character in a read name": report->bad_pos is the text offset of the first such byte in
 *   the lowest-numbered sequence whose name has one, bad_record its record, bad_char '\r'.
 *   The call waits for its work.  The success path reads back once; a second read-back happens only where the text holds a
 *   '\r' that no '\n' follows (anywhere: such a text has its names validated after the copy).
 * dnagpu_names_take: the names of the sequences seq_ids[0 .. n_ids) in that order -- dnagpu_dna_take's rules: ids may repeat
 *   and come in any order, they are uint64, host memory or device memory when on_device != 0 (the buffer of
 *   dnagpu_seq_hits_select or the seg_seq of dnagpu_quals_trim goes straight in).  A NULL ctx, names or out, or NULL seq_ids
 *   with n_ids > 0, is DNAGPU_ERR_BAD_ARG; n_ids > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE (no device).  An id >= the column's
 *   sequences is DNAGPU_ERR_BAD_ARG, found over all entries before anything is allocated for the result; a total above
 *   2^32 - 1 bytes is DNAGPU_ERR_TOO_LARGE.  n_ids == 0 gives a valid empty column.  Given the same ids, the result is the
 *   names of the table dnagpu_dna_take returns.
 * dnagpu_table_to_text_named: dnagpu_table_to_text where the name of sequence s is the column's string s; name_prefix,
 *   name_base and numbers are ignored (prefix_len must still be <= 64).  Checks, in order: a NULL ctx, table, names, opt or
 *   out; the option checks of dnagpu_table_to_text; a format that is not FASTA or FASTQ; a non-empty stream without a
 *   sequence set; dnagpu_names_sequences(names) != the table's sequences -- all DNAGPU_ERR_BAD_ARG and without a device; then
 *   the limit on the bytes that are no bases, DNAGPU_ERR_TOO_LARGE.  The result is an ordinary dnagpu_text_image:
 *   dnagpu_text_image_bytes, _read, _record_pos, _read_quals, _free, the window and tiling rules and the "no byte outside the
 *   window is touched" rule hold unchanged.  The image BORROWS the column as it borrows the table.
 * dnagpu_names_geometry (no device): the sweep of dnagpu_names_from_text marks the bytes that end a name per chunk_bytes of
 *   text; a name ends in the marks of the tile of tile_bytes it begins in, or else where a suffix minimum over the tiles
 *   says, which is formed in groups of group_tiles tiles and then over the groups. */
typedef struct dnagpu_names dnagpu_names;
#define DNAGPU_NAMES_FIRST_WORD 1u     /* a name ends before its first ' ' or '\t' */
typedef struct dnagpu_names_report {
    uint64_t bad_pos;     /* "invalid character in a read name": upload: the offset in bytes; from_text: in the text; ~0 otherwise */
    uint64_t bad_record;  /* dnagpu_names_from_text: the record bad_pos lies in; ~0 otherwise */
    char     bad_char;    /* the character, else 0 */
    char     reserved[7];
} dnagpu_names_report;
int      dnagpu_names_upload(dnagpu_ctx *ctx, const char *bytes, const uint64_t *offsets, uint64_t n, int on_device,
                             dnagpu_names **out, dnagpu_names_report *report);
uint64_t dnagpu_names_sequences(const dnagpu_names *names);
uint64_t dnagpu_names_bytes(const dnagpu_names *names);
int      dnagpu_names_offsets(dnagpu_ctx *ctx, const dnagpu_names *names, uint64_t first, uint64_t count, uint64_t *out,
                              int out_on_device);
int      dnagpu_names_read(dnagpu_ctx *ctx, const dnagpu_names *names, uint64_t first_byte, uint64_t count, char *out,
                           int out_on_device);
void     dnagpu_names_free(dnagpu_ctx *ctx, dnagpu_names *names);
int      dnagpu_names_from_text(dnagpu_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device, int format, unsigned flags,
                                const uint64_t *record_pos, uint64_t n_records, const uint64_t *src_record, uint64_t n_seqs,
                                dnagpu_names **out, dnagpu_names_report *report);
int      dnagpu_names_take(dnagpu_ctx *ctx, const dnagpu_names *names, const uint64_t *seq_ids, uint64_t n_ids, int on_device,
                           dnagpu_names **out);
int      dnagpu_table_to_text_named(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_names *names,
                                    const dnagpu_text_out_options *opt, dnagpu_text_image **out);
int      dnagpu_names_geometry(uint64_t *chunk_bytes, uint64_t *tile_bytes, uint64_t *group_tiles);
/* Same over an arbitrary array of n keys of k bases already in device memory.  dev_keys is used as
 * scratch and its contents are unspecified afterwards. */
int dnagpu_count_keys(dnagpu_ctx *ctx, uint64_t *dev_keys, uint64_t n, int k, dnagpu_hist **out);
/* Same, when the caller knows that every key lies in [key_min, key_max] (an owner's key range after
 * the multi-GPU exchange): the bits the two bounds share are not partitioned on again.  Any range with
 * key_min <= key_max is valid, aligned to a power of two or not; key_min == key_max is the one-key range (every
 * key equals it: one group of n rows).  Bits of the two bounds above the 2k key bits are ignored.  A wider range
 * than the keys need gives the same histogram.  key_min > key_max: DNAGPU_ERR_BAD_ARG; a key outside the range
 * breaks the promise and the result is then unspecified. */
int dnagpu_count_keys_in_range(dnagpu_ctx *ctx, uint64_t *dev_keys, uint64_t n, int k,
                               uint64_t key_min, uint64_t key_max, dnagpu_hist **out);

uint64_t dnagpu_hist_distinct(const dnagpu_hist *h);   /* count(*) over groups                   */
uint64_t dnagpu_hist_total(const dnagpu_hist *h);      /* sum(count)                              */
/* The groups in device memory, in the order they were produced (NOT ascending: see dnagpu_hist_download /
 * dnagpu_hist_sorted_view for that).  An ordered histogram stores its dnagpu_hist_distinct groups back to back.  An
 * unordered one (dnagpu_hist_is_sorted == 0) stores them bucket by bucket over dnagpu_hist_extent slots, and a
 * bucket that held copies of a k-mer is followed by padding slots whose COUNT IS 0 (their keys are undefined): skip
 * them. */
const uint64_t *dnagpu_hist_device_keys(const dnagpu_hist *h);
uint64_t dnagpu_hist_extent(const dnagpu_hist *h);     /* slots of the two device arrays in use (>= distinct) */
/* counts are 32-bit in device memory (one call covers at most 2^32 - 1 rows); dnagpu_hist_download
 * widens them to the 64-bit count(*) of SQL */
const uint32_t *dnagpu_hist_device_counts(const dnagpu_hist *h);
/* A histogram may consist of several PARTS, each with device arrays of its own (the pipelined multi-GPU count makes
 * them: one per bucket group of an owner).  dnagpu_hist_parts is 1 for every other histogram.  For a histogram of
 * several parts dnagpu_hist_device_keys / _counts are NULL -- walk the parts instead (dnagpu_hist_part(h, i): a
 * borrowed view, freed with h); distinct / total / extent / summary / download / sorted_view cover all parts, the
 * groups of part i before those of part i + 1. */
uint32_t dnagpu_hist_parts(const dnagpu_hist *h);
const dnagpu_hist *dnagpu_hist_part(const dnagpu_hist *h, uint32_t i);
/* Copies groups [first, first+count) of the ASCENDING-KEY order to host arrays (either may be
 * NULL). */
int dnagpu_hist_download(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t first, uint64_t count,
                         uint64_t *keys, uint64_t *counts);
/* Same view into device memory: groups [first, first+count) of the ascending-key order as two dense
 * arrays of `count` uint64 each (either may be NULL), e.g. for a caller that post-processes on the GPU. */
int dnagpu_hist_sorted_view(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t first, uint64_t count,
                            uint64_t *dev_keys, uint64_t *dev_counts);
/* total = sum(count), unique = count(*) FILTER (WHERE count = 1) (test.sql:112-114), checksum =
 * wrapping sum over groups of an order-independent digest of (key, count), computed on device. */
int dnagpu_hist_summary(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t *total, uint64_t *unique,
                        uint64_t *checksum);
/* *out = the groups of a and b added up (equal keys: counts summed) -- what a caller that counts a large table batch by
 * batch (dnagpu_count_kmers_batch) does with the batches' histograms; also a PostgreSQL aggregate's combine step.  a and
 * b stay as they are; all three live on ctx's device.  The result is an unordered histogram of one part (dnagpu_hist_is_sorted
 * == 0; here the groups are in no order at all, also inside its one segment).  DNAGPU_ERR_TOO_LARGE when the totals pass
 * 2^32 - 1 (counts are 32-bit in device memory).  DNAGPU_ERR_BAD_ARG, and no histogram, when a and b were counted with
 * different k: every histogram of dnagpu_count_kmers, _unordered, _batch, _table, _owned, dnagpu_count_keys and
 * _keys_in_range records its k (a merge result takes its inputs'); one that records none (the multi-GPU counts) merges with
 * any.  A utility (one random probe of a device-memory table per group), not part of the streaming path. */
int dnagpu_hist_merge(dnagpu_ctx *ctx, const dnagpu_hist *a, const dnagpu_hist *b, dnagpu_hist **out);
void dnagpu_hist_free(dnagpu_ctx *ctx, dnagpu_hist *h);

/* ---- k-mer accumulator: GROUP BY over a table of any size, batch by batch (the HashAggregate of test.sql:140-150 with
 * its int8 counts) ---------------------------------------------------------------------------------------------------
 * An accumulator stays in device memory and adds histograms into 64-bit counts; no total limit.  It belongs to one context
 * and its buffers come from that context's pool (the stream rule above).
 * dnagpu_acc_create: DNAGPU_ERR_INVALID_K unless 1 <= k <= 32; an empty accumulator holds no device memory yet.
 * dnagpu_acc_add adds the groups of h (equal keys: counts summed, 64-bit).  Any histogram: ordered or unordered, one part or
 *   several, from every count entry point and dnagpu_hist_merge; count-0 padding slots are skipped and the all-ones key
 *   (32 G's) counts like any other.  h is left as it is and may be freed right after the call; adding the same histogram
 *   twice doubles every count.  DNAGPU_ERR_BAD_ARG when h records a k other than the accumulator's (a histogram that
 *   records none -- the multi-GPU counts -- is accepted: dnagpu_hist_merge's rule).  Every error (bad k, OOM while the
 *   table grows, a HIP error before the merge) leaves the accumulator as it was: a larger table is built in new buffers and
 *   takes over only when the add succeeds.  Cost: one streaming pass over the histogram and the partitions it touches,
 *   not a random probe per group (DESIGN.md "accumulator").
 * dnagpu_acc_distinct = count(*) over groups, dnagpu_acc_total = sum(count) (0 for NULL).
 * dnagpu_acc_summary: total, unique = groups with count 1, checksum = wrapping sum of the (key, count) digest of
 *   dnagpu_hist_summary over 64-bit counts -- an accumulator holding one histogram reports exactly that histogram's summary.
 * dnagpu_acc_download: groups [first, first+count) into host arrays (either may be NULL).  The order is unspecified, as
 *   GROUP BY's, but fixed until the next add: the windows of one pass tile the groups exactly once. */
typedef struct dnagpu_acc dnagpu_acc;
int dnagpu_acc_create(dnagpu_ctx *ctx, int k, dnagpu_acc **out);
int dnagpu_acc_add(dnagpu_ctx *ctx, dnagpu_acc *acc, const dnagpu_hist *h);
/* The strand-neutral add: every group of h is added under the CANONICAL form of its key (dnagpu_kmer_strand below, k = the
 * accumulator's), so a k-mer and its reverse complement are one group: its count is count(x) + count(rc(x)), or count(x)
 * alone when x is its own reverse complement (even k only; such a key is not doubled).  Every rule of dnagpu_acc_add holds:
 * any histogram, padding slots skipped, a histogram that records no k accepted, and every error leaves the accumulator as
 * it was.  total grows by the histogram's total; distinct grows by the canonical keys that are new.  The all-ones key (32
 * G's) folds into 0xAAAA... (32 C's); key 0 (32 A's) stays, and 32 T's fold into it.  The accumulator holds canonical groups
 * only if EVERY add into it is this one; the library does not track that -- a plain dnagpu_acc_add of a key that is not
 * canonical simply makes a group of its own.  spectrum, select, top, rank, download and dnagpu_acc_join read such an
 * accumulator like any other, so Jaccard and containment of two canonical sets are strand-neutral.  Cost: the same passes
 * as dnagpu_acc_add. */
int dnagpu_acc_add_canonical(dnagpu_ctx *ctx, dnagpu_acc *acc, const dnagpu_hist *h);
uint64_t dnagpu_acc_distinct(const dnagpu_acc *acc);
uint64_t dnagpu_acc_total(const dnagpu_acc *acc);
int dnagpu_acc_summary(dnagpu_ctx *ctx, const dnagpu_acc *acc, uint64_t *total, uint64_t *unique, uint64_t *checksum);
int dnagpu_acc_download(dnagpu_ctx *ctx, dnagpu_acc *acc, uint64_t first, uint64_t count, uint64_t *keys, uint64_t *counts);
void dnagpu_acc_free(dnagpu_ctx *ctx, dnagpu_acc *acc);

/* ---- hash join of two accumulators: what kmer_hash_ops (dna--1.0.sql:204-212) is for besides GROUP BY -- the plans that
 * pair equal k-mers of two inputs, here over two counted sets that already sit in device memory:
 *   SELECT a.kmer, a.count, b.count FROM counts_a a JOIN counts_b b ON a.kmer = b.kmer     (Hash Join)      DNAGPU_JOIN_INNER
 *   SELECT kmer FROM counts_a INTERSECT SELECT kmer FROM counts_b                          (hashed SetOp)   DNAGPU_JOIN_INNER
 *   SELECT kmer FROM counts_a EXCEPT SELECT kmer FROM counts_b; NOT IN; NOT EXISTS         (hashed SetOp)   DNAGPU_JOIN_ANTI
 *   ... FROM counts_a a LEFT JOIN counts_b b ON a.kmer = b.kmer                                             DNAGPU_JOIN_LEFT
 * The join runs on the device and hands out only the result rows and their statistics.
 * Rows: keys are distinct inside an accumulator, so every kind yields at most one row per group of `left` (SEMI equals
 *   INNER).  Rows come in unspecified order.  At most `cap` rows go to each of out_keys / out_left / out_right; any of them
 *   may be NULL; they are host memory, or device memory when out_on_device != 0.  *n_out = ALL result rows, even beyond cap
 *   (dnagpu_*_select's rule); which cap of them are written is then unspecified.  With cap == 0 or all three arrays NULL
 *   nothing is stored: the statistics-only call.  stats may be NULL; when given it always covers all result rows, never only
 *   those within cap.  All sums are exact 64-bit: sum_left <= dnagpu_acc_total(left).
 * Derived figures: with the two dnagpu_acc_distinct values dL and dR, INNER's rows give Jaccard = rows / (dL + dR - rows) and
 *   the containment rows / dL; with the two dnagpu_acc_total values, sum_min gives the weighted forms.
 * Sources: both sides are read only -- the tables, the download order and the summaries stay as they were.  left == right is
 *   allowed: INNER then returns every group with equal counts, ANTI nothing.  An empty side holds no table: an empty left
 *   gives 0 rows; an empty right gives INNER 0 rows and ANTI / LEFT every group of left with count_right = 0.  The all-ones
 *   key and key 0 are keys like any other.
 * Checks, in order: a kind outside 0 .. 2 is DNAGPU_ERR_BAD_ARG (the range before the missing object, as elsewhere in this
 *   header); a NULL ctx, left, right or n_out is DNAGPU_ERR_BAD_ARG; accumulators of different k are DNAGPU_ERR_BAD_ARG
 *   (nothing is written); an allocation failure is DNAGPU_ERR_OOM with nothing leaked.
 * Waiting: the call waits for its work, as select does: host and device outputs are complete when it returns.
 * dnagpu_acc_partitions: the partitions of the accumulator's table, a power of two (0 for NULL or an accumulator that holds
 *   no table yet).  The join picks its path from the two sides' partition counts alone.
 * Out of scope: a histogram as a side (dnagpu_acc_create plus one dnagpu_acc_add puts it into an accumulator: the same bin
 *   pass a native form would need); FULL OUTER (LEFT, plus ANTI the other way round); a result that is itself an accumulator;
 *   more than one GPU. */
#define DNAGPU_JOIN_INNER 0   /* rows of left that have a partner in right: key, count_left, count_right (JOIN .. ON a.kmer = b.kmer; INTERSECT) */
#define DNAGPU_JOIN_ANTI  1   /* rows of left that have none: key, count_left, count_right = 0 (EXCEPT; NOT IN; NOT EXISTS)                 */
#define DNAGPU_JOIN_LEFT  2   /* every row of left: count_right = the partner's count, 0 when there is none (LEFT JOIN)                      */
typedef struct dnagpu_join_stats {
    uint64_t rows;            /* result rows of `kind`                                              */
    uint64_t sum_left;        /* sum of count_left over the result rows                             */
    uint64_t sum_right;       /* sum of count_right over the result rows                            */
    uint64_t sum_min;         /* sum of min(count_left, count_right) over the result rows           */
    uint64_t checksum_left;   /* wrapping sum of the (key, count_left) digest of dnagpu_acc_summary */
    uint64_t checksum_right;  /* the same over (key, count_right), rows with count_right > 0 only   */
} dnagpu_join_stats;
int dnagpu_acc_join(dnagpu_ctx *ctx, const dnagpu_acc *left, const dnagpu_acc *right, int kind,
                    uint64_t *out_keys, uint64_t *out_left, uint64_t *out_right, uint64_t cap,
                    uint64_t *n_out, dnagpu_join_stats *stats, int out_on_device);
uint64_t dnagpu_acc_partitions(const dnagpu_acc *acc);

/* ---- per-sequence hits of a table's k-mers in a counted set: the other plan kmer_hash_ops (dna--1.0.sql:204-212) makes
 * possible -- the rows of a table of sequences hash-joined to a counted set and folded BY SEQUENCE:
 *   SELECT d.id, count(*) AS hits
 *   FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS g(kmer) JOIN counts_b b ON g.kmer = b.kmer
 *   WHERE b.count BETWEEN min_count AND max_count GROUP BY d.id           [HAVING count(*) >= m, or hits / rows >= f]
 * (read screening, host depletion, containment of a read in a reference).  It runs on the device and hands
 * back 8 bytes per SEQUENCE, or with a threshold only the sequences that pass.
 * Input: dna is a table made resident with dnagpu_dna_set_sequences; set is any accumulator of the same context; k is the
 *   accumulator's.  Both are only read: the set's summary and download order and the table's sequence set stay as they were.
 * Meaning: for every sequence s of [seq_first, seq_first + seq_count): rows[s] = the rows of its own generate_kmers, len - k + 1,
 *   0 when len < k (the 64-bit restatement of dna.c:781; empty sequences have 0); hits[s] = those rows whose key is a group of
 *   set with min_count <= count <= max_count.  With DNAGPU_HITS_CANONICAL the canonical form of the row's key
 *   (dnagpu_kmer_strand's) is looked up instead: the form for a set made with dnagpu_acc_add_canonical.  min_count == 0 means
 *   1; min_count > max_count matches nothing (DNAGPU_OK).  Key 0 and the all-ones key are keys like any other; a partition
 *   that holds nothing is never read; a set without a table gives hits of 0 and the true rows.
 * Snapshot: a dnagpu_seq_hits owns two dense uint32 device arrays of seq_count entries from the context's pool (the stream
 *   rule above) -- what dnagpu_seq_hits_device_rows / _hits return, entry i belonging to sequence seq_first + i -- and does
 *   not depend on dna or set afterwards.  seq_count == 0 gives a valid object of 0 sequences that holds no device memory
 *   (both accessors NULL).
 * Limit: the window's bases, seq_starts[seq_first + seq_count] - seq_starts[seq_first], may be at most 2^32 - 1, else
 *   DNAGPU_ERR_TOO_LARGE (dnagpu_generate_kmers_table's per-call rule: it is what makes the 32-bit arrays exact); larger tables
 *   are paged by sequence window, and windows tile.  (More than 2^32 - 1 sequences in one window: DNAGPU_ERR_TOO_LARGE too.)
 *   Today dnagpu_dna_set_sequences itself refuses a stream of more than 2^32 - 1 bases, so no resident table reaches either
 *   limit: they are stated, and checked, for the day that rule is lifted.
 * Checks, in order: flags outside 0 .. 1 is DNAGPU_ERR_BAD_ARG (the range before the missing object); a NULL ctx, dna, set or
 *   out is DNAGPU_ERR_BAD_ARG; a non-empty stream without a sequence set is DNAGPU_ERR_BAD_ARG; seq_first > the table's
 *   sequences or seq_count > sequences - seq_first is DNAGPU_ERR_BAD_ARG; the limit above; an allocation failure is
 *   DNAGPU_ERR_OOM with nothing leaked and *out = NULL.  The call waits for its work.
 * dnagpu_seq_hits_sequences / _first / _k: seq_count, seq_first, k; 0 for NULL.
 * dnagpu_seq_hits_totals: the sums of rows and of hits over the window and the sequences with at least one hit, exact 64-bit
 *   sums made on the device when the object is built (any output may be NULL; a NULL h is DNAGPU_ERR_BAD_ARG).
 * dnagpu_seq_hits_read: entries [first, first + count) of the window widened to uint64, to out_rows / out_hits (either may be
 *   NULL; host memory, or device memory when out_on_device != 0), by dnagpu_ranking_read's window rule: first > sequences or
 *   count > sequences - first is DNAGPU_ERR_BAD_ARG; count == 0 or both outputs NULL is DNAGPU_OK.  Waits for the copy.
 * dnagpu_seq_hits_select: the sequences with min_hits <= hits <= max_hits and hits * frac_den >= frac_num * rows (the HAVING
 *   forms; 0 / 1 asks nothing of the fraction).  frac_den == 0, or frac_num or frac_den above 2^32 - 1 (the products must stay
 *   exact in 64 bits), is DNAGPU_ERR_BAD_ARG and is checked first; then a NULL ctx, h or n_out.  Rows come in ASCENDING
 *   SEQUENCE ID: out_seq holds global ids, seq_first + i; at most cap rows go to each of out_seq / out_rows / out_hits (any
 *   may be NULL); *n_out = ALL matches, and when it exceeds cap the FIRST cap of that order are written -- deterministic,
 *   unlike the count selects, because a caller pages on it.  min_hits = 0, max_hits = 0 is the depletion query: the
 *   sequences with no hit.  Waits for its work.
 * dnagpu_seq_hits_free returns the arrays to ctx's pool (NULL h: nothing).
 * Out of scope: a weight per sequence (the sum of the set's counts over the hits); a histogram as the set (make an
 *   accumulator and add it once); more than one GPU. */
typedef struct dnagpu_seq_hits dnagpu_seq_hits;
#define DNAGPU_HITS_CANONICAL 1u   /* probe with the canonical form of the row's key (dnagpu_kmer_strand's) */
int dnagpu_table_hits(dnagpu_ctx *ctx, const dnagpu_dna *dna, const dnagpu_acc *set, unsigned flags,
                      uint64_t min_count, uint64_t max_count, uint64_t seq_first, uint64_t seq_count, dnagpu_seq_hits **out);
uint64_t dnagpu_seq_hits_sequences(const dnagpu_seq_hits *h);
uint64_t dnagpu_seq_hits_first(const dnagpu_seq_hits *h);
int      dnagpu_seq_hits_k(const dnagpu_seq_hits *h);
int dnagpu_seq_hits_totals(const dnagpu_seq_hits *h, uint64_t *rows, uint64_t *hits, uint64_t *seqs_hit);
const uint32_t *dnagpu_seq_hits_device_rows(const dnagpu_seq_hits *h);
const uint32_t *dnagpu_seq_hits_device_hits(const dnagpu_seq_hits *h);
int dnagpu_seq_hits_read(dnagpu_ctx *ctx, const dnagpu_seq_hits *h, uint64_t first, uint64_t count,
                         uint64_t *out_rows, uint64_t *out_hits, int out_on_device);
int dnagpu_seq_hits_select(dnagpu_ctx *ctx, const dnagpu_seq_hits *h, uint64_t min_hits, uint64_t max_hits,
                           uint64_t frac_num, uint64_t frac_den, uint64_t *out_seq, uint64_t *out_rows, uint64_t *out_hits,
                           uint64_t cap, uint64_t *n_out, int out_on_device);
void dnagpu_seq_hits_free(dnagpu_ctx *ctx, dnagpu_seq_hits *h);

/* ---- the k-mer profile of every sequence of a table: test.sql:140-150 with d.id added to the GROUP BY,
 *   SELECT d.id, k.kmer, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer)
 *   GROUP BY d.id, k.kmer
 * -- the tetranucleotide profile of a contig, the hexamer table of a gene, GC content at k = 1 -- as a dense matrix of
 * W = 4^k columns per sequence, for k <= DNAGPU_PROFILE_MAX_K.
 * dnagpu_profile_width(k) = 4^k for k in 1 .. 6, otherwise 0; it needs no device.
 * dnagpu_table_profile
 *   Input: a table made resident with dnagpu_dna_set_sequences, or one dnagpu_dna_take / dnagpu_dna_gather produced; a
 *   non-empty stream without a set is DNAGPU_ERR_BAD_ARG (dnagpu_count_kmers_table's rule).  The table, its set and the
 *   stream are only read; no word at or beyond the stream's words is read and the result never depends on bits behind the
 *   last base (dnagpu_dna_wrap's rule).
 *   Window: sequences [seq_first, seq_first + seq_count) under dnagpu_dna_sequence_starts' rule applied to the table's
 *   sequences: seq_first > sequences or seq_count > sequences - seq_first is DNAGPU_ERR_BAD_ARG; seq_count == 0 is DNAGPU_OK
 *   and writes nothing; seq_count > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE.  Callers page by window, and windows tile.
 *   Output: out_counts[(s - seq_first) * W + key] = the rows of sequence s's own generate_kmers(., k) whose key is `key`
 *   (the library's key format: base i at bits 2i .. 2i + 1, A = 0 T = 1 C = 2 G = 3, so the column order is the `keys` order
 *   of every other entry point); out_rows[s - seq_first] = len >= k ? len - k + 1 : 0, and may be NULL.  Every cell of
 *   the window's matrix is written, zeros included -- the caller does not clear it -- and nothing outside it is touched.
 *   Counts are 32-bit: a resident table holds at most 2^32 - 1 bases.  Outputs are host memory, or device memory when
 *   out_on_device != 0 (out_counts 4-byte aligned, out_rows 8-byte aligned).  The host form stages in pool memory; a
 *   staging buffer that cannot be had is DNAGPU_ERR_OOM.  The call waits for its work.
 *   DNAGPU_PROFILE_CANONICAL: every row is counted under its canonical form (dnagpu_kmer_strand's, A < T < C < G); columns
 *   that are not canonical are 0, and a k-mer that is its own reverse complement counts once per row:
 *   canon[c] = fwd[c] + fwd[rc(c)] when c != rc(c), fwd[c] when c == rc(c).
 *   Checks, in order: a NULL ctx or dna is DNAGPU_ERR_BAD_ARG; flags other than 0 or 1 is DNAGPU_ERR_BAD_ARG; k < 1 or
 *   k > 32 is DNAGPU_ERR_INVALID_K; k in 7 .. 32 is DNAGPU_ERR_TOO_LARGE (wider than a dense profile offers:
 *   dnagpu_last_error() says so); the window; the missing set; a NULL out_counts with seq_count > 0 is DNAGPU_ERR_BAD_ARG.
 *   On any error no output byte is written.
 * dnagpu_profile_geometry: the two limits of the kernels' sequence classes, in rows -- a sequence of at most *wave_rows
 *   rows is counted by one wave, a longer one in items of *tile_rows rows (either pointer may be NULL; needs no device).
 *   For tests and measurements.
 * Out of scope: k > 6 (a sparse, sorted (id, kmer, count) result); frequencies or distances; more than one GPU. */
#define DNAGPU_PROFILE_CANONICAL 1u
#define DNAGPU_PROFILE_MAX_K     6
uint64_t dnagpu_profile_width(int k);
int dnagpu_table_profile(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, unsigned flags,
                         uint64_t seq_first, uint64_t seq_count,
                         uint32_t *out_counts, uint64_t *out_rows, int out_on_device);
int dnagpu_profile_geometry(uint64_t *wave_rows, uint64_t *tile_rows);

/* ---- equal sequences: dna = dna, DISTINCT, the join on sequence (equals / dna_ne, dna.c:334-384; the operators =, <> and
 * ~= of dna--1.0.sql:58-86; test.sql:1-20).  The type has no hash or btree operator class, so the reference answers
 *   SELECT min(id), count(*) FROM t GROUP BY sequence        WHERE sequence = $1        a JOIN b ON a.sequence = b.sequence
 * as nested loops over dna_eq_internal; here they run on the device over resident tables.
 * Equality: two sequences are equal when they have the same number of bases and every base is equal -- dna.c:334-350 for
 *   well-formed values.  The result never depends on bits behind a last base (dnagpu_dna_wrap's rule; the reference compares
 *   whole words and relies on zero tails).  Two empty sequences are equal.  Length is part of the identity: A is code 00, so
 *   ACG, ACGA and ACGAA have the same words and are three different sequences.
 * dnagpu_dna_equals: the whole values a and b (sequence sets are ignored); *equal = 1 or 0.  Different lengths answer 0 with
 *   no device work; a == b (the same object) is 1.  A NULL ctx, a, b or equal is DNAGPU_ERR_BAD_ARG.  No word at or beyond
 *   either side's n_words is read.  Waits for its work.
 * dnagpu_table_classes: partitions the sequences of a resident table (from dnagpu_dna_set_sequences, or a result of
 *   dnagpu_dna_take / _gather) into classes of equal sequences: rep[s] = the smallest id of s's class (rep[rep[s]] == rep[s] <=
 *   s), copies[s] = the size of s's class, dnagpu_seq_classes_distinct = the number of classes.  Exact for every input: a
 *   64-bit content fingerprint only proposes candidates, the bases decide.  The object owns its device arrays, which come
 *   from the context's pool (the stream rule above), and it BORROWS the table -- the second exception beside dnagpu_dna_wrap
 *   to "the library never keeps a caller pointer": the caller keeps the dnagpu_dna alive, with its sequence set unchanged,
 *   until dnagpu_seq_classes_free, because dnagpu_table_match verifies against the table's bases.  A table of 0 sequences
 *   gives a valid object that holds no device memory (distinct 0, rounds 0).
 *   Checks, in order: a NULL ctx, table or out is DNAGPU_ERR_BAD_ARG; a non-empty stream without a sequence set is
 *   DNAGPU_ERR_BAD_ARG (dnagpu_count_kmers_table's rule); more than 2^32 - 1 sequences is DNAGPU_ERR_TOO_LARGE; an allocation
 *   failure is DNAGPU_ERR_OOM with nothing leaked and *out left as it was.  Waits for its work.
 * dnagpu_seq_classes_sequences / _distinct / _rounds: 0 for NULL.  _rounds = the verify rounds the build ran: 0 for an empty
 *   table, 1 whenever no two different sequences shared a fingerprint (for tests and probes).
 * dnagpu_seq_classes_read: entries [first, first + count) of rep and copies as uint64 (either may be NULL; host memory, or
 *   device memory when out_on_device != 0), by dnagpu_ranking_read's window rule: first > sequences or count > sequences -
 *   first is DNAGPU_ERR_BAD_ARG; count == 0 or both outputs NULL is DNAGPU_OK.  Waits for the copy.
 * dnagpu_seq_classes_select: the representatives (rep[s] == s) with min_copies <= copies <= max_copies, in ASCENDING ID --
 *   GROUP BY sequence with min(id), count(*) and HAVING: 1 .. max is DISTINCT, 2 .. max the duplicated reads, 1 .. 1 the
 *   singletons.  min_copies == 0 means 1; min > max matches nothing (DNAGPU_OK).  *n_out = ALL matches, and when it exceeds
 *   cap the FIRST cap of that order are written (dnagpu_seq_hits_select's rule: a caller pages on it and feeds out_seq to
 *   dnagpu_dna_take).  Either array may be NULL.  A NULL ctx, c or n_out is DNAGPU_ERR_BAD_ARG.  Waits for its work.
 * dnagpu_seq_classes_members: the ids of every sequence equal to sequence seq, seq included, ascending -- SELECT id FROM t
 *   WHERE sequence = (that one) -- under the same cap rule; seq >= sequences is DNAGPU_ERR_BAD_ARG.
 * dnagpu_table_match: the join of a probe table to a built one,
 *     SELECT a.id, min(b.id), count(*) FROM a JOIN b ON a.sequence = b.sequence GROUP BY a.id
 *   with a row for every a.id: for every sequence s of [seq_first, seq_first + seq_count) of probe, out_match[s - seq_first] =
 *   the smallest id in the built table of a sequence equal to it, or DNAGPU_MATCH_NONE, and out_copies[s - seq_first] = that
 *   class's size, or 0; *n_matched (may be NULL) = the probe sequences with a match.  A probe of one sequence is WHERE
 *   sequence = $1; probe may be the built table itself (the result is then rep and copies); an empty built table matches
 *   nothing.  The window follows dnagpu_table_profile's rule and windows tile; every cell of the window is written, nothing
 *   outside it, and on any error no output byte is written.  Outputs are host memory, or device memory when out_on_device
 *   != 0.  Checks, in order: a NULL ctx, build or probe is DNAGPU_ERR_BAD_ARG; the window (a window that leaves the probe's
 *   sequences is DNAGPU_ERR_BAD_ARG, then seq_count > 2^32 - 1 is DNAGPU_ERR_TOO_LARGE); a probe stream without a set;
 *   both outputs and n_matched NULL with seq_count > 0 is DNAGPU_ERR_BAD_ARG.  Waits for its work.
 * dnagpu_seq_equal_geometry: the limits of the kernels' two sequence classes, in bases -- a sequence of at most *wave_bases
 *   bases is fingerprinted and compared whole by a part of one wave, a longer one in items of *tile_bases bases (either
 *   pointer may be NULL; needs no device).  For tests and measurements.
 * Out of scope: strand-neutral equality (a read equal to its reverse complement); prefix, containment or approximate
 *   matches; an order on dna; updating a classes object after the table changes; more than one GPU; tables past one resident
 *   stream of 2^32 - 1 bases. */
typedef struct dnagpu_seq_classes dnagpu_seq_classes;
#define DNAGPU_MATCH_NONE UINT64_MAX
int dnagpu_dna_equals(dnagpu_ctx *ctx, const dnagpu_dna *a, const dnagpu_dna *b, int *equal);
int dnagpu_table_classes(dnagpu_ctx *ctx, const dnagpu_dna *table, dnagpu_seq_classes **out);
uint64_t dnagpu_seq_classes_sequences(const dnagpu_seq_classes *c);
uint64_t dnagpu_seq_classes_distinct(const dnagpu_seq_classes *c);
uint32_t dnagpu_seq_classes_rounds(const dnagpu_seq_classes *c);
int dnagpu_seq_classes_read(dnagpu_ctx *ctx, const dnagpu_seq_classes *c, uint64_t first, uint64_t count,
                            uint64_t *out_rep, uint64_t *out_copies, int out_on_device);
int dnagpu_seq_classes_select(dnagpu_ctx *ctx, const dnagpu_seq_classes *c, uint64_t min_copies, uint64_t max_copies,
                              uint64_t *out_seq, uint64_t *out_copies, uint64_t cap, uint64_t *n_out, int out_on_device);
int dnagpu_seq_classes_members(dnagpu_ctx *ctx, const dnagpu_seq_classes *c, uint64_t seq,
                               uint64_t *out_seq, uint64_t cap, uint64_t *n_out, int out_on_device);
int dnagpu_table_match(dnagpu_ctx *ctx, const dnagpu_seq_classes *build, const dnagpu_dna *probe,
                       uint64_t seq_first, uint64_t seq_count,
                       uint64_t *out_match, uint64_t *out_copies, uint64_t *n_matched, int out_on_device);
void dnagpu_seq_classes_free(dnagpu_ctx *ctx, dnagpu_seq_classes *c);
int dnagpu_seq_equal_geometry(uint64_t *wave_bases, uint64_t *tile_bases);

/* ---- count-ordered queries over counted groups: the reference's first counting statement is not a bare GROUP BY but
 *   SELECT k.kmer, count(*) FROM generate_kmers(...) AS k(kmer) GROUP BY k.kmer ORDER BY count(*) DESC   (test.sql:95)
 * and its second summarises the distribution of the counts (count(*) FILTER (WHERE count = 1), test.sql:112-114) -----------
 * Three read-only queries, each over a histogram (dnagpu_hist_*) and over an accumulator (dnagpu_acc_*: a table past 2^32
 * rows only ever exists as one).  They run on the device and hand out only the answer, not every group.
 * Every histogram is accepted, under dnagpu_acc_add's rule: ordered or unordered, one part or several, results of
 * dnagpu_hist_merge, borrowed dnagpu_hist_part views.  Count-0 padding slots, empty accumulator slots and unoccupied
 * partitions are never a group; the all-ones key is a key like any other.  The object is left as it is (the accumulator's
 * download order too).  A NULL ctx, object, bins or n_out is DNAGPU_ERR_BAD_ARG; the range of n_bins / n is checked first
 * (dnagpu_acc_create's order).
 *
 * spectrum: the k-mer spectrum.  bins[c - 1] = the groups with count == c for 1 <= c < n_bins, bins[n_bins - 1] = the groups
 *   with count >= n_bins (bins: n_bins words of host memory).  sum(bins) = distinct; with n_bins >= 2, bins[0] is the
 *   `unique` of dnagpu_hist_summary; n_bins == 1 gives [distinct].  n_bins outside 1 .. DNAGPU_SPECTRUM_MAX_BINS:
 *   DNAGPU_ERR_BAD_ARG.
 * select: GROUP BY kmer HAVING count(*) BETWEEN min_count AND max_count.  The groups with min_count <= count <= max_count, in
 *   unspecified order, counts as uint64 (dnagpu_hist_download's widening), at most `cap` rows to each of out_keys /
 *   out_counts (either may be NULL; host memory, or device memory when out_on_device != 0).  *n_out = ALL matching groups
 *   even when that exceeds cap (dnagpu_generate_kmers_filtered's rule); which cap of them are written is then unspecified.
 *   min_count > max_count matches nothing (DNAGPU_OK); min_count == 0 means 1.
 * top: GROUP BY kmer ORDER BY count(*) DESC LIMIT n.  *n_out = min(n, distinct) rows sorted by count descending, keys
 *   ascending (as uint64) among rows of equal count.  With T the count of the last row, every group with count > T is
 *   returned; which groups of count == T fill the remaining places is unspecified (PostgreSQL's LIMIT over ties promises no
 *   more).  n >= distinct (with distinct <= DNAGPU_TOP_MAX) is the whole ORDER BY count(*) DESC of test.sql:95.  n == 0 or
 *   an empty object: *n_out = 0, DNAGPU_OK.  n > DNAGPU_TOP_MAX: DNAGPU_ERR_TOO_LARGE. */
#define DNAGPU_SPECTRUM_MAX_BINS (1u << 20)
#define DNAGPU_TOP_MAX           (1u << 20)
int dnagpu_hist_spectrum(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t n_bins, uint64_t *bins);
int dnagpu_acc_spectrum(dnagpu_ctx *ctx, const dnagpu_acc *acc, uint64_t n_bins, uint64_t *bins);
int dnagpu_hist_select(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t min_count, uint64_t max_count,
                       uint64_t *out_keys, uint64_t *out_counts, uint64_t cap, uint64_t *n_out, int out_on_device);
int dnagpu_acc_select(dnagpu_ctx *ctx, const dnagpu_acc *acc, uint64_t min_count, uint64_t max_count,
                      uint64_t *out_keys, uint64_t *out_counts, uint64_t cap, uint64_t *n_out, int out_on_device);
int dnagpu_hist_top(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t n,
                    uint64_t *out_keys, uint64_t *out_counts, uint64_t *n_out, int out_on_device);
int dnagpu_acc_top(dnagpu_ctx *ctx, const dnagpu_acc *acc, uint64_t n,
                   uint64_t *out_keys, uint64_t *out_counts, uint64_t *n_out, int out_on_device);

/* ---- rank: GROUP BY kmer ORDER BY count(*) [DESC] with NO LIMIT -- every group in count order (test.sql:95 as written),
 * for any number of groups: top stops at DNAGPU_TOP_MAX rows, and before this the whole order meant downloading every
 * group and sorting on the host.  The order is made on the device (a counting sort by count class, DESIGN.md 4.10 "Rank").
 * Snapshot: a dnagpu_ranking owns two dense device arrays of `rows` uint64 each (keys, counts; rows = distinct of the
 *   source), taken from the context's pool (the stream rule above).  It does not depend on its source afterwards: the
 *   histogram may be freed, the accumulator may take further adds.  The source is left exactly as it was (its summary, the
 *   accumulator's download order).
 * Row order: counts non-increasing (DNAGPU_ORDER_COUNT_DESC) or non-decreasing (DNAGPU_ORDER_COUNT_ASC: the rarest first).
 *   The order among rows of EQUAL count is unspecified (PostgreSQL promises none) but fixed for the ranking's life, so the
 *   windows of dnagpu_ranking_read tile the rows exactly once.  This is deliberately weaker than top's key-ascending ties: a
 *   key sort of a class that holds 10^8 keys is not what this pass is for.
 * Sources: every source dnagpu_acc_add accepts -- ordered and unordered histograms, histograms of several parts and borrowed
 *   dnagpu_hist_part views, dnagpu_hist_merge results -- and accumulators with their 64-bit counts.  Count-0 padding slots,
 *   empty accumulator slots and partitions that hold nothing are never a row; the all-ones key is a key.
 * An empty source gives a ranking of 0 rows (DNAGPU_OK) whose device arrays are NULL; it holds no device memory.
 * Errors: an `order` other than the two values is DNAGPU_ERR_BAD_ARG and is checked first (range before missing object); a
 *   NULL ctx, source or out is DNAGPU_ERR_BAD_ARG; an allocation failure is DNAGPU_ERR_OOM with nothing leaked and *out = NULL.
 * dnagpu_ranking_rows / _order: 0 for NULL.  dnagpu_ranking_device_keys / _counts: the rows dense, in rank order; counts are
 *   uint64 (dnagpu_hist_download's widening).
 * dnagpu_ranking_read: rows [first, first + count) to out_keys / out_counts (either may be NULL; host memory, or device
 *   memory when out_on_device != 0), by dnagpu_hist_download's window rule: first > rows or count > rows - first is
 *   DNAGPU_ERR_BAD_ARG; count == 0 or both outputs NULL is DNAGPU_OK; a NULL ctx or r is DNAGPU_ERR_BAD_ARG.  Waits for the copy.
 * dnagpu_ranking_free returns the arrays to ctx's pool (NULL r: nothing). */
typedef struct dnagpu_ranking dnagpu_ranking;
#define DNAGPU_ORDER_COUNT_DESC 0   /* ORDER BY count(*) DESC  (test.sql:95) */
#define DNAGPU_ORDER_COUNT_ASC  1   /* ORDER BY count(*)       (rarest first) */
int dnagpu_hist_rank(dnagpu_ctx *ctx, const dnagpu_hist *h, int order, dnagpu_ranking **out);
int dnagpu_acc_rank(dnagpu_ctx *ctx, const dnagpu_acc *acc, int order, dnagpu_ranking **out);
uint64_t dnagpu_ranking_rows(const dnagpu_ranking *r);
int dnagpu_ranking_order(const dnagpu_ranking *r);
const uint64_t *dnagpu_ranking_device_keys(const dnagpu_ranking *r);
const uint64_t *dnagpu_ranking_device_counts(const dnagpu_ranking *r);
int dnagpu_ranking_read(dnagpu_ctx *ctx, const dnagpu_ranking *r, uint64_t first, uint64_t count,
                        uint64_t *out_keys, uint64_t *out_counts, int out_on_device);
void dnagpu_ranking_free(dnagpu_ctx *ctx, dnagpu_ranking *r);

/* ---- multi-GPU sharding of the count (one process per GPU; the exchange itself is the
 * caller's collective, e.g. RCCL all-to-all) -------------------------------------------------
 * Step 1 on every rank: the keys of rows [first, first+count) partitioned by owner.  Owner o of
 * n_owners owns the keys whose top `owner_bits` bits d satisfy (d * n_owners) >> owner_bits == o
 * (contiguous, ascending key ranges).  *dev_keys receives a device buffer of `count` keys grouped
 * by owner, owner_offsets[0..n_owners] the group boundaries.  Free with dnagpu_buffer_free.
 * 1 <= n_owners <= 1024, else DNAGPU_ERR_BAD_ARG.  k <= 5 is DNAGPU_ERR_BAD_ARG too (the whole key is the owner
 * digit: such counts run on one GPU); the call is refused before any device work and *dev_keys is NULL.
 * Step 2 (caller): exchange the groups.  Step 3: dnagpu_count_keys on what was received; the
 * concatenation of the owners' downloads in owner order is the global result, keys ascending. */
/* Alternative without moving keys (the default of sharded.py): every rank holds the whole packed
 * sequence (an all-gather of 2 bits per base instead of an all-to-all of 64 bits per k-mer), scans
 * all of it and keeps only the keys it owns (same owner rule as above).  The histogram covers
 * exactly this owner's key range; dnagpu_hist_total() is the number of rows it owns. */
int dnagpu_count_kmers_owned(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, uint64_t first,
                             uint64_t count, int owner, int n_owners, dnagpu_hist **out);
int dnagpu_partition_kmers(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k,
                           uint64_t first, uint64_t count, int n_owners,
                           uint64_t **dev_keys, uint64_t *owner_offsets);
/* Device buffers from the context's pool.  Stream rule for every pooled buffer a caller touches with its
 * own HIP work (these, *dev_keys of dnagpu_partition_kmers, the arrays of a dnagpu_hist): the pool recycles a
 * block as soon as it is freed and orders reuse only on dnagpu_stream().  So (1) work a caller queues on
 * another stream must be ordered behind dnagpu_stream() before it first touches a buffer, and (2) must have
 * finished (or dnagpu_stream() must wait for it) before dnagpu_buffer_free / dnagpu_hist_free. */
int dnagpu_buffer_alloc(dnagpu_ctx *ctx, uint64_t bytes, void **dev_ptr);
void dnagpu_buffer_free(dnagpu_ctx *ctx, void *dev_ptr);
/* Copies between host memory and a device buffer on the context's stream and waits for the copy
 * (what the glue does with device-resident results before it builds Datums from them). */
int dnagpu_buffer_download(dnagpu_ctx *ctx, const void *dev_ptr, uint64_t bytes, void *host);
int dnagpu_buffer_upload(dnagpu_ctx *ctx, void *dev_ptr, const void *host, uint64_t bytes);

/* ---- the unordered count in two halves, for rows that live on several GPUs (the real exchange step
 * of the sharded path; dna-sequences-pg-extension_amd/sharded.py: count_sharded_exchange_records) -------------------
 * The super-k-mer engine (dnagpu_count_kmers_unordered) cuts the rows into 16-byte RECORDS -- runs of consecutive
 * k-mers that share their minimizer, ~9 k-mers each at k = 31 -- and sends every record to a coarse bucket that
 * depends on the k-mers' content alone.  A rank therefore cuts only its OWN rows (dnagpu_sk_records), ships every
 * bucket to its owner (1.8 bytes per k-mer instead of 8; the caller's all-to-all), and counts what it receives
 * (dnagpu_count_records): equal k-mers meet because they share the bucket.  global_rows = the rows of the whole
 * count: every rank must pass the same value (it fixes the bucket geometry, and the digits are part of the
 * records).  k in [20, 32] (minimizers of 15 bases for k >= 23, of 13 for k = 21 and 22, of 12 for k = 20). */
typedef struct dnagpu_records dnagpu_records;
/* number of coarse buckets of a count of global_rows rows (0: arguments out of range) */
int dnagpu_sk_buckets(const dnagpu_ctx *ctx, uint64_t global_rows, int k);
/* records of rows [first, first+count) of generate_kmers(dna, k), grouped by bucket in device memory */
int dnagpu_sk_records(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, uint64_t first, uint64_t count,
                      uint64_t global_rows, dnagpu_records **out);
uint32_t dnagpu_records_buckets(const dnagpu_records *r);
/* offsets[b] .. offsets[b+1] = bucket b's records (dnagpu_records_buckets(r) + 1 entries, host memory) */
int dnagpu_records_offsets(const dnagpu_records *r, uint64_t *offsets);
void *dnagpu_records_device(const dnagpu_records *r);      /* 16 bytes per record; pooled (stream rule above) */
void dnagpu_records_free(dnagpu_ctx *ctx, dnagpu_records *r);
/* GROUP BY kmer, count(*) over the k-mers of the given records: pieces[i] = piece_len[i] records of bucket
 * piece_bucket[i] in device memory (any order, several pieces per bucket allowed: one per sending rank); every
 * record of a bucket that exists anywhere must be among them, or equal k-mers are counted apart.  The histogram is
 * unordered (dnagpu_hist_is_sorted == 0); dnagpu_hist_total = the k-mers the records held.  The pieces are copied
 * before the call returns. */
int dnagpu_count_records(dnagpu_ctx *ctx, const void *const *pieces, const uint64_t *piece_len,
                         const uint32_t *piece_bucket, uint32_t n_pieces, int k, uint64_t global_rows,
                         dnagpu_hist **out);

/* ---- multi-GPU count from one process (the call a PostgreSQL backend's glue makes; SURVEY.md 8(b)
 * dnagpu_count_multi) ----------------------------------------------------------------------------------
 * A dnagpu_multi holds one context per rank (rank r on HIP device devices[r]; devices == NULL means 0..n-1;
 * the same device may appear more than once, which is how the path is rehearsed on a one-GPU box) and the
 * exchange transport: DNAGPU_MULTI_RCCL = ncclCommInitAll + ncclAllGather over xGMI (librccl.so is loaded on
 * demand; needs distinct devices), DNAGPU_MULTI_COPY = peer copies, DNAGPU_MULTI_AUTO = RCCL when n_gpus > 1
 * distinct devices and the library loads, else copies. */
typedef struct dnagpu_multi dnagpu_multi;
#define DNAGPU_MULTI_AUTO 0
#define DNAGPU_MULTI_RCCL 1
#define DNAGPU_MULTI_COPY 2
int dnagpu_multi_init(const int *devices, int n_gpus, int transport, dnagpu_multi **out);
void dnagpu_multi_destroy(dnagpu_multi *m);
int dnagpu_multi_size(const dnagpu_multi *m);
dnagpu_ctx *dnagpu_multi_ctx(dnagpu_multi *m, int rank);
/* "rccl" when the communicator exists (ncclCommInitAll succeeded: the ordered paths' all-gather / reduce use it, and the
 * record exchange can, see DNAGPU_MULTI_OPT_EXCHANGE_RCCL), else "copy".  This says what is AVAILABLE; what a count actually
 * moved its data with is dnagpu_multi_exchange_transport. */
const char *dnagpu_multi_transport(const dnagpu_multi *m);
/* How the most recent dnagpu_count_multi / dnagpu_count_multi_unordered call on m moved data between ranks: "peer-copy"
 * (hipMemcpyPeerAsync pulls; plain device copies when ranks share a device), "rccl-sendrecv" (the record exchange through
 * ncclSend / ncclRecv), "rccl-allgather" / "rccl-reduce" (the ordered paths), "none" (one rank, or no call yet). */
const char *dnagpu_multi_exchange_transport(const dnagpu_multi *m);
/* ranks of the RCCL communicator (0 when there is none) */
int dnagpu_multi_rccl_ranks(const dnagpu_multi *m);

/* The packed sequence sharded by contiguous word chunk: rank r is resident with words
 * [r*per, (r+1)*per), per = ceil(ceil(n_bases/32) / n).  upload: from the host words of dna->bit_sequence
 * (dna.c:45-46); synth: every rank generates its own chunk (dnagpu_dna_synth's sequence). */
typedef struct dnagpu_multi_dna dnagpu_multi_dna;
int dnagpu_multi_dna_upload(dnagpu_multi *m, const uint64_t *words, uint64_t n_bases, dnagpu_multi_dna **out);
int dnagpu_multi_dna_synth(dnagpu_multi *m, uint64_t seed, uint64_t n_bases, uint64_t motif_len,
                           dnagpu_multi_dna **out);
uint64_t dnagpu_multi_dna_length(const dnagpu_multi_dna *d);
void dnagpu_multi_dna_free(dnagpu_multi *m, dnagpu_multi_dna *d);

/* GROUP BY kmer, count(*) over rows [first, first+count) of generate_kmers(dna, k) on all ranks: one
 * all-gather of the packed chunks (2 bits per base), then rank r counts the keys it owns (owner rule of
 * dnagpu_count_kmers_owned) in its own host thread.  hists[r] (n entries, caller's array) = rank r's
 * histogram, living on rank r's device; the ranks' ascending downloads concatenated in rank order are the
 * global result in ascending key order, sum of dnagpu_hist_total = count.  Free each with
 * dnagpu_hist_free(dnagpu_multi_ctx(m, r), hists[r]).
 * Short k-mers (k <= 9 with enough rows, the single-GPU table path's rule) gather nothing: rank r counts the rows
 * that start in its own chunk into a table of 4^k counters (one word of halo from its neighbour), the tables
 * are summed onto rank 0 (ncclReduce, or peer copies + adds) and compacted there: hists[0] then holds the whole
 * result, the other ranks' histograms are empty -- the same concatenation property. */
int dnagpu_count_multi(dnagpu_multi *m, const dnagpu_multi_dna *dna, int k, uint64_t first, uint64_t count,
                       dnagpu_hist **hists);
/* The same groups with no order promise (PostgreSQL's GROUP BY makes none, test.sql:95-104), for long k-mers (k >= 20;
 * shorter ones go through dnagpu_count_multi): the record exchange above from one process.  Nothing is gathered:
 * rank r cuts the super-k-mer records of the rows that start in its own chunk, the owner of a coarse bucket pulls the
 * bucket's pieces from every rank (peer copies of 16-byte records, 1.8 B per k-mer at k = 31) and counts them.
 * The exchange is pipelined with the count: an owner's buckets travel in DNAGPU_MULTI_OPT_PARTS groups on a transfer
 * stream of their own and group g is counted while group g + 1 is still in flight.
 * hists[r] = the groups of rank r's buckets (a histogram of up to that many parts, dnagpu_hist_parts): disjoint between
 * ranks, dnagpu_hist_is_sorted == 0, sum of dnagpu_hist_total = count. */
int dnagpu_count_multi_unordered(dnagpu_multi *m, const dnagpu_multi_dna *dna, int k, uint64_t first, uint64_t count,
                                 dnagpu_hist **hists);

/* Options of a dnagpu_multi (dnagpu_multi_set_option):
 *   DNAGPU_MULTI_OPT_PARTS             bucket groups per owner of dnagpu_count_multi_unordered's pipelined exchange, 1 ..
 *                                      DNAGPU_MULTI_MAX_PARTS (1 = all pieces first, then one count)
 *   DNAGPU_MULTI_OPT_EMULATE_LINK_GBS  rehearsal aid for ranks that share one device: every group of inbound pieces is
 *                                      followed, on the transfer stream, by the time the same bytes would take at this
 *                                      many GB/s (0 = off, the default) -- timing only, results are unaffected
 *   DNAGPU_MULTI_OPT_PROBE_OWNER       TIMING PROBE, RESULTS ARE PARTIAL: only this owner (0 .. n-1) pulls and counts its
 *                                      buckets, the other ranks' histograms stay EMPTY (the sum of dnagpu_hist_total is then
 *                                      smaller than `count`), so that on a shared device the call's times are one owner's
 *                                      own (-1 = off, the default: every owner counts).  Never set it in a caller that uses
 *                                      the groups.
 *   DNAGPU_MULTI_OPT_EXCHANGE_RCCL     how dnagpu_count_multi_unordered moves the records between ranks: 0 (default) = every
 *                                      owner pulls its buckets' pieces with peer copies; 1 = every piece is one ncclSend on its
 *                                      rank's transfer stream and one ncclRecv on its owner's, one group call per bucket group
 *                                      (needs dnagpu_multi_transport() == "rccl", else DNAGPU_ERR_BAD_ARG); 2 = as 1, and a
 *                                      rank's own pieces go through RCCL too (so that one rank alone exercises the path) */
#define DNAGPU_MULTI_OPT_PARTS             1
#define DNAGPU_MULTI_OPT_EMULATE_LINK_GBS  2
#define DNAGPU_MULTI_OPT_PROBE_OWNER       3
#define DNAGPU_MULTI_OPT_EXCHANGE_RCCL     4
#define DNAGPU_MULTI_MAX_PARTS             8
#define DNAGPU_MULTI_DEFAULT_PARTS         3
int dnagpu_multi_set_option(dnagpu_multi *m, int option, double value);

/* Host wall-clock milliseconds of the most recent dnagpu_count_multi_unordered call on m, per phase, the slowest rank of
 * each phase: records_ms = every rank cutting the records of its own rows, exchange_ms = the owners' copies of their
 * buckets' pieces (until the last piece of the slowest owner has landed; the part of it that ran while the owner was
 * already counting earlier buckets is hidden_ms; both from HIP events on the owner's streams), count_ms = the owners'
 * phase as a whole (copies queued, groups counted as they land), total_ms = the whole call.  All 0 before the first call
 * or when the call took another path (short k-mers). */
typedef struct dnagpu_multi_times {
    double records_ms, exchange_ms, hidden_ms, count_ms, total_ms;
    uint64_t bytes_moved;     /* record bytes copied between ranks (pieces that stayed on their rank not counted) */
    int parts;                /* bucket groups per owner of the pipelined exchange */
} dnagpu_multi_times;
int dnagpu_multi_last_times(const dnagpu_multi *m, dnagpu_multi_times *out);

/* ---- batched operators over arrays of keys (bulk scans of stored kmer columns) -------------- */

/* kmer_hash (dna.c:722-735): PostgreSQL hash_any over the 8 bytes of bit_sequence. n keys in,
 * n uint32 out; both host, or both device when on_device != 0. */
int dnagpu_kmer_hash(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, uint32_t *out, int on_device);
/* The strand forms of n keys of k bases.  Codes are the reference's, A=00 T=01 C=10 G=11, so the complement of a base is
 * code ^ 1 and, with rev2 = the 32 two-bit fields of a word in reverse order and mask = the low 2k bits,
 *   rc(key, k) = (rev2(key & mask) >> (64 - 2k)) ^ (0x5555555555555555 & mask).
 * The canonical form of a k-mer is whichever of key and rc(key) comes FIRST IN THIS LIBRARY'S INDEX ORDER: text order under
 * A < T < C < G with base 0 most significant (dnagpu_kmer_index_*).  That is not the conventional A < C < G < T: canonical
 * keys of another tool are a different choice of strand for about half the k-mers, though the groups are the same.
 * key == rc(key) happens only at even k (16 such keys at k = 4, none at k = 5); such a key is canonical.
 * out[i] = rc(keys[i]) (DNAGPU_STRAND_REVCOMP) or canonical(keys[i]) (DNAGPU_STRAND_CANONICAL); flipped[i] (may be NULL) = 1
 * when out[i] != (keys[i] & mask), else 0.  Bits of a key above 2k are masked off (the index build's rule).  out may equal
 * keys.  All arrays host, or all device when on_device != 0.  Checks, in order: a mode other than the two is
 * DNAGPU_ERR_BAD_ARG; k outside 1 .. 32 is DNAGPU_ERR_INVALID_K; a NULL ctx, or NULL keys / out with n > 0, is
 * DNAGPU_ERR_BAD_ARG; n == 0 is DNAGPU_OK. */
#define DNAGPU_STRAND_REVCOMP   0
#define DNAGPU_STRAND_CANONICAL 1
int dnagpu_kmer_strand(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, int k, int mode,
                       uint64_t *out, uint8_t *flipped, int on_device);
/* flags[i] = 1 when keys[i] (a kmer of k bases) satisfies `filter`, else 0.  Same error rules as
 * dnagpu_generate_kmers_filtered. */
int dnagpu_kmer_match(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, int k,
                      const dnagpu_filter *filter, uint8_t *flags, int on_device);

/* ---- index over a stored kmer column: CREATE INDEX ... USING spgist (kmer_sequence spgist_kmer_ops) and the index scans
 * of `=`, `^@` and `@>` (dna--1.0.sql:304-314, dna.c:1234-1738; test.sql:156-270: kmer_data_t filled from generate_kmers,
 * indexed, asked the three operators) --------------------------------------------------------------------------------
 * dnagpu_kmer_match above is the sequential scan of such a column: it reads all of it for every query and returns flags.
 * An index is built once and asked many times; a query reads only the part of it that can hold matches and returns ROW IDS.
 * It is not an SP-GiST tree (a page-by-page access method PostgreSQL drives) but what the tree is for, as a sort and a few
 * binary searches, and it is exact: the reference's index scans lose rows (1021 of 1025 at test.sql:191 /
 * 208, 4036 of 4044 at :223 / :237) and its `@>` strategy is marked "DOES NOT WORK" (dna--1.0.sql:308).
 * Order: entries are sorted by the key's TEXT under A < T < C < G (base 0 most significant), row ids ascending among equal
 *   keys: "index order".  The keys that start with a given prefix are one contiguous window of it.
 * Storage: an index of n entries owns 12 bytes per entry from the context's pool (the stream rule below) and does not depend
 *   on the caller's key array afterwards; the build only reads that array (unlike dnagpu_count_keys).  It is kept up to date
 *   with dnagpu_kmer_index_append and dnagpu_kmer_index_delete (below) without a rebuild.  What it does not do: one k per
 *   index; one GPU; row ids are not reused; no update in place -- a changed row is a delete plus an append.
 * dnagpu_kmer_index_build: keys = n keys of k bases, host memory, or device memory when on_device != 0; bits of a key above
 *   2k are masked off; row id = position in keys.  Checks, in order: k outside 1..32: DNAGPU_ERR_INVALID_K; NULL ctx / out,
 *   NULL keys with n > 0: DNAGPU_ERR_BAD_ARG; n > 2^32 - 1: DNAGPU_ERR_TOO_LARGE (before any device work).  n == 0: a valid
 *   index of 0 rows that holds no device memory; every scan of it returns 0 rows.  An allocation failure is DNAGPU_ERR_OOM
 *   with nothing leaked and *out = NULL.
 * dnagpu_kmer_index_rows / _distinct / _k: entries now, distinct keys among them (exact after every update), k (0 for NULL).
 * dnagpu_kmer_index_scan: the rows that satisfy `filter`, in index order (NOT heap order: a caller that wants ascending row
 *   ids sorts the answer): row ids (as uint64) to out_rows and the keys to out_keys (either may be NULL), at most cap of
 *   each, host memory, or device memory when out_on_device != 0; *n_out = all matches even beyond cap; *visited (may be
 *   NULL) = the index entries inside the pruned ranges, i.e. what the query read.  Pruning: with S_i the set of codes the
 *   filter admits at position i, the prune depth p is the largest p in 0..k with |S_0| * ... * |S_(p-1)| <=
 *   DNAGPU_INDEX_MAX_RANGES; the entries whose first p bases lie in the sets are visited and positions p..k-1 are tested on
 *   each.  `=` visits its matches only, `^@` too (p = min(k, length + 5)); a pattern that opens with N's prunes little, as
 *   in any prefix tree.  NULL ctx / idx / n_out / filter: DNAGPU_ERR_BAD_ARG.  Otherwise dnagpu_kmer_match's rules exactly:
 *   a malformed filter is always an error; DNAGPU_ERR_QKMER_LEN_MISMATCH and DNAGPU_ERR_PREFIX_TOO_LONG are raised only when
 *   the index has at least one row; an EQUALS filter of another length, and a pattern with 'U', give 0 rows (visited = 0);
 *   a 32-base prefix compares all 64 bits.
 * dnagpu_kmer_index_lookup: batch equality (the join of a key list with the column): for each of m query keys of k bases
 *   the window of the index order that holds it, out_first[j] / out_count[j] (count 0: absent; first is then unspecified).
 *   A query key with bits above 2k matches nothing.  keys / out_* all host, or all device when on_device != 0.
 * dnagpu_kmer_index_read: entries [first, first + count) of the index order (dnagpu_hist_download's window rule: first > rows
 *   or count > rows - first is DNAGPU_ERR_BAD_ARG; count == 0 or both outputs NULL is DNAGPU_OK).
 * dnagpu_kmer_index_free returns the arrays to ctx's pool (NULL idx: nothing).
 * Updates (aminsert / ambulkdelete of the reference's operator class: spgist_kmer_choose / _picksplit, dna.c:1253-1502;
 * test.sql:168-184):
 * Row ids: dnagpu_kmer_index_next_row = the rows the index has ever been given, the build's n plus every append's m (0 for
 *   NULL).  Appended key j gets row id next_row + j.  Ids are never reused after a delete; dnagpu_kmer_index_rows stays
 *   "entries now".
 * dnagpu_kmer_index_append: m keys of the index's k (bits above 2k are masked off), host memory, or device memory when
 *   on_device != 0; only read.  The batch is sorted like a build and merged with the index in one stable pass, an old entry
 *   before a new one of the same key -- every new id is larger than every old one, so the result is index order, and for an
 *   index that has had no delete exactly what dnagpu_kmer_index_build gives over the concatenated column.  Checks, in order:
 *   NULL ctx / idx, NULL keys with m > 0: DNAGPU_ERR_BAD_ARG; next_row + m > 2^32 - 1: DNAGPU_ERR_TOO_LARGE (before any
 *   device work).  m == 0: DNAGPU_OK, nothing changes.  An index of 0 entries (built with n = 0, or emptied by deletes) takes
 *   an append like any other.
 * dnagpu_kmer_index_delete: rows = m row ids as uint64, in any order, host memory, or device memory when on_device != 0; only
 *   read.  Ignored: ids that are not in the index (never given, already deleted, >= next_row), repeats within the list, ids
 *   above 2^32 - 1.  *n_deleted (may be NULL) = the entries removed.  The remaining entries keep their ids and their order.
 *   NULL ctx / idx, NULL rows with m > 0: DNAGPU_ERR_BAD_ARG; m > 2^32 - 1: DNAGPU_ERR_TOO_LARGE.  Deleting every entry
 *   leaves a valid index of 0 entries that holds no device memory; next_row is unchanged.
 * Both: the new arrays are built in new pool buffers and take over only when the call succeeds (dnagpu_acc_add's rule), so
 *   every error -- DNAGPU_ERR_OOM, a HIP error -- leaves the index exactly as it was, with nothing leaked.  During the call the
 *   pool holds the old and the new arrays.  The call waits for its work: a scan right after sees the new index. */
typedef struct dnagpu_kmer_index dnagpu_kmer_index;
#define DNAGPU_INDEX_MAX_RANGES 1024u
int dnagpu_kmer_index_build(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, int k, int on_device, dnagpu_kmer_index **out);
uint64_t dnagpu_kmer_index_rows(const dnagpu_kmer_index *idx);
uint64_t dnagpu_kmer_index_distinct(const dnagpu_kmer_index *idx);
int dnagpu_kmer_index_k(const dnagpu_kmer_index *idx);
int dnagpu_kmer_index_scan(dnagpu_ctx *ctx, const dnagpu_kmer_index *idx, const dnagpu_filter *filter, uint64_t *out_rows,
                           uint64_t *out_keys, uint64_t cap, uint64_t *n_out, uint64_t *visited, int out_on_device);
int dnagpu_kmer_index_lookup(dnagpu_ctx *ctx, const dnagpu_kmer_index *idx, const uint64_t *keys, uint64_t m,
                             uint64_t *out_first, uint64_t *out_count, int on_device);
int dnagpu_kmer_index_read(dnagpu_ctx *ctx, const dnagpu_kmer_index *idx, uint64_t first, uint64_t count, uint64_t *out_rows,
                           uint64_t *out_keys, int out_on_device);
void dnagpu_kmer_index_free(dnagpu_ctx *ctx, dnagpu_kmer_index *idx);
int dnagpu_kmer_index_append(dnagpu_ctx *ctx, dnagpu_kmer_index *idx, const uint64_t *keys, uint64_t m, int on_device);
int dnagpu_kmer_index_delete(dnagpu_ctx *ctx, dnagpu_kmer_index *idx, const uint64_t *rows, uint64_t m, int on_device,
                             uint64_t *n_deleted);
uint64_t dnagpu_kmer_index_next_row(const dnagpu_kmer_index *idx);

/* ---- debug aids (off by default) ---------------------------------------------------------------
 * DNAGPU_DEBUG_POISON_POOL: every work buffer the pool hands out -- fresh or recycled, internal or through
 * dnagpu_buffer_alloc -- is first filled with 0xFF bytes on the context's stream, so a kernel that reads a
 * work buffer before writing it sees garbage in every run, not only in a warm context. */
#define DNAGPU_DEBUG_POISON_POOL 1u
/* DNAGPU_DEBUG_FORCE_SUPERKMER: dnagpu_count_kmers_unordered takes the super-k-mer engine for every k it supports
 * (20..32) and every sequence length, not only where it is the faster one (tests of its shorter windows). */
#define DNAGPU_DEBUG_FORCE_SUPERKMER 2u
/* DNAGPU_DEBUG_HEAVY_EXPAND: the super-k-mer engine expands its heavy mid buckets to keys for the ordinary levels (the
 * older path, still what records received from other ranks take when most of them are heavy) instead of splitting
 * them with the chunked level kernels. */
#define DNAGPU_DEBUG_HEAVY_EXPAND 4u
/* DNAGPU_DEBUG_GUARD_POOL: every work buffer the pool hands out is followed by a 256-byte guard band of 0xA5 bytes, placed
 * right behind the bytes that were asked for; dnagpu_synchronize() then checks every band (of buffers in use and of
 * buffers already returned) and fails with DNAGPU_ERR_INTERNAL -- dnagpu_last_error() names the buffer's size -- if a
 * kernel wrote past the end of one.  Complements DNAGPU_DEBUG_POISON_POOL (reads of memory a call never wrote). */
#define DNAGPU_DEBUG_GUARD_POOL 8u
/* Level 1 of the super-k-mer engine normally runs WITHOUT its histogram: every mid bucket is a region of the record buffer
 * sized from its parent (mean + 12.5 % + 72 records), the sweep reserves slots from cursors, and a region that overflows
 * (repeats) sends the level through the exact path (histogram, prefix, sweep).  DNAGPU_DEBUG_NO_SPEC1 always takes the exact
 * path; DNAGPU_DEBUG_SPEC1_OVERFLOW runs the speculative sweep and then treats it as overflowed (tests of the fall-back). */
#define DNAGPU_DEBUG_NO_SPEC1 16u
#define DNAGPU_DEBUG_SPEC1_OVERFLOW 32u
/* Level 0 likewise runs WITHOUT its histogram sweep on long sequences (from 2^29 rows): a histogram over 1/64 of the rows
 * sizes, per coarse bucket, the slots every chunk of rows reserves in the bucket's region; slots a chunk does not use
 * hold NULL records, which level 1 skips; a chunk that runs out of slots (or uneven buckets in the sample: repeats) sends
 * the level through the exact pair (histogram sweep, prefix, scatter sweep).  DNAGPU_DEBUG_SLAB0 takes the slab sweep for
 * every length, DNAGPU_DEBUG_NO_SLAB0 never, DNAGPU_DEBUG_SLAB0_OVERFLOW runs it and then treats it as overflowed. */
#define DNAGPU_DEBUG_SLAB0 64u
#define DNAGPU_DEBUG_NO_SLAB0 128u
#define DNAGPU_DEBUG_SLAB0_OVERFLOW 256u
/* Over uneven coarse buckets (repeats; the coarse buckets only show them on long sequences) the regions of level 1's
 * speculative sweep come from a sampled histogram -- one piece of 1024 records in every eight -- instead of the parents' sizes.
 * DNAGPU_DEBUG_SAMPLE1 takes the sampled regions whatever the coarse buckets look like (tests on short sequences). */
#define DNAGPU_DEBUG_SAMPLE1 512u
/* dnagpu_*_rank sorts by count class: the groups with a count below the class limit (2048) go straight to their class's
 * rows, the others (the tail) are sorted in chunks of up to 2^20 rows, peeled off the tail from the largest counts down.
 * DNAGPU_DEBUG_RANK_SMALL shrinks both limits -- a class limit of 4 counts, a sort chunk of 2048 rows -- so that small inputs
 * take the tail path and several peels (tests). */
#define DNAGPU_DEBUG_RANK_SMALL 1024u
/* dnagpu_acc_join picks the partition path or the direct path from the two sides' partition counts.
 * DNAGPU_DEBUG_JOIN_PARTITION takes the partition path for any sizes, DNAGPU_DEBUG_JOIN_DIRECT the direct path (tests, and
 * the probe that times both); the first holds when both are set. */
#define DNAGPU_DEBUG_JOIN_PARTITION 2048u
#define DNAGPU_DEBUG_JOIN_DIRECT 4096u
/* DNAGPU_DEBUG_WEAK_FINGERPRINT: dnagpu_table_classes and dnagpu_table_match keep only the low 2 bits of every fingerprint, so
 * that at small sizes different sequences share fingerprints: the several verify rounds of the build and the run walk of the
 * match (tests).  Results are identical with and without it. */
#define DNAGPU_DEBUG_WEAK_FINGERPRINT 8192u
/* DNAGPU_DEBUG_EARLY_L2: the record count queues level 2 behind its device-side gate after a level 1 with
 * SAMPLED regions too.  By itself it does so only after the plain speculative level: uneven coarse buckets mean repeats, whose
 * heavy and long mid buckets shut the gate, and a shut gate costs ~0.1 ms.  (Tests: the gate's verdict on such buckets.) */
#define DNAGPU_DEBUG_EARLY_L2 16384u
int dnagpu_set_debug(dnagpu_ctx *ctx, unsigned flags);

/* ---- instrumentation ------------------------------------------------------------------------
 * Device time in milliseconds (HIP events on the context's stream) of the phases of the most
 * recent dnagpu_count_kmers / dnagpu_count_keys call.  names[i] are static strings. */
#define DNAGPU_MAX_PHASES 48
typedef struct dnagpu_phase_times {
    int         n;
    const char *names[DNAGPU_MAX_PHASES];
    float       ms[DNAGPU_MAX_PHASES];
} dnagpu_phase_times;
int dnagpu_last_phase_times(dnagpu_ctx *ctx, dnagpu_phase_times *out);
/* The same for rank `rank` of the most recent dnagpu_count_multi_unordered on m: the phases of its record pass (level 0)
 * followed by those of its owner phase (a name appears once per bucket group there). */
int dnagpu_multi_last_phase_times(dnagpu_multi *m, int rank, dnagpu_phase_times *out);
/* Enables (1) / disables (0) per-phase event timing; off by default (it adds event records only). */
int dnagpu_set_profiling(dnagpu_ctx *ctx, int enabled);

#ifdef __cplusplus
}
#endif
#endif /* DNAGPU_H */
