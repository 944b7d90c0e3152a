/*
 * dna_glue.h -- host-side mirror of the reference's SQL-visible functions on the k-mer path.
 *
 * This is what the fmgr glue of dna.c looks like once its per-base loops call include/dnagpu.h:
 * the same function names, argument meaning and error text as the reference, with PostgreSQL's
 * plumbing (palloc, ereport/longjmp, the value-per-call SRF protocol, varlena headers) replaced by
 * plain C so that it builds and is testable without a PostgreSQL tree.  INTEGRATION.md maps every
 * function here to the PG_FUNCTION it stands for.
 *
 * Per-datum scalar operators (kmer_eq, starts_with, contains, kmer_hash on ONE value) stay host
 * code exactly as in the reference -- they are O(1) and run once per row inside the executor.
 * Everything that loops over a sequence (generate_kmers, its fused WHERE forms, the GROUP BY count)
 * runs on the GPU through libdnagpu.so; there is no CPU implementation of those here.
 *
 * Errors: a failing call returns NULL / false / a negative value and leaves the text the reference
 * would have passed to ereport(ERROR, errmsg(...)) in dna_glue_errmsg().
 */
#ifndef DNA_GLUE_H
#define DNA_GLUE_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dna.c:42-47 without the varlena header; `dev` caches the device-resident copy */
typedef struct Dna {
    uint64_t length;            /* nucleotides */
    uint64_t *bit_sequence;     /* ceil(length/32) words, 2 bits per base, LSB first */
    void *dev;                  /* dnagpu_dna*, created on first GPU use */
} Dna;

/* dna.c:61-65 */
typedef struct Kmer {
    int32_t length;
    uint64_t bit_sequence;
} Kmer;

/* dna.c:81-84 */
typedef struct Qkmer {
    char sequence[33];
} Qkmer;

const char *dna_glue_errmsg(void);      /* text of the last "ereport(ERROR)" on this thread */
/* Device used by this process (default 0); must be called before the first GPU call. */
void dna_glue_set_device(int device);
/* GPUs count_kmers shards over (default 1 = the single device above): ranks on HIP devices devices[0..n)
 * (NULL = 0..n-1; a device may repeat, which rehearses the path on a one-GPU box) and the exchange
 * transport (DNAGPU_MULTI_AUTO / _RCCL / _COPY of include/dnagpu.h).  Takes effect at the next count. */
void dna_glue_set_gpus(int n_gpus, const int *devices, int transport);
/* Releases the GPU context (end of backend). */
void dna_glue_shutdown(void);

/* ---- type input/output (dna.c:220-242, 528-546, 932-951) ---- */
Dna *dna_in(const char *str);
char *dna_out(const Dna *dna);          /* malloc'd */
void dna_free(Dna *dna);
uint64_t dna_length(const Dna *dna);    /* length(dna), dna.c:366-384 */
bool kmer_in(const char *str, Kmer *out);
char *kmer_out(const Kmer *kmer);       /* malloc'd */
bool qkmer_in(const char *str, Qkmer *out);

/* ---- binary I/O (dna_recv/dna_send dna.c:244-291, kmer_recv/kmer_send dna.c:552-597) ----
 * The wire image the reference describes -- length, then the packed words through pq_sendint64 --
 * with a length field that works (the reference's pq_sendint(.., 8) is rejected by PostgreSQL).
 * dna: int64 length + ceil(length/32) int64 words, network byte order; kmer: int32 length + int64. */
unsigned char *dna_send(const Dna *dna, size_t *wire_bytes);       /* malloc'd */
Dna *dna_recv(const unsigned char *wire, size_t wire_bytes);
void kmer_send(const Kmer *kmer, unsigned char wire[12]);
bool kmer_recv(const unsigned char wire[12], Kmer *out);           /* ERROR "Invalid K-mer length: must be between 1 and 32" */

/* ---- per-datum operators (host, as in the reference) ---- */
bool kmer_eq(const Kmer *a, const Kmer *b);                         /* dna.c:686-696  `=`  */
bool kmer_ne(const Kmer *a, const Kmer *b);                         /* dna.c:708-720  `<>` */
int32_t kmer_hash(const Kmer *kmer);                                /* dna.c:722-735       */
int starts_with(const Kmer *kmer, const Kmer *prefix);              /* dna.c:842-866  `^@`: 1/0, -1 = ERROR */
int contains(const Qkmer *pattern, const Kmer *kmer);               /* dna.c:1091-1135 `@>`: 1/0, -1 = ERROR */

/* ---- strand forms of one value (no counterpart in the reference): reverse_complement(dna) (malloc'd like
 * dna_in's; NULL + dna_glue_errmsg() when out of memory), reverse_complement(kmer), canonical(kmer) = whichever of the kmer and
 * its reverse complement comes first as text under A < T < C < G, the order of the kmer index (NOT A < C < G < T).  Host loops
 * over one value; the bulk forms are dnagpu_dna_revcomp and dnagpu_kmer_strand.  out may be the input. */
Dna *reverse_complement(const Dna *dna);
void kmer_reverse_complement(const Kmer *kmer, Kmer *out);
void kmer_canonical(const Kmer *kmer, Kmer *out);

/* ---- generate_kmers(dna, k) RETURNS SETOF kmer (dna.c:743-837) ----
 * begin = the SRF_IS_FIRSTCALL block (validates k, dna.c:771-773); next = one SRF_RETURN_NEXT
 * (false = SRF_RETURN_DONE).  Rows are produced on the GPU in windows and served from a host
 * buffer, one per call, in position order. */
typedef struct GenerateKmers GenerateKmers;
GenerateKmers *generate_kmers_begin(Dna *dna, int k);
bool generate_kmers_next(GenerateKmers *g, Kmer *out);
/* true when generate_kmers_next stopped because an ERROR was raised (text in dna_glue_errmsg) */
bool generate_kmers_failed(const GenerateKmers *g);
void generate_kmers_end(GenerateKmers *g);

/* generate_kmers(dna,k) AS k(kmer) WHERE <op>: the filter is evaluated inside the extraction kernel.
 * op: '=' (rhs kmer), '^' (kmer ^@ rhs kmer), '@' (rhs_pattern @> kmer).  Same rows, same order and
 * same ERRORs as evaluating the operator row by row (test.sql:61-92). */
GenerateKmers *generate_kmers_where_begin(Dna *dna, int k, char op, const Kmer *rhs, const Qkmer *rhs_pattern);

/* ---- SELECT kmer, count(*) FROM generate_kmers(dna,k) GROUP BY kmer (test.sql:95-119) as one
 * set-returning call: count_kmers(dna, k) RETURNS SETOF (kmer, bigint) ---- */
typedef struct CountKmers CountKmers;
CountKmers *count_kmers_begin(Dna *dna, int k);
bool count_kmers_next(CountKmers *c, Kmer *kmer, int64_t *count);
/* sum(count), count(*), count(*) FILTER (WHERE count = 1) over the groups (test.sql:112-114) */
void count_kmers_totals(const CountKmers *c, int64_t *total, int64_t *distinct, int64_t *unique);
void count_kmers_end(CountKmers *c);
/* ... GROUP BY k.kmer ORDER BY count(*) DESC LIMIT limit -- the reference's own first counting statement (test.sql:95) with
 * the sort and the cut done on the device (dnagpu_hist_top): count_kmers_next then serves min(limit, distinct) rows, counts
 * descending, kmers ascending among equal counts; count_kmers_totals still covers every group.  limit < 1 or >
 * DNAGPU_TOP_MAX: NULL and dna_glue_errmsg().  One device (dna_glue_set_device) whatever dna_glue_set_gpus asked for. */
CountKmers *count_kmers_top_begin(Dna *dna, int k, int64_t limit);
/* ... GROUP BY k.kmer ORDER BY count(*) DESC (descending) or ORDER BY count(*) (the rarest first) with NO LIMIT -- test.sql:95
 * as written: count_kmers_ordered(dna, int, bool) RETURNS SETOF (kmer, bigint), which replaces the planner's Sort node above
 * count_kmers.  The groups are counted, ranked on the device (dnagpu_hist_rank) and the histogram is freed; count_kmers_next
 * then serves EVERY group in count order, read from the ranking in windows of at most 2^20 rows (dnagpu_ranking_read); the
 * order among equal counts is unspecified.  count_kmers_totals still covers every group.  One device, as count_kmers_top_begin. */
CountKmers *count_kmers_ordered_begin(Dna *dna, int k, bool descending);
/* the k-mer spectrum of a count: bins[c - 1] = groups with count c, bins[n_bins - 1] = groups with count >= n_bins
 * (test.sql:112-114 is bins[0]); dnagpu_hist_spectrum.  false + dna_glue_errmsg() on an ERROR. */
bool count_kmers_spectrum(const CountKmers *c, int64_t *bins, int n_bins);

/* ---- SELECT k.kmer, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) GROUP BY k.kmer
 * (test.sql:140-150) as an aggregate over the table's rows ----
 * begin = the aggregate's first call (NULL + dna_glue_errmsg() on a bad k: dna.c:773); add = SFUNC, one call per row: the
 * row's bases are appended on the host to one packed stream at any 2-bit offset, and a batch is counted on the GPU
 * (dnagpu_count_kmers_batch) and added into a device-resident accumulator of 64-bit counts (dnagpu_acc_add) whenever it
 * reaches the flush size -- a row longer than that is a batch of its own; next = FINALFUNC rows (the first call flushes the
 * rest; false = done, or an ERROR: count_kmers_agg_failed); totals = sum(count), count(*), count(*) FILTER (WHERE count = 1),
 * valid once next has been called.  No limit on the table's size: 2^32 - 1 bases apply per batch only. */
typedef struct CountKmersAgg CountKmersAgg;
CountKmersAgg *count_kmers_agg_begin(int k);
/* the strand-neutral aggregate, count_kmers_canonical: a kmer and its reverse complement are one group, served under its
 * canonical form (above) -- every flush is dnagpu_acc_add_canonical.  Everything else (add, next, totals, _top, _order,
 * count_kmers_join_*) is the aggregate's as it is. */
CountKmersAgg *count_kmers_agg_begin_canonical(int k);
bool count_kmers_agg_add(CountKmersAgg *a, const Dna *row);
bool count_kmers_agg_next(CountKmersAgg *a, Kmer *kmer, int64_t *count);
bool count_kmers_agg_failed(const CountKmersAgg *a);
void count_kmers_agg_totals(const CountKmersAgg *a, int64_t *total, int64_t *distinct, int64_t *unique);
void count_kmers_agg_end(CountKmersAgg *a);
/* ... ORDER BY count(*) DESC LIMIT limit over the aggregate (dnagpu_acc_top): called before the first count_kmers_agg_next,
 * which then serves those rows only; false + dna_glue_errmsg() for a bad limit (as count_kmers_top_begin) or a late call */
bool count_kmers_agg_top(CountKmersAgg *a, int64_t limit);
/* ... ORDER BY count(*) [DESC] with no LIMIT over the aggregate (dnagpu_acc_rank): called before the first
 * count_kmers_agg_next, which then serves every group in count order; false + dna_glue_errmsg() for a late call.  The later
 * of count_kmers_agg_top and count_kmers_agg_order holds. */
bool count_kmers_agg_order(CountKmersAgg *a, bool descending);
/* bases per batch (default 2^30); tests use small values to force many batches */
void dna_glue_set_agg_flush_bases(uint64_t n);

/* ---- two counted tables paired on the k-mer -- what the reference's kmer_hash_ops (dna--1.0.sql:204-212) gives the planner
 * besides GROUP BY:
 *   'i'  SELECT a.kmer, a.count, b.count FROM counts_a a JOIN counts_b b ON a.kmer = b.kmer;  ... INTERSECT ...
 *   'a'  SELECT kmer FROM counts_a EXCEPT SELECT kmer FROM counts_b;  NOT IN;  NOT EXISTS      (count_right = 0)
 *   'l'  ... FROM counts_a a LEFT JOIN counts_b b ON a.kmer = b.kmer                           (count_right = 0: no partner)
 * over two count_kmers_agg aggregates.  begin flushes both (rows added so far are in; the aggregates stay usable afterwards:
 * more rows, count_kmers_agg_next, further joins), joins their accumulators on the device (dnagpu_acc_join) into device
 * buffers sized from the join's statistics, and next serves the rows, in unspecified order, from windows of at most 2^20
 * rows.  NULL + dna_glue_errmsg(): an unknown kind, sides of different k (messages of the glue's own), a failed aggregate, a
 * GPU error.  stats = count(*), sum(a.count), sum(b.count), sum(least(a.count, b.count)) over the result rows. */
typedef struct CountKmersJoin CountKmersJoin;
CountKmersJoin *count_kmers_join_begin(CountKmersAgg *left, CountKmersAgg *right, char kind);
bool count_kmers_join_next(CountKmersJoin *j, Kmer *kmer, int64_t *count_left, int64_t *count_right);
bool count_kmers_join_failed(const CountKmersJoin *j);
void count_kmers_join_stats(const CountKmersJoin *j, int64_t *rows, int64_t *sum_left, int64_t *sum_right, int64_t *sum_min);
void count_kmers_join_end(CountKmersJoin *j);


/* ---- SELECT d.id, k.kmer FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) [WHERE <op>]: the ROWS of
 * a table (what test.sql:172-176 inserts into kmer_data_t, and the WHERE forms test.sql:187-262 asks of that column) as one
 * set-returning scan, kmers_of_table ----
 * begin: op 0 = no WHERE; '=', '^', '@' as generate_kmers_where_begin (NULL + dna_glue_errmsg() on a bad k: dna.c:773);
 * add = one call per row of the table, in order (packed on the host as count_kmers_agg_add packs them); next = one row:
 * seq = the 0-based ordinal of the add call the k-mer came from, pos = its ordinal inside that row's generate_kmers, in table
 * order.  At the first next the table goes to the device in batches of at most the aggregate's flush size
 * (dna_glue_set_agg_flush_bases; a row longer than that is a batch of its own), each made resident
 * (dnagpu_dna_upload + dnagpu_dna_set_sequences) and read in windows of at most 2^20 stream rows
 * (dnagpu_generate_kmers_table).  The operator ERRORs (dna.c:854-856, 1106-1108) come at the first next, if the table has a
 * row at all; false from next = done, or an ERROR: table_kmers_failed. */
typedef struct TableKmers TableKmers;
TableKmers *table_kmers_begin(int k, char op, const Kmer *rhs, const Qkmer *rhs_pattern);
bool table_kmers_add(TableKmers *t, const Dna *row);
bool table_kmers_next(TableKmers *t, int64_t *seq, int64_t *pos, Kmer *out);
bool table_kmers_failed(const TableKmers *t);
void table_kmers_end(TableKmers *t);

/* ---- SELECT d.id, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS g(kmer) JOIN counts_b b ON g.kmer =
 * b.kmer WHERE b.count BETWEEN min_count AND max_count GROUP BY d.id: per ROW of a table, how many of its k-mers occur in a
 * counted set -- the Hash Join through kmer_hash_ops folded by sequence on the device ----
 * begin: the set is a count_kmers_agg aggregate (k is the aggregate's); begin flushes it, as count_kmers_join_begin does, and
 * the aggregate stays usable afterwards but must outlive this object.  canonical = look the canonical form of every k-mer up
 * (for an aggregate begun with count_kmers_agg_begin_canonical).  min_count <= 0 means 1, max_count < 0 no upper bound.
 * NULL + dna_glue_errmsg() for a NULL or failed aggregate or a GPU error.
 * add = one call per row, in order, packed and batched exactly as table_kmers_add does (the aggregate's flush size; a longer
 * row is a batch of its own); a batch that is full is looked up at once (dnagpu_dna_upload + dnagpu_dna_set_sequences +
 * dnagpu_table_hits) and only its 16 bytes per row are kept.  next = one row of the answer, in table order: seq = the 0-based
 * ordinal of the add call, rows = its generate_kmers rows, hits = those found in the set; the first next looks the last batch
 * up, and add is refused from then on.  totals (complete from the first next on) = sum(rows), sum(hits), rows with hits > 0. */
typedef struct TableHits TableHits;
TableHits *table_hits_begin(CountKmersAgg *set, bool canonical, int64_t min_count, int64_t max_count);
bool table_hits_add(TableHits *t, const Dna *row);
bool table_hits_next(TableHits *t, int64_t *seq, int64_t *rows, int64_t *hits);
void table_hits_totals(const TableHits *t, int64_t *rows, int64_t *hits, int64_t *seqs_hit);
bool table_hits_failed(const TableHits *t);
void table_hits_end(TableHits *t);

/* ---- SELECT d.id, k.kmer, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) GROUP BY d.id,
 * k.kmer: the k-mer profile of every ROW of a table as 4^k counts per row, k <= 6 ----
 * begin: NULL + dna_glue_errmsg() for a k outside 1 .. 32 (the reference's text, dna.c:772-773) and for k in 7 .. 32 (the
 * glue's own text: a profile that wide is not offered).  canonical = count every k-mer under its canonical form.
 * add = one call per row, in order, packed and batched exactly as table_hits_add does (the aggregate's flush size; a longer
 * row is a batch of its own); a batch that is full is profiled at once (dnagpu_dna_upload + dnagpu_dna_set_sequences +
 * dnagpu_table_profile).  next = one row of the answer, in table order: seq = the 0-based ordinal of the add call, rows =
 * its generate_kmers rows, counts[key] (table_profile_width(t) = 4^k entries, the caller's array; may be NULL) = those of
 * them whose key is `key`; the first next profiles the last batch, and add is refused from then on. */
typedef struct TableProfile TableProfile;
TableProfile *table_profile_begin(int k, bool canonical);
bool table_profile_add(TableProfile *t, const Dna *row);
bool table_profile_next(TableProfile *t, int64_t *seq, int64_t *rows, int64_t *counts);
int64_t table_profile_width(const TableProfile *t);
bool table_profile_failed(const TableProfile *t);
void table_profile_end(TableProfile *t);

/* ---- dna = dna, dna <> dna (equals / dna_ne, dna.c:334-384; the operators of dna--1.0.sql:58-86): the same
 * number of bases and every base equal.  Two host datums are a length test and a memcmp, so these two run on the host; the
 * set forms below run on the device. */
bool dna_equals(const Dna *a, const Dna *b);
bool dna_ne(const Dna *a, const Dna *b);

/* ---- SELECT min(<row ordinal>), count(*) FROM t GROUP BY sequence: the distinct ROWS of a table (dnagpu_table_classes +
 * dnagpu_seq_classes_select).  add = one call per row, in order; all rows are ONE resident table (classes span batches), so
 * more than 2^32 - 1 bases is an ERROR.  next = one class: seq = the ordinal of the first add call of that content, copies =
 * the rows equal to it; classes come in ascending seq; the first next runs the device work and add is refused from then on. */
typedef struct TableDistinct TableDistinct;
TableDistinct *table_distinct_begin(void);
bool table_distinct_add(TableDistinct *t, const Dna *row);
bool table_distinct_next(TableDistinct *t, int64_t *seq, int64_t *copies);
bool table_distinct_failed(const TableDistinct *t);
void table_distinct_end(TableDistinct *t);

/* ---- SELECT a.id, min(b.id), count(*) FROM a JOIN b ON a.sequence = b.sequence GROUP BY a.id (also WHERE sequence IN (SELECT
 * sequence FROM b)): the join of a probe table to a built one (dnagpu_table_classes over the build rows + dnagpu_table_match).
 * add_build / add_probe = one call per row of that side, in any interleaving; either side is ONE resident table (the 2^32 - 1
 * bases ERROR above).  next = one MATCHED probe row, in ascending probe ordinal: build_seq = the ordinal of the first build row
 * equal to it, copies = the build rows equal to it; a probe row without a partner gives no row. */
typedef struct TableMatch TableMatch;
TableMatch *table_match_begin(void);
bool table_match_add_build(TableMatch *t, const Dna *row);
bool table_match_add_probe(TableMatch *t, const Dna *row);
bool table_match_next(TableMatch *t, int64_t *probe_seq, int64_t *build_seq, int64_t *copies);
bool table_match_failed(const TableMatch *t);
void table_match_end(TableMatch *t);

/* ---- SELECT d.id, d.sequence, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS g(kmer) JOIN counts_b b
 * ON g.kmer = b.kmer WHERE b.count BETWEEN min_count AND max_count GROUP BY d.id, d.sequence HAVING <hits / fraction>: the
 * ROWS of a table that pass a screen against a counted set, themselves (read screening, host depletion, containment
 * filtering) ----
 * begin: set / canonical / min_count / max_count as table_hits_begin.  The HAVING forms are dnagpu_seq_hits_select's: a row
 * passes with min_hits <= hits <= max_hits and hits * frac_den >= frac_num * rows; min_hits < 0 means 0, max_hits < 0 no
 * upper bound, frac_num < 0 means 0 (0 / 1 asks nothing of the fraction; min_hits = max_hits = 0 is the depletion query).
 * NULL + dna_glue_errmsg() for frac_den <= 0, a term of the fraction above 2^32 - 1, a NULL or failed aggregate or a GPU error.
 * add = one call per row, in order, batched exactly as table_hits_add batches them (the aggregate's flush size; a longer row
 * is a batch of its own).  A batch that is full is screened at once and on the device alone: dnagpu_dna_upload +
 * dnagpu_dna_set_sequences + dnagpu_table_hits + dnagpu_seq_hits_select into device buffers + dnagpu_dna_take with those ids
 * still on the device; then dnagpu_dna_download + dnagpu_dna_sequence_starts of the taken table and the 24 bytes (id, rows,
 * hits) per passing row are all that comes back.  next = one passing row, in table order: seq = the 0-based ordinal of its add
 * call, rows / hits as table_hits_next, *row = the row itself (malloc'd: dna_free it; row may be NULL); the first next
 * screens the last batch, and add is refused from then on.  false from next = done, or an ERROR: table_screen_failed. */
typedef struct TableScreen TableScreen;
TableScreen *table_screen_begin(CountKmersAgg *set, bool canonical, int64_t min_count, int64_t max_count,
                                int64_t min_hits, int64_t max_hits, int64_t frac_num, int64_t frac_den);
bool table_screen_add(TableScreen *t, const Dna *row);
bool table_screen_next(TableScreen *t, int64_t *seq, int64_t *rows, int64_t *hits, Dna **row);
bool table_screen_failed(const TableScreen *t);
void table_screen_end(TableScreen *t);

/* ---- COPY dna_sequences (sequence) FROM '...' WITH (FORMAT text) (test.sql:128-130), and the same from a FASTA file: the
 * bytes of the file go in as they are read, the rows come out ----
 * begin: format = 1 (one sequence per line) or 2 (FASTA: '>' header lines open records), dnagpu_table_from_text's formats.
 * feed = the next bytes of the file, in order, in pieces of any size; last = these are the file's last bytes (n may be 0).
 *   The bytes are buffered; every full chunk (dna_glue_set_copy_chunk_bytes, default 64 MiB) is split, validated and packed
 *   on the device (dnagpu_table_from_text with DNAGPU_TEXT_MORE), the unfinished record at its end is carried over to the
 *   next chunk, and a record longer than the chunk doubles the chunk; the remainder is loaded without the flag on `last`.
 * next = one loaded row, in file order, as a malloc'd Dna (dna_free it; row may be NULL); line = its 1-based row of the whole
 *   file (may be NULL).  Rows can be fetched between feeds or after the last.  false = no row is waiting, or an ERROR:
 *   copy_dna_failed.
 * An input ERROR -- from feed -- carries the reference's message verbatim ("Invalid character in DNA sequence: %c", "DNA
 *   sequence cannot be empty"; FASTA: "sequence data before the first header"); after it next returns false with line = the
 *   1-based row of the whole file the error belongs to (0: before the first record), as COPY names the line, and no further
 *   row is served. */
typedef struct CopyDna CopyDna;
CopyDna *copy_dna_begin(int format);
bool copy_dna_feed(CopyDna *c, const char *bytes, size_t n, bool last);
bool copy_dna_next(CopyDna *c, Dna **row, int64_t *line);
bool copy_dna_failed(const CopyDna *c);
void copy_dna_end(CopyDna *c);
/* ---- COPY reads (record, start, sequence) FROM 'x.fastq' (INTEGRATION.md 2.4n): the same feeding, through
 * dnagpu_reads_from_text ----
 * copy_reads_begin: format = 1, 2 or 3 (FASTQ); ambiguous = DNAGPU_AMBIG_ERROR / _DROP / _SPLIT; flags = 0 or
 *   DNAGPU_READS_FOLD_CASE; min_bases: shorter sequences are left out.  The handle is fed with copy_dna_feed, asked with
 *   copy_dna_failed and ended with copy_dna_end; the chunks go through the device with DNAGPU_READS_MORE as copy_dna's do.
 * copy_reads_next = one loaded row as copy_dna_next, with record = the 0-based source record of the whole file it came from
 *   (the numbers continue across chunks) and offset = the index of its first base in that record's sequence (0 unless the
 *   policy is SPLIT); each may be NULL.  After an input ERROR it returns false with record = the 0-based source record the
 *   error belongs to (-1: none).  The messages are the library's: copy_dna's, and for FASTQ "FASTQ record does not begin
 *   with '@'", "FASTQ separator line does not begin with '+'", "truncated FASTQ record". */
CopyDna *copy_reads_begin(int format, int ambiguous, unsigned flags, uint64_t min_bases);
bool copy_reads_next(CopyDna *c, Dna **row, int64_t *record, int64_t *offset);
/* bytes per chunk of copy_dna (default 2^26); tests use small values to force many chunks */
void dna_glue_set_copy_chunk_bytes(uint64_t n);
/* ---- COPY dna_sequences (sequence) TO a text, FASTA or FASTQ file: the mirror of copy_dna, through dnagpu_table_to_text
 * (the reference calls dna_out -> decode_dna once per row, dna.c:135-152, 230-239) ----
 * copy_dna_to_begin: format = 1 (one sequence per line), 2 (FASTA, lines of line_width bases, 0 = one line) or 3 (FASTQ, every
 *   quality byte 'I'); crlf: every terminator is "\r\n".  Another format, or a line width with a format other than 2, is an
 *   ERROR (NULL) before any device is touched.  FASTA and FASTQ name row r of the whole COPY r, in decimal.
 * add = the next row.  The rows are collected; at dna_glue_set_copy_chunk_bytes of packed input they are made a resident table
 *   and written out on the device, and the names count on across such flushes.  finish = no more rows.
 * next = the next chunk of the file, at most dna_glue_set_copy_chunk_bytes of text: *bytes (not NUL-terminated, valid until the
 *   next call of next or end) and *n.  Chunks can be fetched between adds or after finish.  false = none is waiting, or an
 *   ERROR: copy_dna_to_failed. */
typedef struct CopyDnaTo CopyDnaTo;
CopyDnaTo *copy_dna_to_begin(int format, uint32_t line_width, bool crlf);
bool copy_dna_to_add(CopyDnaTo *c, const Dna *row);
bool copy_dna_to_finish(CopyDnaTo *c);
bool copy_dna_to_next(CopyDnaTo *c, const char **bytes, size_t *n);
bool copy_dna_to_failed(const CopyDnaTo *c);
void copy_dna_to_end(CopyDnaTo *c);
/* ---- FASTQ reads WITH their qualities: in through the quality column, trimmed and filtered on the
 * device; out with every quality line the row's own ----
 * trim_reads_begin: a copy_reads handle for FASTQ (ambiguous and flags as copy_reads_begin) whose chunks also go through
 *   dnagpu_quals_from_fastq and dnagpu_quals_trim: cut_front / cut_tail are cutadapt's thresholds (0: no cut), a read passes
 *   iff its kept length is > 0 and >= min_bases, its Phred sum >= min_mean_q * length, and its bases below low_q number at most
 *   low_num / low_den of it (low_den 0: no such test).  With all of them 0 it is the plain load with qualities.  A threshold
 *   above 255 is an ERROR (NULL).  Fed with copy_dna_feed, asked with copy_dna_failed, ended with copy_dna_end.
 * trim_reads_next = one passing read: its kept bases, record = its 0-based source record of the whole file, offset = the index
 *   of its first kept base in that record's sequence, *quality = its quality text (malloc'd, NUL-terminated, the caller's;
 *   NULL: not wanted).  After an input ERROR false with record as copy_reads_next.  Besides copy_reads' messages: "FASTQ
 *   quality line length differs from the sequence's", "invalid FASTQ quality character".
 * copy_reads_to_begin / _add: copy_dna_to for FASTQ where every row comes with its quality text, quality_len bytes (not
 *   NUL-terminated).  A text of another length than the row is the ERROR "FASTQ quality line length differs from the
 *   sequence's"; a byte outside 33 .. 126 is "invalid FASTQ quality character", raised when the batch is written.
 *   finish, next, failed and end are copy_dna_to's. */
CopyDna *trim_reads_begin(int ambiguous, unsigned flags, uint32_t cut_front, uint32_t cut_tail, uint64_t min_bases, uint32_t min_mean_q,
                          uint32_t low_q, uint32_t low_num, uint32_t low_den);
bool trim_reads_next(CopyDna *c, Dna **row, int64_t *record, int64_t *offset, char **quality);
CopyDnaTo *copy_reads_to_begin(bool crlf);
bool copy_reads_to_add(CopyDnaTo *c, const Dna *row, const char *quality, size_t quality_len);
bool copy_reads_to_finish(CopyDnaTo *c);
bool copy_reads_to_next(CopyDnaTo *c, const char **bytes, size_t *n);
bool copy_reads_to_failed(const CopyDnaTo *c);
void copy_reads_to_end(CopyDnaTo *c);
/* ---- the reads' own names: in through the names column, out into the headers ----
 * copy_reads_keep_names: every row of a copy_reads / trim_reads handle for FASTA or FASTQ carries the name of its source
 *   record -- the header line without its marker and terminator, with first_word cut before its first blank or tab
 *   (dnagpu_names_from_text on every chunk; after a trim dnagpu_names_take on the passing ids).  Call it after the begin and
 *   before the first feed: another format, or a call after feeding, is an ERROR (false).  Besides the loader's messages:
 *   "invalid character in a read name" for a '\r' inside a name, reported as an input ERROR with its record.
 * copy_reads_name = the name of the row last returned by copy_reads_next / trim_reads_next (NUL-terminated, *len its bytes;
 *   valid until the next call of a _next or the end; NULL before the first row or without keep_names).
 * copy_reads_to_add_named / copy_dna_to_add_named: the _add of copy_reads_to (FASTQ) / copy_dna_to (FASTA, FASTQ) where the
 *   header is the row's name, name_len bytes (not NUL-terminated), instead of the row's number.  Rows with a name and rows
 *   without one in the same handle are an ERROR; a '\r' or '\n' in a name is the library's "invalid character in a read
 *   name", raised when the batch is written. */
bool copy_reads_keep_names(CopyDna *c, bool first_word);
const char *copy_reads_name(const CopyDna *c, size_t *len);
bool copy_reads_to_add_named(CopyDnaTo *c, const Dna *row, const char *name, size_t name_len, const char *quality, size_t quality_len);
bool copy_dna_to_add_named(CopyDnaTo *c, const Dna *row, const char *name, size_t name_len);
/* ---- 3' adapters of a trim_reads handle: cut on the device behind the quality trim ----
 * trim_reads_add_adapter: one more adapter (1 .. 32 letters of the qkmer alphabet, at most 32 adapters) of a trim_reads
 *   handle.  Every chunk then goes, behind the quality trim, through dnagpu_dna_adapters: the trim's passing lists stay in
 *   device memory and are its input, a read is cut at its first hit, and min_bases is applied again to the final length; the
 *   gathers and the names take are given that call's passing lists.  trim_reads_next's offset is unchanged: a 3' cut moves no
 *   start.  With no adapter added the handle behaves exactly as without this call.
 * trim_reads_adapter_options: the error rate err_num / err_den (a hit has mismatches * err_den <= err_num * overlap), min_overlap
 *   (1 .. 32) and flags (DNAGPU_ADAPTERS_DISCARD_*; not both).  Without this call: no mismatch, min_overlap 3, no flag.
 * Both after trim_reads_begin and before the first feed: called later, on another handle, or with a bad adapter or option, an
 *   ERROR (false). */
bool trim_reads_add_adapter(CopyDna *c, const char *adapter);
bool trim_reads_adapter_options(CopyDna *c, uint32_t err_num, uint32_t err_den, uint32_t min_overlap, unsigned flags);

/* ---- CREATE INDEX ... ON kmer_data_t USING spgist (kmer_sequence spgist_kmer_ops) and the index scans of `=`, `^@` and `@>`
 * over the stored column (dna--1.0.sql:304-314; test.sql:156-270) ----
 * create: column[i] = the kmer of heap row i; the keys go to the device once and are sorted there (dnagpu_kmer_index_build).
 * An index covers ONE length: a column of mixed lengths is refused with a message of its own (a divergence: the reference's
 * operator class takes any kmer).  n == 0 is a valid, empty index.
 * scan_eq / scan_starts_with / scan_contains: the row ids that satisfy the operator, in ASCENDING ROW ORDER -- the order a
 * bitmap heap scan hands rows out in; the device answers in index order and the glue sorts on the host.  Returns the number
 * of rows and stores a malloc'd array in *rows (NULL when there are none); -1 + dna_glue_errmsg() on an ERROR: the reference's
 * own texts (dna.c:854-856, 1106-1108), raised only when the index has a row.  Exact, where the reference's index scans lose
 * rows (test.sql:191 against :208, :223 against :237) and its `@>` strategy does not work (dna--1.0.sql:308).
 * insert (aminsert; INSERT INTO kmer_data_t, test.sql:168-179): rows[j] becomes heap row first + j, first = the rows the index
 * has ever been given; returns first, or -1 + message.  One call appends one BATCH (dnagpu_kmer_index_append: a sort of the
 * batch and one merge with the index): the caller collects a statement's rows and inserts them together before the next scan.
 * A kmer of another length is refused with kmer_index_create's message for mixed lengths; an index created over an empty
 * column takes the length of its first rows.
 * delete (ambulkdelete; VACUUM, test.sql:184): removes the entries of the listed heap rows; ids the index does not hold are
 * ignored, ids are never reused.  Returns the entries removed, or -1 + message. */
typedef struct KmerIndex KmerIndex;
KmerIndex *kmer_index_create(const Kmer *column, uint64_t n);
uint64_t kmer_index_rows(const KmerIndex *idx);
int64_t kmer_index_scan_eq(KmerIndex *idx, const Kmer *rhs, int64_t **rows);
int64_t kmer_index_scan_starts_with(KmerIndex *idx, const Kmer *prefix, int64_t **rows);
int64_t kmer_index_scan_contains(KmerIndex *idx, const Qkmer *pattern, int64_t **rows);
int64_t kmer_index_insert(KmerIndex *idx, const Kmer *rows, uint64_t n);
int64_t kmer_index_delete(KmerIndex *idx, const int64_t *rows, uint64_t n);
void kmer_index_end(KmerIndex *idx);

#ifdef __cplusplus
}
#endif
#endif
