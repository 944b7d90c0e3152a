/*
 * dna_glue.c -- see dna_glue.h.  Written against the behaviour of /root/reference/dna.c (cited per
 * function); PostgreSQL plumbing replaced by plain C.  Heavy lifting: include/dnagpu.h.
 */
#include "dna_glue.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dnagpu.h"
#include "row_batch.h"

static __thread char g_msg[256];
static dnagpu_ctx *g_ctx;          /* one per process, created lazily (post-fork) */
static int g_device;

static void ereport_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
}

const char *dna_glue_errmsg(void) { return g_msg; }
void dna_glue_set_device(int device) { g_device = device; }

static void multi_shutdown(void);

void dna_glue_shutdown(void)
{
    multi_shutdown();
    if (g_ctx) {
        dnagpu_destroy(g_ctx);
        g_ctx = NULL;
    }
}

/* status of a dnagpu call -> the reference's message (codes 1..3) or the library's detail */
static bool gpu_ok(int rc)
{
    if (rc == DNAGPU_OK)
        return true;
    if (rc <= DNAGPU_ERR_QKMER_INVALID)
        ereport_error("%s", dnagpu_strerror(rc));
    else
        ereport_error("%s: %s", dnagpu_strerror(rc), dnagpu_last_error());
    return false;
}

static dnagpu_ctx *ctx(void)
{
    if (!g_ctx && !gpu_ok(dnagpu_init(g_device, &g_ctx)))
        return NULL;
    return g_ctx;
}

static dnagpu_dna *device_dna(Dna *dna)
{
    if (!dna->dev) {
        dnagpu_dna *d = NULL;
        if (!ctx() || !gpu_ok(dnagpu_dna_upload(g_ctx, dna->bit_sequence, dna->length, &d)))
            return NULL;
        dna->dev = d;
    }
    return (dnagpu_dna *)dna->dev;
}

/* ------------------------------------------------------------------ dna */

/* dna_in -> dna_make -> validate_dna_sequence + encode_dna (dna.c:220-228, 178-202, 159-171, 114-128) */
Dna *dna_in(const char *str)
{
    if (str == NULL || *str == '\0') {
        ereport_error("DNA sequence cannot be empty");                    /* dna.c:161 */
        return NULL;
    }
    for (const char *p = str; *p; p++)
        if (*p != 'A' && *p != 'T' && *p != 'C' && *p != 'G') {
            ereport_error("Invalid character in DNA sequence: %c", *p);   /* dna.c:166 */
            return NULL;
        }
    uint64_t length = (uint64_t)strlen(str);
    uint64_t n_words = (length * 2 + 63) / 64;                            /* dna.c:181-182 */
    Dna *dna = (Dna *)calloc(1, sizeof(Dna));
    uint64_t *w = (uint64_t *)calloc(n_words ? n_words : 1, sizeof(uint64_t));   /* palloc0, dna.c:186 */
    if (!dna || !w) {
        free(dna);
        free(w);
        ereport_error("out of memory");
        return NULL;
    }
    for (uint64_t i = 0; i < length; i++) {                               /* dna.c:115-127 */
        uint64_t code = str[i] == 'A' ? 0 : str[i] == 'T' ? 1 : str[i] == 'C' ? 2 : 3;
        w[i / 32] |= code << ((i * 2) % 64);
    }
    dna->length = length;
    dna->bit_sequence = w;
    return dna;
}

/* dna_out -> decode_dna (dna.c:230-242, 135-152) */
char *dna_out(const Dna *dna)
{
    static const char L[4] = { 'A', 'T', 'C', 'G' };
    char *s = (char *)malloc(dna->length + 1);
    if (!s)
        return NULL;
    for (uint64_t i = 0; i < dna->length; i++)
        s[i] = L[(dna->bit_sequence[i / 32] >> ((i * 2) % 64)) & 3];
    s[dna->length] = '\0';
    return s;
}

/* ---- binary I/O: per-datum host loops like dna_in/dna_out (bulk, device-side: dnagpu_dna_from_wire) ---- */
static void put_be64(unsigned char *p, uint64_t v)
{
    for (int i = 0; i < 8; i++)
        p[i] = (unsigned char)(v >> (56 - 8 * i));                        /* pq_sendint64 */
}
static uint64_t get_be64(const unsigned char *p)
{
    uint64_t v = 0;
    for (int i = 0; i < 8; i++)
        v = (v << 8) | p[i];                                              /* pq_getmsgint64 */
    return v;
}

/* dna_send (dna.c:270-291) */
unsigned char *dna_send(const Dna *dna, size_t *wire_bytes)
{
    uint64_t bit_length = (dna->length * 2 + 63) / 64;                    /* dna.c:279 */
    unsigned char *buf = (unsigned char *)malloc(8 + 8 * bit_length);
    if (!buf) {
        ereport_error("out of memory");
        return NULL;
    }
    put_be64(buf, dna->length);                                           /* dna.c:282, as an int64 */
    for (uint64_t i = 0; i < bit_length; i++)                             /* dna.c:284-286 */
        put_be64(buf + 8 + 8 * i, dna->bit_sequence[i]);
    *wire_bytes = 8 + 8 * bit_length;
    return buf;
}

/* dna_recv (dna.c:244-268) */
Dna *dna_recv(const unsigned char *wire, size_t wire_bytes)
{
    if (wire == NULL || wire_bytes < 8) {
        ereport_error("insufficient data left in message");               /* pq_getmsgint64's own ERROR */
        return NULL;
    }
    uint64_t length = get_be64(wire);                                     /* dna.c:251 */
    if (length == 0) {
        ereport_error("DNA sequence cannot be empty");                    /* the type's invariant, dna.c:161 */
        return NULL;
    }
    uint64_t bit_length = (length * 2 + 63) / 64;                         /* dna.c:252-253 */
    if (length > ((uint64_t)1 << 40) || wire_bytes != 8 + 8 * bit_length) {
        ereport_error("insufficient data left in message");
        return NULL;
    }
    Dna *dna = (Dna *)calloc(1, sizeof(Dna));
    uint64_t *w = (uint64_t *)calloc(bit_length, sizeof(uint64_t));       /* palloc0, dna.c:257 */
    if (!dna || !w) {
        free(dna);
        free(w);
        ereport_error("out of memory");
        return NULL;
    }
    for (uint64_t i = 0; i < bit_length; i++)                             /* dna.c:263-265 */
        w[i] = get_be64(wire + 8 + 8 * i);
    if (length % 32)
        w[bit_length - 1] &= (((uint64_t)1 << (2 * (length % 32))) - 1);  /* keep the tail bits zero (dna.c:186) */
    dna->length = length;
    dna->bit_sequence = w;
    return dna;
}

/* kmer_send (dna.c:579-597) */
void kmer_send(const Kmer *kmer, unsigned char wire[12])
{
    uint32_t l = (uint32_t)kmer->length;                                  /* dna.c:588 */
    wire[0] = (unsigned char)(l >> 24);
    wire[1] = (unsigned char)(l >> 16);
    wire[2] = (unsigned char)(l >> 8);
    wire[3] = (unsigned char)l;
    put_be64(wire + 4, kmer->bit_sequence);                               /* dna.c:591 */
}

/* kmer_recv (dna.c:552-574) */
bool kmer_recv(const unsigned char wire[12], Kmer *out)
{
    int32_t length = (int32_t)(((uint32_t)wire[0] << 24) | ((uint32_t)wire[1] << 16) |
                               ((uint32_t)wire[2] << 8) | wire[3]);       /* dna.c:559 */
    if (length <= 0 || length > 32) {
        ereport_error("Invalid K-mer length: must be between 1 and 32");  /* dna.c:566-568 */
        return false;
    }
    out->length = length;
    out->bit_sequence = get_be64(wire + 4);                               /* dna.c:571 */
    return true;
}

void dna_free(Dna *dna)
{
    if (!dna)
        return;
    if (dna->dev)
        dnagpu_dna_free(g_ctx, (dnagpu_dna *)dna->dev);
    free(dna->bit_sequence);
    free(dna);
}

uint64_t dna_length(const Dna *dna) { return dna->length; }

/* ------------------------------------------------------------------ kmer / qkmer text */

/* kmer_in -> kmer_make -> validate_kmer_sequence + encode_kmer (dna.c:528-536, 487-515, 457-479, 397-420) */
bool kmer_in(const char *str, Kmer *out)
{
    if (str == NULL) {
        ereport_error("K-mer sequence cannot be NULL");                   /* dna.c:496 */
        return false;
    }
    if (*str == '\0') {
        ereport_error("K-mer sequence cannot be empty");                  /* dna.c:461 */
        return false;
    }
    size_t len = strlen(str);
    if (len > 32) {
        ereport_error("K-mer length cannot exceed 32 nucleotides");       /* dna.c:467 */
        return false;
    }
    uint64_t bits = 0;
    for (size_t i = 0; i < len; i++) {
        uint64_t code;
        switch (str[i]) {
        case 'A': case 'X': code = 0; break;                              /* 'X' is 00 like 'A', dna.c:413 */
        case 'T': code = 1; break;
        case 'C': code = 2; break;
        case 'G': code = 3; break;
        default:
            ereport_error("Invalid character in K-mer sequence: '%c'", str[i]);   /* dna.c:473 */
            return false;
        }
        bits |= code << (2 * i);
    }
    out->length = (int32_t)len;
    out->bit_sequence = bits;
    return true;
}

/* kmer_out -> decode_kmer (dna.c:538-546, 428-452) */
char *kmer_out(const Kmer *kmer)
{
    static const char L[4] = { 'A', 'T', 'C', 'G' };
    if (kmer->length <= 0 || kmer->length > 32) {
        ereport_error("K-mer length must be between 1 and 32 nucleotides");   /* dna.c:434 */
        return NULL;
    }
    char *s = (char *)malloc((size_t)kmer->length + 1);
    if (!s)
        return NULL;
    for (int i = 0; i < kmer->length; i++)
        s[i] = L[(kmer->bit_sequence >> (2 * i)) & 3];
    s[kmer->length] = '\0';
    return s;
}

/* qkmer_in -> qkmer_make -> validate_qkmer_pattern (dna.c:932-940, 908-930, 876-900) */
bool qkmer_in(const char *str, Qkmer *out)
{
    if (str == NULL || *str == '\0') {
        ereport_error("qkmer pattern cannot be empty");                   /* dna.c:878 */
        return false;
    }
    if (strlen(str) > 32) {
        ereport_error("Qkmer pattern length cannot exceed 32 characters");   /* dna.c:884 */
        return false;
    }
    for (const char *p = str; *p; p++)
        if (!strchr("ATCGUWSMKRYBDHVN", *p)) {
            ereport_error("Invalid character in qkmer pattern: %c", *p);  /* dna.c:894 */
            return false;
        }
    strcpy(out->sequence, str);
    return true;
}

/* ------------------------------------------------------------------ per-datum operators */

bool kmer_eq(const Kmer *a, const Kmer *b)                                /* kmer_eq_internal, dna.c:655-668 */
{
    return a->length == b->length && a->bit_sequence == b->bit_sequence;
}

bool kmer_ne(const Kmer *a, const Kmer *b) { return !kmer_eq(a, b); }

/* ---- strand forms of ONE value (host loops, like every per-datum operator here; bulk: dnagpu_dna_revcomp, dnagpu_kmer_strand).
 * The complement of a base is code ^ 1 (A=00 <-> T=01, C=10 <-> G=11). */
Dna *reverse_complement(const Dna *dna)
{
    uint64_t n_words = (dna->length + 31) / 32;
    Dna *out = (Dna *)calloc(1, sizeof(Dna));
    uint64_t *w = (uint64_t *)calloc(n_words ? n_words : 1, sizeof(uint64_t));
    if (!out || !w) {
        free(out);
        free(w);
        ereport_error("out of memory");
        return NULL;
    }
    for (uint64_t j = 0; j < dna->length; j++) {
        uint64_t i = dna->length - 1 - j;
        uint64_t code = ((dna->bit_sequence[i / 32] >> ((i * 2) % 64)) & 3) ^ 1;
        w[j / 32] |= code << ((j * 2) % 64);
    }
    out->length = dna->length;
    out->bit_sequence = w;
    return out;
}

void kmer_reverse_complement(const Kmer *kmer, Kmer *out)
{
    uint64_t bits = 0;
    for (int i = 0; i < kmer->length; i++)
        bits |= (((kmer->bit_sequence >> (2 * (kmer->length - 1 - i))) & 3) ^ 1) << (2 * i);
    out->length = kmer->length;
    out->bit_sequence = bits;
}

/* whichever of kmer and its reverse complement comes first as text under A < T < C < G (the codes' own order, base 0 first:
 * the order of the kmer index) */
void kmer_canonical(const Kmer *kmer, Kmer *out)
{
    Kmer rc;
    kmer_reverse_complement(kmer, &rc);
    uint64_t own = kmer->length >= 32 ? kmer->bit_sequence : kmer->bit_sequence & (((uint64_t)1 << (2 * kmer->length)) - 1);
    bool take_rc = false;
    for (int i = 0; i < kmer->length; i++) {
        uint64_t a = (own >> (2 * i)) & 3, b = (rc.bit_sequence >> (2 * i)) & 3;
        if (a != b) {
            take_rc = b < a;
            break;
        }
    }
    out->length = kmer->length;
    out->bit_sequence = take_rc ? rc.bit_sequence : own;
}

/* dna.c:722-735: hash_any over the 8 bytes of bit_sequence (PostgreSQL hash_bytes, lookup3). */
int32_t kmer_hash(const Kmer *kmer)
{
#define ROT(x, k) (((x) << (k)) | ((x) >> (32 - (k))))
    uint32_t a, b, c;
    a = b = c = 0x9e3779b9u + 8u + 3923095u;
    b += (uint32_t)(kmer->bit_sequence >> 32);
    a += (uint32_t)kmer->bit_sequence;
    c ^= b; c -= ROT(b, 14);
    a ^= c; a -= ROT(c, 11);
    b ^= a; b -= ROT(a, 25);
    c ^= b; c -= ROT(b, 16);
    a ^= c; a -= ROT(c, 4);
    b ^= a; b -= ROT(a, 14);
    c ^= b; c -= ROT(b, 24);
#undef ROT
    return (int32_t)c;
}

/* dna.c:842-866; a 32-base prefix compares all 64 bits (the reference shifts by 64 there: UB) */
int starts_with(const Kmer *kmer, const Kmer *prefix)
{
    if (prefix->length > kmer->length) {
        ereport_error("Prefix length cannot exceed kmer length");        /* dna.c:855 */
        return -1;
    }
    uint64_t mask = prefix->length >= 32 ? ~(uint64_t)0 : (((uint64_t)1 << (2 * prefix->length)) - 1);
    return prefix->bit_sequence == (kmer->bit_sequence & mask);
}

/* nucleotide_matches (dna.c:1064-1086) as a set lookup: bit0 = A, bit1 = T, bit2 = C, bit3 = G */
static int iupac_set(char c)
{
    switch (c) {
    case 'A': return 1; case 'T': return 2; case 'C': return 4; case 'G': return 8;
    case 'U': return 0;                                                   /* never equals a decoded base */
    case 'W': return 3; case 'S': return 12; case 'M': return 5; case 'K': return 10;
    case 'R': return 9; case 'Y': return 6; case 'B': return 14; case 'D': return 11;
    case 'H': return 7; case 'V': return 13; case 'N': return 15;
    }
    return -1;
}

/* dna.c:1091-1135 */
int contains(const Qkmer *pattern, const Kmer *kmer)
{
    int qlen = (int)strlen(pattern->sequence);
    if (qlen != kmer->length) {
        ereport_error("Qkmer pattern and kmer lengths do not match");    /* dna.c:1107 */
        return -1;
    }
    for (int i = 0; i < qlen; i++) {
        int code = (int)((kmer->bit_sequence >> (2 * i)) & 3);
        int set = iupac_set(pattern->sequence[i]);
        if (set < 0) {
            ereport_error("Invalid character in pattern: %c!", pattern->sequence[i]);   /* dna.c:1083 */
            return -1;
        }
        if (!(set & (1 << code)))
            return 0;
    }
    return 1;
}

/* ------------------------------------------------------------------ generate_kmers */

#define GK_WINDOW ((uint64_t)1 << 22)     /* rows fetched from the GPU per refill (32 MiB of keys) */

struct GenerateKmers {
    Dna *dna;
    int k;
    uint64_t total;        /* max_calls, dna.c:781 */
    uint64_t next_row;     /* call_cntr */
    /* host window */
    uint64_t *keys;
    uint64_t win_first, win_count;
    /* filtered mode */
    bool filtered;
    dnagpu_filter filter;
    uint64_t scan_pos;     /* next unscanned row of generate_kmers */
    uint64_t win_used;
    bool failed;           /* an ERROR was raised: the statement is aborted */
};

static GenerateKmers *gk_new(Dna *dna, int k)
{
    uint64_t total = 0;
    if (!gpu_ok(dnagpu_kmer_count(dna->length, k, &total)))              /* dna.c:771-773 */
        return NULL;
    GenerateKmers *g = (GenerateKmers *)calloc(1, sizeof *g);
    if (!g) {
        ereport_error("out of memory");
        return NULL;
    }
    g->dna = dna;
    g->k = k;
    g->total = total;
    g->keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(total < GK_WINDOW ? (total ? total : 1) : GK_WINDOW));
    if (!g->keys) {
        free(g);
        ereport_error("out of memory");
        return NULL;
    }
    return g;
}

GenerateKmers *generate_kmers_begin(Dna *dna, int k)
{
    return gk_new(dna, k);
}

GenerateKmers *generate_kmers_where_begin(Dna *dna, int k, char op, const Kmer *rhs, const Qkmer *rhs_pattern)
{
    GenerateKmers *g = gk_new(dna, k);
    if (!g)
        return NULL;
    g->filtered = true;
    memset(&g->filter, 0, sizeof g->filter);
    switch (op) {
    case '=':
        g->filter.kind = DNAGPU_FILTER_EQUALS;
        g->filter.length = rhs->length;
        g->filter.bits = rhs->bit_sequence;
        break;
    case '^':
        g->filter.kind = DNAGPU_FILTER_STARTS_WITH;
        g->filter.length = rhs->length;
        g->filter.bits = rhs->bit_sequence;
        break;
    case '@':
        g->filter.kind = DNAGPU_FILTER_CONTAINS;
        strncpy(g->filter.pattern, rhs_pattern->sequence, sizeof g->filter.pattern - 1);
        break;
    default:
        ereport_error("unknown operator");
        generate_kmers_end(g);
        return NULL;
    }
    return g;
}

bool generate_kmers_next(GenerateKmers *g, Kmer *out)
{
    if (!g->filtered) {
        if (g->next_row >= g->total)
            return false;                                                 /* SRF_RETURN_DONE */
        if (g->next_row >= g->win_first + g->win_count) {
            dnagpu_dna *d = device_dna(g->dna);
            uint64_t n = g->total - g->next_row < GK_WINDOW ? g->total - g->next_row : GK_WINDOW;
            if (!d || !gpu_ok(dnagpu_generate_kmers(g_ctx, d, g->k, g->next_row, n, g->keys, 0))) {
                g->failed = true;
                return false;
            }
            g->win_first = g->next_row;
            g->win_count = n;
        }
        out->length = g->k;
        out->bit_sequence = g->keys[g->next_row - g->win_first];
        g->next_row++;
        return true;
    }
    /* filtered: refill with the next window of source rows until one has matches */
    while (g->win_used >= g->win_count) {
        if (g->scan_pos >= g->total)
            return false;
        dnagpu_dna *d = device_dna(g->dna);
        uint64_t n = g->total - g->scan_pos < GK_WINDOW ? g->total - g->scan_pos : GK_WINDOW;
        uint64_t n_out = 0;
        if (!d || !gpu_ok(dnagpu_generate_kmers_filtered(g_ctx, d, g->k, &g->filter, g->scan_pos, n, g->keys,
                                                          NULL, GK_WINDOW, &n_out, 0))) {
            g->scan_pos = g->total;                                       /* the ERROR aborts the statement */
            g->failed = true;
            return false;
        }
        g->scan_pos += n;
        g->win_count = n_out;
        g->win_used = 0;
    }
    out->length = g->k;
    out->bit_sequence = g->keys[g->win_used++];
    return true;
}

bool generate_kmers_failed(const GenerateKmers *g) { return g->failed; }

void generate_kmers_end(GenerateKmers *g)
{
    if (!g)
        return;
    free(g->keys);
    free(g);
}

/* ------------------------------------------------------------------ count_kmers */

#define CK_WINDOW ((uint64_t)1 << 21)
#define CK_MAX_RANKS 64

/* one histogram per rank (one rank unless dna_glue_set_gpus asked for more); rank order = ascending key ranges */
struct CountKmers {
    int k;
    int n_ranks, rank;                       /* rank = the histogram rows are being served from */
    dnagpu_hist *hist[CK_MAX_RANKS];
    dnagpu_ctx *hctx[CK_MAX_RANKS];
    dnagpu_ranking *ranking;                 /* count_kmers_ordered_begin: the rows come from it, the histogram is gone */
    uint64_t rank_distinct, next, win_first, win_count;   /* cursor inside hist[rank] */
    uint64_t distinct;
    uint64_t *keys, *counts;
    uint64_t total, unique;
};

/* multi-GPU configuration of this backend: count_kmers shards over these devices (dnagpu_count_multi) */
static int g_n_gpus = 1, g_transport = DNAGPU_MULTI_AUTO;
static int g_gpu_list[CK_MAX_RANKS];
static dnagpu_multi *g_multi;

void dna_glue_set_gpus(int n_gpus, const int *devices, int transport)
{
    if (g_multi) {
        dnagpu_multi_destroy(g_multi);
        g_multi = NULL;
    }
    g_n_gpus = n_gpus < 1 ? 1 : (n_gpus > CK_MAX_RANKS ? CK_MAX_RANKS : n_gpus);
    for (int r = 0; r < g_n_gpus; r++)
        g_gpu_list[r] = devices ? devices[r] : r;
    g_transport = transport;
}

static void multi_shutdown(void)
{
    if (g_multi) {
        dnagpu_multi_destroy(g_multi);
        g_multi = NULL;
    }
}

static dnagpu_multi *multi(void)
{
    if (!g_multi && !gpu_ok(dnagpu_multi_init(g_gpu_list, g_n_gpus, g_transport, &g_multi)))
        return NULL;
    return g_multi;
}

/* single: one histogram on this backend's device whatever dna_glue_set_gpus asked for (count_kmers_top_begin) */
static CountKmers *ck_begin(Dna *dna, int k, bool single)
{
    uint64_t n_rows = 0;
    if (!gpu_ok(dnagpu_kmer_count(dna->length, k, &n_rows)))
        return NULL;
    CountKmers *c = (CountKmers *)calloc(1, sizeof *c);
    if (!c) {
        ereport_error("out of memory");
        return NULL;
    }
    c->k = k;
    bool ok;
    if (g_n_gpus > 1 && !single) {
        /* the sequence goes to the ranks as contiguous word chunks; one all-gather + per-rank owner counts */
        dnagpu_multi *m = multi();
        dnagpu_multi_dna *md = NULL;
        ok = m && gpu_ok(dnagpu_multi_dna_upload(m, dna->bit_sequence, dna->length, &md));
        if (ok) {
            c->n_ranks = g_n_gpus;
            for (int r = 0; r < c->n_ranks; r++)
                c->hctx[r] = dnagpu_multi_ctx(m, r);
            ok = gpu_ok(dnagpu_count_multi_unordered(m, md, k, 0, n_rows, c->hist));   /* GROUP BY promises no order */
            dnagpu_multi_dna_free(m, md);
        }
    } else {
        dnagpu_dna *d = device_dna(dna);
        ok = d != NULL;
        if (ok) {
            c->n_ranks = 1;
            c->hctx[0] = g_ctx;
            /* GROUP BY promises no order (test.sql:95-104): the entry point that may partition by super-k-mers */
            ok = gpu_ok(dnagpu_count_kmers_unordered(g_ctx, d, k, 0, n_rows, &c->hist[0]));
        }
    }
    for (int r = 0; ok && r < c->n_ranks; r++) {
        uint64_t t = 0, u = 0, checksum;
        ok = gpu_ok(dnagpu_hist_summary(c->hctx[r], c->hist[r], &t, &u, &checksum));
        c->total += t;
        c->unique += u;
        c->distinct += dnagpu_hist_distinct(c->hist[r]);
    }
    if (!ok) {
        count_kmers_end(c);
        return NULL;
    }
    c->rank = 0;
    c->rank_distinct = dnagpu_hist_distinct(c->hist[0]);
    c->keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)CK_WINDOW);
    c->counts = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)CK_WINDOW);
    if (!c->keys || !c->counts) {
        ereport_error("out of memory");
        count_kmers_end(c);
        return NULL;
    }
    return c;
}

CountKmers *count_kmers_begin(Dna *dna, int k) { return ck_begin(dna, k, false); }

static bool top_limit_ok(const char *who, int64_t limit)
{
    if (limit >= 1 && limit <= (int64_t)DNAGPU_TOP_MAX)
        return true;
    ereport_error("%s: limit must be between 1 and %u", who, (unsigned)DNAGPU_TOP_MAX);
    return false;
}

/* ... GROUP BY k.kmer ORDER BY count(*) DESC LIMIT limit (test.sql:95): the rows are chosen and sorted on the device
 * (dnagpu_hist_top) and served from the window buffers, which hold DNAGPU_TOP_MAX rows */
CountKmers *count_kmers_top_begin(Dna *dna, int k, int64_t limit)
{
    if (!top_limit_ok("count_kmers_top", limit))
        return NULL;
    CountKmers *c = ck_begin(dna, k, true);
    if (!c)
        return NULL;
    uint64_t n = 0;
    if (!gpu_ok(dnagpu_hist_top(c->hctx[0], c->hist[0], (uint64_t)limit, c->keys, c->counts, &n, 0))) {
        count_kmers_end(c);
        return NULL;
    }
    c->rank_distinct = n;                        /* _next serves rows [0, n) of the one window */
    c->win_first = 0;
    c->win_count = n;
    return c;
}

/* ... GROUP BY k.kmer ORDER BY count(*) [DESC] with no LIMIT: every group ranked on the device (dnagpu_hist_rank); the
 * histogram is freed, count_kmers_next reads the ranking window by window */
#define CK_RANK_WINDOW ((uint64_t)1 << 20)
CountKmers *count_kmers_ordered_begin(Dna *dna, int k, bool descending)
{
    CountKmers *c = ck_begin(dna, k, true);
    if (!c)
        return NULL;
    if (!gpu_ok(dnagpu_hist_rank(c->hctx[0], c->hist[0], descending ? DNAGPU_ORDER_COUNT_DESC : DNAGPU_ORDER_COUNT_ASC,
                                 &c->ranking))) {
        count_kmers_end(c);
        return NULL;
    }
    dnagpu_hist_free(c->hctx[0], c->hist[0]);
    c->hist[0] = NULL;
    c->rank_distinct = dnagpu_ranking_rows(c->ranking);
    return c;
}

bool count_kmers_spectrum(const CountKmers *c, int64_t *bins, int n_bins)
{
    if (!c || !bins || n_bins < 1 || (uint64_t)n_bins > DNAGPU_SPECTRUM_MAX_BINS) {
        ereport_error("count_kmers_spectrum: n_bins must be between 1 and %u", (unsigned)DNAGPU_SPECTRUM_MAX_BINS);
        return false;
    }
    uint64_t *part = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n_bins);
    if (!part) {
        ereport_error("out of memory");
        return false;
    }
    bool ok = true;
    memset(bins, 0, sizeof(int64_t) * (size_t)n_bins);
    for (int r = 0; ok && r < c->n_ranks; r++) {     /* the ranks' groups are disjoint: their spectra add up */
        ok = gpu_ok(dnagpu_hist_spectrum(c->hctx[r], c->hist[r], (uint64_t)n_bins, part));
        for (int b = 0; ok && b < n_bins; b++)
            bins[b] += (int64_t)part[b];
    }
    free(part);
    return ok;
}

bool count_kmers_next(CountKmers *c, Kmer *kmer, int64_t *count)
{
    while (c->next >= c->rank_distinct) {            /* this rank's key range is served: on to the next one */
        if (c->rank + 1 >= c->n_ranks)
            return false;
        c->rank++;
        c->rank_distinct = dnagpu_hist_distinct(c->hist[c->rank]);
        c->next = c->win_first = c->win_count = 0;
    }
    if (c->next >= c->win_first + c->win_count) {
        uint64_t n = c->rank_distinct - c->next < CK_WINDOW ? c->rank_distinct - c->next : CK_WINDOW;
        if (c->ranking && n > CK_RANK_WINDOW)
            n = CK_RANK_WINDOW;
        if (!gpu_ok(c->ranking ? dnagpu_ranking_read(c->hctx[0], c->ranking, c->next, n, c->keys, c->counts, 0)
                               : dnagpu_hist_download(c->hctx[c->rank], c->hist[c->rank], c->next, n, c->keys, c->counts)))
            return false;
        c->win_first = c->next;
        c->win_count = n;
    }
    kmer->length = c->k;
    kmer->bit_sequence = c->keys[c->next - c->win_first];
    *count = (int64_t)c->counts[c->next - c->win_first];
    c->next++;
    return true;
}

void count_kmers_totals(const CountKmers *c, int64_t *total, int64_t *distinct, int64_t *unique)
{
    if (total) *total = (int64_t)c->total;
    if (distinct) *distinct = (int64_t)c->distinct;
    if (unique) *unique = (int64_t)c->unique;
}

void count_kmers_end(CountKmers *c)
{
    if (!c)
        return;
    for (int r = 0; r < c->n_ranks; r++)
        if (c->hist[r])
            dnagpu_hist_free(c->hctx[r], c->hist[r]);
    if (c->ranking)
        dnagpu_ranking_free(c->hctx[0], c->ranking);
    free(c->keys);
    free(c->counts);
    free(c);
}

/* ------------------------------------------------------------------ the count over a TABLE of rows as an aggregate */

static uint64_t g_agg_flush_bases = (uint64_t)1 << 30;

void dna_glue_set_agg_flush_bases(uint64_t n) { g_agg_flush_bases = n ? n : 1; }

struct CountKmersAgg {
    int k;
    bool canonical;                              /* count_kmers_agg_begin_canonical: the flush is dnagpu_acc_add_canonical */
    dnagpu_acc *acc;                             /* created on the first flush (the GPU context is lazy) */
    RowBatch b;                                  /* the open batch */
    bool finished, failed;
    uint64_t top_limit;                          /* count_kmers_agg_top: serve only the first rows of ORDER BY count(*) DESC */
    int order;                                   /* count_kmers_agg_order: 0 = none, 1 = count descending, 2 = ascending */
    dnagpu_ranking *ranking;                     /* ... every group in that order, made when the aggregate finishes */
    uint64_t serve_n;                            /* rows _next serves: distinct, or the rows of the top */
    uint64_t distinct, total, unique;
    uint64_t next, win_first, win_count;
    uint64_t *keys, *counts;
};

CountKmersAgg *count_kmers_agg_begin(int k)
{
    if (k < 1 || k > 32) {
        ereport_error("%s", dnagpu_strerror(DNAGPU_ERR_INVALID_K));          /* dna.c:772-773 */
        return NULL;
    }
    CountKmersAgg *a = (CountKmersAgg *)calloc(1, sizeof *a);
    if (!a) {
        ereport_error("out of memory");
        return NULL;
    }
    a->k = k;
    return a;
}

CountKmersAgg *count_kmers_agg_begin_canonical(int k)
{
    CountKmersAgg *a = count_kmers_agg_begin(k);
    if (a)
        a->canonical = true;
    return a;
}

/* rb_grow for the arrays of answers, with the ERROR */
static bool agg_grow(void **p, uint64_t *cap, uint64_t need)
{
    if (rb_grow(p, cap, need))
        return true;
    ereport_error("out of memory");
    return false;
}

/* the batch as a resident table with its boundaries; rows without a base make a stream of no words.  *d is the caller's to
 * free, also after an ERROR */
static bool batch_upload(const RowBatch *b, dnagpu_dna **d)
{
    static const uint64_t none[1] = {0};
    return ctx() != NULL && gpu_ok(dnagpu_dna_upload(g_ctx, b->n_bases ? b->words : none, b->n_bases, d)) &&
           gpu_ok(dnagpu_dna_set_sequences(g_ctx, *d, b->starts, b->n_seqs));
}

/* The add policy of the streaming objects: a long row gets a batch of its own (the open one is flushed first), the row goes
 * behind the batch's rows, and a batch that has reached g_agg_flush_bases is flushed.  flush(self) empties the batch. */
static bool batch_add(RowBatch *b, const Dna *row, bool (*flush)(void *), void *self)
{
    if (rb_spills(b, row->length, g_agg_flush_bases) && !flush(self))
        return false;
    if (!rb_append(b, row->bit_sequence, row->length)) {
        ereport_error("out of memory");
        return false;
    }
    return !rb_full(b, g_agg_flush_bases) || flush(self);
}

/* the batch so far: counted, added into the accumulator, emptied */
static bool agg_flush(void *self)
{
    CountKmersAgg *a = (CountKmersAgg *)self;
    bool ok = true;
    if (a->b.n_bases > 0) {
        dnagpu_dna *d = NULL;
        dnagpu_hist *h = NULL;
        ok = ctx() != NULL && (a->acc || gpu_ok(dnagpu_acc_create(g_ctx, a->k, &a->acc))) &&
             gpu_ok(dnagpu_dna_upload(g_ctx, a->b.words, a->b.n_bases, &d)) &&
             gpu_ok(dnagpu_count_kmers_batch(g_ctx, d, a->b.starts, a->b.n_seqs, a->k, &h)) &&
             gpu_ok(a->canonical ? dnagpu_acc_add_canonical(g_ctx, a->acc, h) : dnagpu_acc_add(g_ctx, a->acc, h));
        if (h)
            dnagpu_hist_free(g_ctx, h);
        if (d)
            dnagpu_dna_free(g_ctx, d);
    }
    rb_clear(&a->b);
    return ok;
}

bool count_kmers_agg_add(CountKmersAgg *a, const Dna *row)
{
    if (a->finished || a->failed) {
        ereport_error("count_kmers_agg: row added after the aggregate finished or failed");
        return false;
    }
    if (!batch_add(&a->b, row, agg_flush, a))
        a->failed = true;
    return !a->failed;
}

/* FINALFUNC's first step: the last batch, then the totals over the accumulated groups */
static bool agg_finish(CountKmersAgg *a)
{
    if (a->finished)
        return true;
    if (!agg_flush(a))
        return false;
    if (a->acc) {
        uint64_t t = 0, u = 0, checksum;
        if (!gpu_ok(dnagpu_acc_summary(g_ctx, a->acc, &t, &u, &checksum)))
            return false;
        a->total = t;
        a->unique = u;
        a->distinct = dnagpu_acc_distinct(a->acc);
    }
    a->keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)CK_WINDOW);
    a->counts = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)CK_WINDOW);
    if (!a->keys || !a->counts) {
        ereport_error("out of memory");
        return false;
    }
    a->serve_n = a->distinct;
    if (a->top_limit && a->acc) {                /* chosen and sorted on the device; the window buffers hold DNAGPU_TOP_MAX rows */
        uint64_t n = 0;
        if (!gpu_ok(dnagpu_acc_top(g_ctx, a->acc, a->top_limit, a->keys, a->counts, &n, 0)))
            return false;
        a->serve_n = n;
        a->win_first = 0;
        a->win_count = n;
    }
    if (a->order && a->acc &&
        !gpu_ok(dnagpu_acc_rank(g_ctx, a->acc, a->order == 1 ? DNAGPU_ORDER_COUNT_DESC : DNAGPU_ORDER_COUNT_ASC, &a->ranking)))
        return false;
    a->finished = true;
    return true;
}

bool count_kmers_agg_order(CountKmersAgg *a, bool descending)
{
    if (a->finished || a->failed) {
        ereport_error("count_kmers_agg_order: called after the first row was served or the aggregate failed");
        return false;
    }
    a->order = descending ? 1 : 2;
    a->top_limit = 0;
    return true;
}

bool count_kmers_agg_top(CountKmersAgg *a, int64_t limit)
{
    if (!top_limit_ok("count_kmers_agg_top", limit))
        return false;
    if (a->finished || a->failed) {
        ereport_error("count_kmers_agg_top: called after the first row was served or the aggregate failed");
        return false;
    }
    a->top_limit = (uint64_t)limit;
    a->order = 0;
    return true;
}

bool count_kmers_agg_next(CountKmersAgg *a, Kmer *kmer, int64_t *count)
{
    if (a->failed)
        return false;
    if (!agg_finish(a)) {
        a->failed = true;
        return false;
    }
    if (a->next >= a->serve_n)
        return false;
    if (a->next >= a->win_first + a->win_count) {
        uint64_t n = a->serve_n - a->next < CK_WINDOW ? a->serve_n - a->next : CK_WINDOW;
        if (a->ranking && n > CK_RANK_WINDOW)
            n = CK_RANK_WINDOW;
        if (!gpu_ok(a->ranking ? dnagpu_ranking_read(g_ctx, a->ranking, a->next, n, a->keys, a->counts, 0)
                               : dnagpu_acc_download(g_ctx, a->acc, a->next, n, a->keys, a->counts))) {
            a->failed = true;
            return false;
        }
        a->win_first = a->next;
        a->win_count = n;
    }
    kmer->length = a->k;
    kmer->bit_sequence = a->keys[a->next - a->win_first];
    *count = (int64_t)a->counts[a->next - a->win_first];
    a->next++;
    return true;
}

bool count_kmers_agg_failed(const CountKmersAgg *a) { return a->failed; }

void count_kmers_agg_totals(const CountKmersAgg *a, int64_t *total, int64_t *distinct, int64_t *unique)
{
    if (total) *total = (int64_t)a->total;
    if (distinct) *distinct = (int64_t)a->distinct;
    if (unique) *unique = (int64_t)a->unique;
}

void count_kmers_agg_end(CountKmersAgg *a)
{
    if (!a)
        return;
    if (a->ranking)
        dnagpu_ranking_free(g_ctx, a->ranking);
    if (a->acc)
        dnagpu_acc_free(g_ctx, a->acc);
    rb_free(&a->b);
    free(a->keys);
    free(a->counts);
    free(a);
}

/* ------------------------------------------------------------------ the join of two aggregates on the k-mer */

#define CK_JOIN_WINDOW ((uint64_t)1 << 20)

struct CountKmersJoin {
    int k;
    bool failed;
    dnagpu_join_stats stats;
    uint64_t rows;                               /* rows _next serves */
    uint64_t *dev[3];                            /* keys, count_left, count_right: the whole result, on the device */
    uint64_t *win[3];                            /* the window being served, on the host */
    uint64_t next, win_first, win_count;
};

/* the aggregate's accumulator with every row so far in it (an aggregate that saw no row gets an empty one) */
static dnagpu_acc *agg_flushed_acc(CountKmersAgg *a, const char *who)
{
    if (a->failed) {
        ereport_error("%s: an aggregate has failed", who);
        return NULL;
    }
    if (!agg_flush(a)) {
        a->failed = true;
        return NULL;
    }
    if (!a->acc && (!ctx() || !gpu_ok(dnagpu_acc_create(g_ctx, a->k, &a->acc))))
        return NULL;
    return a->acc;
}

CountKmersJoin *count_kmers_join_begin(CountKmersAgg *left, CountKmersAgg *right, char kind)
{
    const int kd = kind == 'i' ? DNAGPU_JOIN_INNER : kind == 'a' ? DNAGPU_JOIN_ANTI : kind == 'l' ? DNAGPU_JOIN_LEFT : -1;
    if (kd < 0) {
        ereport_error("count_kmers_join: unknown kind '%c' (expected 'i', 'a' or 'l')", kind);
        return NULL;
    }
    if (!left || !right) {
        ereport_error("count_kmers_join: an aggregate is missing");
        return NULL;
    }
    if (left->k != right->k) {
        ereport_error("count_kmers_join: the two sides count kmers of different lengths (%d and %d)", left->k, right->k);
        return NULL;
    }
    dnagpu_acc *la = agg_flushed_acc(left, "count_kmers_join");
    dnagpu_acc *ra = la ? agg_flushed_acc(right, "count_kmers_join") : NULL;
    if (!la || !ra)
        return NULL;
    CountKmersJoin *j = (CountKmersJoin *)calloc(1, sizeof *j);
    if (!j) {
        ereport_error("out of memory");
        return NULL;
    }
    j->k = left->k;
    /* the statistics size the device buffers; the second call fills them */
    uint64_t n = 0;
    bool ok = gpu_ok(dnagpu_acc_join(g_ctx, la, ra, kd, NULL, NULL, NULL, 0, &n, &j->stats, 0));
    if (ok && n > 0) {
        for (int i = 0; ok && i < 3; i++) {
            void *d = NULL;
            ok = gpu_ok(dnagpu_buffer_alloc(g_ctx, n * sizeof(uint64_t), &d));
            j->dev[i] = (uint64_t *)d;
            if (ok) {
                const uint64_t w = n < CK_JOIN_WINDOW ? n : CK_JOIN_WINDOW;
                j->win[i] = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)w);
                if (!j->win[i]) {
                    ereport_error("out of memory");
                    ok = false;
                }
            }
        }
        uint64_t got = 0;
        ok = ok && gpu_ok(dnagpu_acc_join(g_ctx, la, ra, kd, j->dev[0], j->dev[1], j->dev[2], n, &got, NULL, 1));
        if (ok && got != n) {
            ereport_error("count_kmers_join: %llu rows, then %llu", (unsigned long long)n, (unsigned long long)got);
            ok = false;
        }
    }
    if (!ok) {
        count_kmers_join_end(j);
        return NULL;
    }
    j->rows = n;
    return j;
}

bool count_kmers_join_next(CountKmersJoin *j, Kmer *kmer, int64_t *count_left, int64_t *count_right)
{
    if (j->failed || j->next >= j->rows)
        return false;
    if (j->next >= j->win_first + j->win_count) {
        const uint64_t n = j->rows - j->next < CK_JOIN_WINDOW ? j->rows - j->next : CK_JOIN_WINDOW;
        for (int i = 0; i < 3; i++)
            if (!gpu_ok(dnagpu_buffer_download(g_ctx, j->dev[i] + j->next, n * sizeof(uint64_t), j->win[i]))) {
                j->failed = true;
                return false;
            }
        j->win_first = j->next;
        j->win_count = n;
    }
    const uint64_t at = j->next - j->win_first;
    kmer->length = j->k;
    kmer->bit_sequence = j->win[0][at];
    *count_left = (int64_t)j->win[1][at];
    *count_right = (int64_t)j->win[2][at];
    j->next++;
    return true;
}

bool count_kmers_join_failed(const CountKmersJoin *j) { return j->failed; }

void count_kmers_join_stats(const CountKmersJoin *j, int64_t *rows, int64_t *sum_left, int64_t *sum_right, int64_t *sum_min)
{
    if (rows) *rows = (int64_t)j->stats.rows;
    if (sum_left) *sum_left = (int64_t)j->stats.sum_left;
    if (sum_right) *sum_right = (int64_t)j->stats.sum_right;
    if (sum_min) *sum_min = (int64_t)j->stats.sum_min;
}

void count_kmers_join_end(CountKmersJoin *j)
{
    if (!j)
        return;
    for (int i = 0; i < 3; i++) {
        if (j->dev[i])
            dnagpu_buffer_free(g_ctx, j->dev[i]);
        free(j->win[i]);
    }
    free(j);
}

/* ------------------------------------------------------------------ the ROWS of a table: kmers_of_table */

#define TK_WINDOW ((uint64_t)1 << 20)     /* stream rows per refill: a window never holds more table rows than stream rows */

typedef struct TableBatch {
    RowBatch b;
    uint64_t first_seq;                          /* ordinal of the batch's first row in the table */
} TableBatch;

struct TableKmers {
    int k;
    bool filtered, started, failed, open;        /* open: the last batch still takes rows */
    dnagpu_filter filter;
    TableBatch *batches;
    uint64_t n_batches, cap_batches, n_rows;     /* n_rows: add calls so far */
    /* the scan */
    uint64_t cur;                                /* batch being read */
    dnagpu_dna *dev;                             /* ... resident, with its sequence set */
    uint64_t scan_pos, scan_total;               /* stream rows of the batch: next unscanned, all */
    uint64_t *keys, *seq, *pos, win_count, win_used;
};

TableKmers *table_kmers_begin(int k, char op, const Kmer *rhs, const Qkmer *rhs_pattern)
{
    if (k < 1 || k > 32) {
        ereport_error("%s", dnagpu_strerror(DNAGPU_ERR_INVALID_K));          /* dna.c:772-773 */
        return NULL;
    }
    TableKmers *t = (TableKmers *)calloc(1, sizeof *t);
    if (!t) {
        ereport_error("out of memory");
        return NULL;
    }
    t->k = k;
    t->filtered = op != 0;
    switch (op) {
    case 0:
        break;
    case '=':
    case '^':
        t->filter.kind = op == '=' ? DNAGPU_FILTER_EQUALS : DNAGPU_FILTER_STARTS_WITH;
        t->filter.length = rhs->length;
        t->filter.bits = rhs->bit_sequence;
        break;
    case '@':
        t->filter.kind = DNAGPU_FILTER_CONTAINS;
        strncpy(t->filter.pattern, rhs_pattern->sequence, sizeof t->filter.pattern - 1);
        break;
    default:
        ereport_error("unknown operator");
        free(t);
        return NULL;
    }
    return t;
}

bool table_kmers_add(TableKmers *t, const Dna *row)
{
    if (t->started || t->failed) {
        ereport_error("table_kmers: row added after the first row was served or the scan failed");
        return false;
    }
    TableBatch *b = t->open ? &t->batches[t->n_batches - 1] : NULL;
    if (b && rb_spills(&b->b, row->length, g_agg_flush_bases))                  /* a long row: a batch of its own */
        b = NULL;
    if (!b) {
        if (t->n_batches == t->cap_batches) {
            const uint64_t c = t->cap_batches ? 2 * t->cap_batches : 16;
            TableBatch *q = (TableBatch *)realloc(t->batches, (size_t)c * sizeof *q);
            if (!q) {
                ereport_error("out of memory");
                t->failed = true;
                return false;
            }
            t->batches = q;
            t->cap_batches = c;
        }
        b = &t->batches[t->n_batches++];
        memset(b, 0, sizeof *b);
        b->first_seq = t->n_rows;
    }
    if (!rb_append(&b->b, row->bit_sequence, row->length)) {
        ereport_error("out of memory");
        t->failed = true;
        return false;
    }
    t->n_rows++;
    t->open = !rb_full(&b->b, g_agg_flush_bases);
    return true;
}

static void tk_drop_device(TableKmers *t)
{
    if (t->dev)
        dnagpu_dna_free(g_ctx, t->dev);
    t->dev = NULL;
}

/* batch t->cur onto the device with its boundaries; false = ERROR */
static bool tk_open_batch(TableKmers *t)
{
    const RowBatch *b = &t->batches[t->cur].b;
    t->scan_pos = 0;
    t->scan_total = b->n_bases >= (uint64_t)t->k ? b->n_bases - (uint64_t)t->k + 1 : 0;
    if (t->scan_total == 0)
        return true;
    return batch_upload(b, &t->dev);
}

bool table_kmers_next(TableKmers *t, int64_t *seq, int64_t *pos, Kmer *out)
{
    if (t->failed)
        return false;
    if (!t->started) {
        t->started = true;
        t->keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)TK_WINDOW);
        t->seq = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)TK_WINDOW);
        t->pos = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)TK_WINDOW);
        if (!t->keys || !t->seq || !t->pos) {
            ereport_error("out of memory");
            t->failed = true;
            return false;
        }
        if (t->n_batches && !tk_open_batch(t)) {
            t->failed = true;
            return false;
        }
    }
    while (t->win_used >= t->win_count) {                                 /* the next window with rows */
        if (t->cur >= t->n_batches)
            return false;
        if (t->scan_pos >= t->scan_total) {                               /* the next batch */
            tk_drop_device(t);
            if (++t->cur >= t->n_batches)
                return false;
            if (!tk_open_batch(t)) {
                t->failed = true;
                return false;
            }
            continue;
        }
        const uint64_t n = t->scan_total - t->scan_pos < TK_WINDOW ? t->scan_total - t->scan_pos : TK_WINDOW;
        uint64_t n_out = 0;
        if (!gpu_ok(dnagpu_generate_kmers_table(g_ctx, t->dev, t->k, t->filtered ? &t->filter : NULL, t->scan_pos, n, t->keys,
                                                t->seq, t->pos, TK_WINDOW, &n_out, 0))) {
            t->failed = true;                                             /* the ERROR aborts the statement */
            return false;
        }
        t->scan_pos += n;
        t->win_count = n_out;
        t->win_used = 0;
    }
    const uint64_t i = t->win_used++;
    if (seq)
        *seq = (int64_t)(t->batches[t->cur].first_seq + t->seq[i]);
    if (pos)
        *pos = (int64_t)t->pos[i];
    out->length = t->k;
    out->bit_sequence = t->keys[i];
    return true;
}

bool table_kmers_failed(const TableKmers *t) { return t->failed; }

void table_kmers_end(TableKmers *t)
{
    if (!t)
        return;
    tk_drop_device(t);
    for (uint64_t i = 0; i < t->n_batches; i++)
        rb_free(&t->batches[i].b);
    free(t->batches);
    free(t->keys);
    free(t->seq);
    free(t->pos);
    free(t);
}

/* ------------------------------------------------------------------ per-row hits of a table in a counted set: table_hits */

struct TableHits {
    dnagpu_acc *set;                             /* the aggregate's accumulator (the aggregate outlives this object) */
    unsigned flags;
    uint64_t min_count, max_count;
    bool started, failed;
    RowBatch b;                                  /* the open batch */
    uint64_t *rows, *hits, n_done, cap_rows, cap_hits;      /* the answers of the rows of the batches looked up so far */
    uint64_t next;
    uint64_t tot_rows, tot_hits, tot_seqs_hit;
};

TableHits *table_hits_begin(CountKmersAgg *set, bool canonical, int64_t min_count, int64_t max_count)
{
    if (!set) {
        ereport_error("table_hits: the aggregate is missing");
        return NULL;
    }
    dnagpu_acc *acc = agg_flushed_acc(set, "table_hits");
    if (!acc)
        return NULL;
    TableHits *t = (TableHits *)calloc(1, sizeof *t);
    if (!t) {
        ereport_error("out of memory");
        return NULL;
    }
    t->set = acc;
    t->flags = canonical ? DNAGPU_HITS_CANONICAL : 0u;
    t->min_count = min_count > 0 ? (uint64_t)min_count : 1;
    t->max_count = max_count < 0 ? UINT64_MAX : (uint64_t)max_count;
    return t;
}

/* the open batch: looked up on the device, its answers appended, emptied */
static bool th_flush(void *self)
{
    TableHits *t = (TableHits *)self;
    const uint64_t n = t->b.n_seqs;
    if (n == 0)
        return true;
    if (!agg_grow((void **)&t->rows, &t->cap_rows, t->n_done + n) || !agg_grow((void **)&t->hits, &t->cap_hits, t->n_done + n))
        return false;
    bool ok = true;
    if (t->b.n_bases == 0) {                                              /* empty rows only: nothing to upload */
        memset(t->rows + t->n_done, 0, (size_t)n * sizeof(uint64_t));
        memset(t->hits + t->n_done, 0, (size_t)n * sizeof(uint64_t));
    } else {
        dnagpu_dna *d = NULL;
        dnagpu_seq_hits *h = NULL;
        uint64_t r = 0, c = 0, s = 0;
        ok = batch_upload(&t->b, &d) &&
             gpu_ok(dnagpu_table_hits(g_ctx, d, t->set, t->flags, t->min_count, t->max_count, 0, n, &h)) &&
             gpu_ok(dnagpu_seq_hits_read(g_ctx, h, 0, n, t->rows + t->n_done, t->hits + t->n_done, 0)) &&
             gpu_ok(dnagpu_seq_hits_totals(h, &r, &c, &s));
        if (ok) {
            t->tot_rows += r;
            t->tot_hits += c;
            t->tot_seqs_hit += s;
        }
        if (h)
            dnagpu_seq_hits_free(g_ctx, h);
        if (d)
            dnagpu_dna_free(g_ctx, d);
    }
    if (ok)
        t->n_done += n;
    rb_clear(&t->b);
    return ok;
}

bool table_hits_add(TableHits *t, const Dna *row)
{
    if (t->started || t->failed) {
        ereport_error("table_hits: row added after the first row was served or the scan failed");
        return false;
    }
    if (!batch_add(&t->b, row, th_flush, t))
        t->failed = true;
    return !t->failed;
}

bool table_hits_next(TableHits *t, int64_t *seq, int64_t *rows, int64_t *hits)
{
    if (t->failed)
        return false;
    if (!t->started) {
        t->started = true;
        if (!th_flush(t)) {                                               /* the last batch */
            t->failed = true;
            return false;
        }
    }
    if (t->next >= t->n_done)
        return false;
    const uint64_t i = t->next++;
    if (seq)
        *seq = (int64_t)i;
    if (rows)
        *rows = (int64_t)t->rows[i];
    if (hits)
        *hits = (int64_t)t->hits[i];
    return true;
}

void table_hits_totals(const TableHits *t, int64_t *rows, int64_t *hits, int64_t *seqs_hit)
{
    if (rows) *rows = (int64_t)t->tot_rows;
    if (hits) *hits = (int64_t)t->tot_hits;
    if (seqs_hit) *seqs_hit = (int64_t)t->tot_seqs_hit;
}

bool table_hits_failed(const TableHits *t) { return t->failed; }

void table_hits_end(TableHits *t)
{
    if (!t)
        return;
    rb_free(&t->b);
    free(t->rows);
    free(t->hits);
    free(t);
}

/* ------------------------------------------------------------------ the k-mer profile of every row of a table: table_profile */

struct TableProfile {
    int k;
    unsigned flags;
    uint64_t width;                              /* 4^k */
    bool started, failed;
    RowBatch b;                                  /* the open batch */
    uint64_t *rows, n_done, cap_rows;            /* the answers of the rows of the batches profiled so far */
    uint32_t *counts;                            /* n_done * width */
    uint64_t cap_counts;                         /* in 8-byte units (agg_grow's) */
    uint64_t next;
};

TableProfile *table_profile_begin(int k, bool canonical)
{
    if (k < 1 || k > 32) {
        ereport_error("%s", dnagpu_strerror(DNAGPU_ERR_INVALID_K));          /* dna.c:772-773 */
        return NULL;
    }
    if (k > DNAGPU_PROFILE_MAX_K) {
        ereport_error("table_profile: a profile has 4^k columns and is offered for k <= %d", DNAGPU_PROFILE_MAX_K);
        return NULL;
    }
    TableProfile *t = (TableProfile *)calloc(1, sizeof *t);
    if (!t) {
        ereport_error("out of memory");
        return NULL;
    }
    t->k = k;
    t->flags = canonical ? DNAGPU_PROFILE_CANONICAL : 0u;
    t->width = dnagpu_profile_width(k);
    return t;
}

/* the open batch: profiled on the device, its answers appended, emptied */
static bool tp_flush(void *self)
{
    TableProfile *t = (TableProfile *)self;
    const uint64_t n = t->b.n_seqs;
    if (n == 0)
        return true;
    if (!agg_grow((void **)&t->rows, &t->cap_rows, t->n_done + n) ||
        !agg_grow((void **)&t->counts, &t->cap_counts, ((t->n_done + n) * t->width + 1) / 2))
        return false;
    uint32_t *counts = t->counts + t->n_done * t->width;
    bool ok = true;
    if (t->b.n_bases == 0) {                                              /* empty rows only: nothing to upload */
        memset(t->rows + t->n_done, 0, (size_t)n * sizeof(uint64_t));
        memset(counts, 0, (size_t)(n * t->width) * sizeof(uint32_t));
    } else {
        dnagpu_dna *d = NULL;
        ok = batch_upload(&t->b, &d) &&
             gpu_ok(dnagpu_table_profile(g_ctx, d, t->k, t->flags, 0, n, counts, t->rows + t->n_done, 0));
        if (d)
            dnagpu_dna_free(g_ctx, d);
    }
    if (ok)
        t->n_done += n;
    rb_clear(&t->b);
    return ok;
}

bool table_profile_add(TableProfile *t, const Dna *row)
{
    if (t->started || t->failed) {
        ereport_error("table_profile: row added after the first row was served or the scan failed");
        return false;
    }
    if (!batch_add(&t->b, row, tp_flush, t))
        t->failed = true;
    return !t->failed;
}

bool table_profile_next(TableProfile *t, int64_t *seq, int64_t *rows, int64_t *counts)
{
    if (t->failed)
        return false;
    if (!t->started) {
        t->started = true;
        if (!tp_flush(t)) {                                               /* the last batch */
            t->failed = true;
            return false;
        }
    }
    if (t->next >= t->n_done)
        return false;
    const uint64_t i = t->next++;
    if (seq)
        *seq = (int64_t)i;
    if (rows)
        *rows = (int64_t)t->rows[i];
    if (counts)
        for (uint64_t c = 0; c < t->width; c++)
            counts[c] = (int64_t)t->counts[i * t->width + c];
    return true;
}

int64_t table_profile_width(const TableProfile *t) { return (int64_t)t->width; }

bool table_profile_failed(const TableProfile *t) { return t->failed; }

void table_profile_end(TableProfile *t)
{
    if (!t)
        return;
    rb_free(&t->b);
    free(t->rows);
    free(t->counts);
    free(t);
}

/* ------------------------------------------------------------------ equal rows: dna = dna, table_distinct, table_match */

/* equals / dna_ne (dna_eq_internal, dna.c:334-384): two host datums are a length test and a memcmp, so these run on the host;
 * bits behind the last base are not compared (the reference relies on zero tails) */
bool dna_equals(const Dna *a, const Dna *b)
{
    if (a->length != b->length)
        return false;
    const uint64_t full = a->length / 32, rest = a->length % 32;
    if (full && memcmp(a->bit_sequence, b->bit_sequence, (size_t)full * sizeof(uint64_t)) != 0)
        return false;
    if (rest) {
        const uint64_t mask = ((uint64_t)1 << (2 * rest)) - 1;
        return ((a->bit_sequence[full] ^ b->bit_sequence[full]) & mask) == 0;
    }
    return true;
}

bool dna_ne(const Dna *a, const Dna *b) { return !dna_equals(a, b); }

#define TABLE_MAX_BASES 0xFFFFFFFFull            /* one resident table: dnagpu_dna_set_sequences' limit */

/* one side of table_distinct / table_match: the rows packed back to back, ONE resident table when uploaded */
typedef struct EqSide {
    RowBatch b;
    dnagpu_dna *dev;
} EqSide;

static bool eq_side_add(EqSide *s, const Dna *row, const char *who)
{
    if (row->length > TABLE_MAX_BASES - s->b.n_bases) {
        ereport_error("%s: the rows hold more than 4294967295 bases (2^32 - 1), the limit of one resident table", who);
        return false;
    }
    if (!rb_append(&s->b, row->bit_sequence, row->length)) {
        ereport_error("out of memory");
        return false;
    }
    return true;
}

static void eq_side_free(EqSide *s)
{
    if (s->dev)
        dnagpu_dna_free(g_ctx, s->dev);
    rb_free(&s->b);
    s->dev = NULL;
}

struct TableDistinct {
    EqSide rows;
    bool started, failed;
    uint64_t *seq, *copies, n_out, next;         /* the representatives, ascending */
};

TableDistinct *table_distinct_begin(void)
{
    TableDistinct *t = (TableDistinct *)calloc(1, sizeof *t);
    if (!t)
        ereport_error("out of memory");
    return t;
}

bool table_distinct_add(TableDistinct *t, const Dna *row)
{
    if (t->started || t->failed) {
        ereport_error("table_distinct: row added after the first row was served or the scan failed");
        return false;
    }
    if (!eq_side_add(&t->rows, row, "table_distinct")) {
        t->failed = true;
        return false;
    }
    return true;
}

/* the whole table: classes on the device, the representatives read back */
static bool td_run(TableDistinct *t)
{
    if (t->rows.b.n_seqs == 0)
        return true;
    dnagpu_seq_classes *c = NULL;
    uint64_t n = 0;
    bool ok = batch_upload(&t->rows.b, &t->rows.dev) && gpu_ok(dnagpu_table_classes(g_ctx, t->rows.dev, &c));
    if (ok) {
        n = dnagpu_seq_classes_distinct(c);
        t->seq = (uint64_t *)malloc((size_t)(n ? n : 1) * sizeof(uint64_t));
        t->copies = (uint64_t *)malloc((size_t)(n ? n : 1) * sizeof(uint64_t));
        if (!t->seq || !t->copies) {
            ereport_error("out of memory");
            ok = false;
        }
    }
    ok = ok && gpu_ok(dnagpu_seq_classes_select(g_ctx, c, 1, UINT64_MAX, t->seq, t->copies, n, &t->n_out, 0));
    if (ok && t->n_out != n) {
        ereport_error("table_distinct: the select returned %llu of %llu classes", (unsigned long long)t->n_out, (unsigned long long)n);
        ok = false;
    }
    if (c)
        dnagpu_seq_classes_free(g_ctx, c);
    return ok;
}

bool table_distinct_next(TableDistinct *t, int64_t *seq, int64_t *copies)
{
    if (t->failed)
        return false;
    if (!t->started) {
        t->started = true;
        if (!td_run(t)) {
            t->failed = true;
            return false;
        }
    }
    if (t->next >= t->n_out)
        return false;
    const uint64_t i = t->next++;
    if (seq)
        *seq = (int64_t)t->seq[i];
    if (copies)
        *copies = (int64_t)t->copies[i];
    return true;
}

bool table_distinct_failed(const TableDistinct *t) { return t->failed; }

void table_distinct_end(TableDistinct *t)
{
    if (!t)
        return;
    eq_side_free(&t->rows);
    free(t->seq);
    free(t->copies);
    free(t);
}

struct TableMatch {
    EqSide build, probe;
    bool started, failed;
    uint64_t *match, *copies, next;              /* one entry per probe row */
};

TableMatch *table_match_begin(void)
{
    TableMatch *t = (TableMatch *)calloc(1, sizeof *t);
    if (!t)
        ereport_error("out of memory");
    return t;
}

static bool tm_add(TableMatch *t, EqSide *side, const Dna *row)
{
    if (t->started || t->failed) {
        ereport_error("table_match: row added after the first row was served or the scan failed");
        return false;
    }
    if (!eq_side_add(side, row, "table_match")) {
        t->failed = true;
        return false;
    }
    return true;
}

bool table_match_add_build(TableMatch *t, const Dna *row) { return tm_add(t, &t->build, row); }
bool table_match_add_probe(TableMatch *t, const Dna *row) { return tm_add(t, &t->probe, row); }

static bool tm_run(TableMatch *t)
{
    const uint64_t np = t->probe.b.n_seqs;
    if (np == 0 || t->build.b.n_seqs == 0) {       /* nothing to ask, or nothing to find: no row */
        t->probe.b.n_seqs = 0;
        return true;
    }
    t->match = (uint64_t *)malloc((size_t)np * sizeof(uint64_t));
    t->copies = (uint64_t *)malloc((size_t)np * sizeof(uint64_t));
    if (!t->match || !t->copies) {
        ereport_error("out of memory");
        return false;
    }
    dnagpu_seq_classes *c = NULL;
    const bool ok = batch_upload(&t->build.b, &t->build.dev) && batch_upload(&t->probe.b, &t->probe.dev) &&
                    gpu_ok(dnagpu_table_classes(g_ctx, t->build.dev, &c)) &&
                    gpu_ok(dnagpu_table_match(g_ctx, c, t->probe.dev, 0, np, t->match, t->copies, NULL, 0));
    if (c)
        dnagpu_seq_classes_free(g_ctx, c);
    return ok;
}

bool table_match_next(TableMatch *t, int64_t *probe_seq, int64_t *build_seq, int64_t *copies)
{
    if (t->failed)
        return false;
    if (!t->started) {
        t->started = true;
        if (!tm_run(t)) {
            t->failed = true;
            return false;
        }
    }
    while (t->next < t->probe.b.n_seqs && t->match[t->next] == DNAGPU_MATCH_NONE)
        t->next++;                               /* (an inner join: a probe row without a partner gives no row) */
    if (t->next >= t->probe.b.n_seqs)
        return false;
    const uint64_t i = t->next++;
    if (probe_seq)
        *probe_seq = (int64_t)i;
    if (build_seq)
        *build_seq = (int64_t)t->match[i];
    if (copies)
        *copies = (int64_t)t->copies[i];
    return true;
}

bool table_match_failed(const TableMatch *t) { return t->failed; }

void table_match_end(TableMatch *t)
{
    if (!t)
        return;
    eq_side_free(&t->build);
    eq_side_free(&t->probe);
    free(t->match);
    free(t->copies);
    free(t);
}

/* ------------------------------------------------------------------ the rows of a table that pass a screen: table_screen */

_Static_assert(sizeof(Dna *) == sizeof(uint64_t), "agg_grow sizes the array of rows");

struct TableScreen {
    dnagpu_acc *set;                             /* the aggregate's accumulator (the aggregate outlives this object) */
    unsigned flags;
    uint64_t min_count, max_count, min_hits, max_hits, frac_num, frac_den;
    bool started, failed;
    RowBatch b;                                  /* the open batch */
    uint64_t n_added;                            /* rows of the batches screened so far = the ordinal of the open batch's first row */
    uint64_t *seq, *rows, *hits, cap_seq, cap_rows, cap_hits;     /* the passing rows of the batches screened so far ... */
    Dna **out;                                   /* ... and the rows themselves (NULL once handed out) */
    uint64_t cap_out, n_pass, next;
};

TableScreen *table_screen_begin(CountKmersAgg *set, bool canonical, int64_t min_count, int64_t max_count, int64_t min_hits,
                                int64_t max_hits, int64_t frac_num, int64_t frac_den)
{
    if (!set) {
        ereport_error("table_screen: the aggregate is missing");
        return NULL;
    }
    if (frac_den <= 0) {
        ereport_error("table_screen: the fraction's denominator must be positive");
        return NULL;
    }
    if (frac_den > (int64_t)UINT32_MAX || frac_num > (int64_t)UINT32_MAX) {
        ereport_error("table_screen: the terms of the fraction must be below 2^32");
        return NULL;
    }
    dnagpu_acc *acc = agg_flushed_acc(set, "table_screen");
    if (!acc)
        return NULL;
    TableScreen *t = (TableScreen *)calloc(1, sizeof *t);
    if (!t) {
        ereport_error("out of memory");
        return NULL;
    }
    t->set = acc;
    t->flags = canonical ? DNAGPU_HITS_CANONICAL : 0u;
    t->min_count = min_count > 0 ? (uint64_t)min_count : 1;
    t->max_count = max_count < 0 ? UINT64_MAX : (uint64_t)max_count;
    t->min_hits = min_hits > 0 ? (uint64_t)min_hits : 0;
    t->max_hits = max_hits < 0 ? UINT64_MAX : (uint64_t)max_hits;
    t->frac_num = frac_num > 0 ? (uint64_t)frac_num : 0;
    t->frac_den = (uint64_t)frac_den;
    return t;
}

/* bases [first, first + len) of a packed stream as a value of its own */
static Dna *dna_cut(const uint64_t *src, uint64_t first, uint64_t len)
{
    const uint64_t nw = (len + 31) / 32;
    Dna *out = (Dna *)calloc(1, sizeof(Dna));
    uint64_t *w = (uint64_t *)calloc(nw ? nw : 1, sizeof(uint64_t));
    if (!out || !w) {
        free(out);
        free(w);
        ereport_error("out of memory");
        return NULL;
    }
    rb_cut(src, first, len, w);
    out->length = len;
    out->bit_sequence = w;
    return out;
}

static bool ts_grow(TableScreen *t, uint64_t more)
{
    const uint64_t need = t->n_pass + more;
    return agg_grow((void **)&t->seq, &t->cap_seq, need) && agg_grow((void **)&t->rows, &t->cap_rows, need) &&
           agg_grow((void **)&t->hits, &t->cap_hits, need) && agg_grow((void **)&t->out, &t->cap_out, need);
}

/* the first n sequences of a resident table as values of their own: out[0 .. n), cut from one download of the stream and of
 * its starts.  On failure none of them stays allocated. */
static bool table_rows(const dnagpu_dna *table, uint64_t n, Dna **out)
{
    const uint64_t total = dnagpu_dna_length(table);
    uint64_t *words = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)((total + 31) / 32 + 1));
    uint64_t *starts = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n + 1));
    bool ok = words && starts;
    if (!ok)
        ereport_error("out of memory");
    ok = ok && gpu_ok(dnagpu_dna_download(g_ctx, table, words)) && gpu_ok(dnagpu_dna_sequence_starts(g_ctx, table, 0, n + 1, starts, 0));
    uint64_t made = 0;
    for (; ok && made < n; made++) {
        out[made] = dna_cut(words, starts[made], starts[made + 1] - starts[made]);
        if (!out[made])
            break;
    }
    if (made < n) {
        ok = false;
        while (made > 0)
            dna_free(out[--made]);
    }
    free(words);
    free(starts);
    return ok;
}

/* the n_out passing rows of the open batch: their ids, rows and hits from the select's device buffers (n entries apart), the
 * rows themselves from the taken table */
static bool ts_collect(TableScreen *t, const dnagpu_dna *taken, const uint64_t *dev, uint64_t n, uint64_t n_out)
{
    if (!ts_grow(t, n_out))
        return false;
    if (!gpu_ok(dnagpu_buffer_download(g_ctx, dev, n_out * 8, t->seq + t->n_pass)) ||
        !gpu_ok(dnagpu_buffer_download(g_ctx, dev + n, n_out * 8, t->rows + t->n_pass)) ||
        !gpu_ok(dnagpu_buffer_download(g_ctx, dev + 2 * n, n_out * 8, t->hits + t->n_pass)) ||
        !table_rows(taken, n_out, t->out + t->n_pass))
        return false;
    for (uint64_t i = 0; i < n_out; i++)
        t->seq[t->n_pass++] += t->n_added;                                /* the ordinal of the add call */
    return true;
}

/* the open batch: screened on the device, its passing rows appended, emptied */
static bool ts_flush(void *self)
{
    TableScreen *t = (TableScreen *)self;
    const uint64_t n = t->b.n_seqs;
    if (n == 0)
        return true;
    bool ok = true;
    if (t->b.n_bases == 0) {                                              /* empty rows only: no row, no hit, nothing to upload */
        if (t->min_hits == 0) {                                           /* (0 * den >= num * 0: the fraction asks nothing of them) */
            ok = ts_grow(t, n);
            for (uint64_t i = 0; ok && i < n; i++) {
                Dna *row = dna_cut(t->b.words, 0, 0);
                if (!row) {
                    ok = false;
                    break;
                }
                t->seq[t->n_pass] = t->n_added + i;
                t->rows[t->n_pass] = t->hits[t->n_pass] = 0;
                t->out[t->n_pass++] = row;
            }
        }
    } else {
        dnagpu_dna *d = NULL, *taken = NULL;
        dnagpu_seq_hits *h = NULL;
        void *dev = NULL;
        uint64_t n_out = 0;
        ok = batch_upload(&t->b, &d) &&
             gpu_ok(dnagpu_table_hits(g_ctx, d, t->set, t->flags, t->min_count, t->max_count, 0, n, &h)) &&
             gpu_ok(dnagpu_buffer_alloc(g_ctx, 3 * 8 * n, &dev));
        uint64_t *dv = (uint64_t *)dev;
        ok = ok && gpu_ok(dnagpu_seq_hits_select(g_ctx, h, t->min_hits, t->max_hits, t->frac_num, t->frac_den, dv, dv + n, dv + 2 * n,
                                                 n, &n_out, 1));
        if (ok && n_out > 0)
            ok = gpu_ok(dnagpu_dna_take(g_ctx, d, dv, NULL, n_out, 1, &taken)) && ts_collect(t, taken, dv, n, n_out);
        if (taken)
            dnagpu_dna_free(g_ctx, taken);
        if (dev)
            dnagpu_buffer_free(g_ctx, dev);
        if (h)
            dnagpu_seq_hits_free(g_ctx, h);
        if (d)
            dnagpu_dna_free(g_ctx, d);
    }
    t->n_added += n;
    rb_clear(&t->b);
    return ok;
}

bool table_screen_add(TableScreen *t, const Dna *row)
{
    if (t->started || t->failed) {
        ereport_error("table_screen: row added after the first row was served or the scan failed");
        return false;
    }
    if (!batch_add(&t->b, row, ts_flush, t))
        t->failed = true;
    return !t->failed;
}

bool table_screen_next(TableScreen *t, int64_t *seq, int64_t *rows, int64_t *hits, Dna **row)
{
    if (t->failed)
        return false;
    if (!t->started) {
        t->started = true;
        if (!ts_flush(t)) {                                               /* the last batch */
            t->failed = true;
            return false;
        }
    }
    if (t->next >= t->n_pass)
        return false;
    const uint64_t i = t->next++;
    if (seq)
        *seq = (int64_t)t->seq[i];
    if (rows)
        *rows = (int64_t)t->rows[i];
    if (hits)
        *hits = (int64_t)t->hits[i];
    if (row) {
        *row = t->out[i];                                                 /* the caller's from here on */
        t->out[i] = NULL;
    }
    return true;
}

bool table_screen_failed(const TableScreen *t) { return t->failed; }

void table_screen_end(TableScreen *t)
{
    if (!t)
        return;
    for (uint64_t i = 0; i < t->n_pass; i++)
        dna_free(t->out[i]);
    rb_free(&t->b);
    free(t->seq);
    free(t->rows);
    free(t->hits);
    free(t->out);
    free(t);
}

/* ------------------------------------------------------------------ COPY ... FROM a text file: copy_dna */

static uint64_t g_copy_chunk_bytes = (uint64_t)64 << 20;

void dna_glue_set_copy_chunk_bytes(uint64_t n) { g_copy_chunk_bytes = n ? n : 1; }

#define COPY_MAX_CHUNK ((uint64_t)UINT32_MAX)    /* dnagpu_table_from_text's limit for one call */

struct CopyDna {
    int format;
    bool failed, finished;
    char *buf;                                   /* the bytes fed and not yet accounted for by a load */
    uint64_t len, cap, chunk;
    Dna **rows;                                  /* the rows loaded and not yet served (NULL once handed out) */
    uint64_t cap_rows, n_rows, next;
    uint64_t first_line;                         /* rows of the whole file before rows[0] */
    int64_t bad_line;                            /* after an input ERROR: the 1-based row of the whole file it belongs to, else 0 */
    /* copy_reads_begin: the load goes through dnagpu_reads_from_text, and every row knows where it came from */
    bool reads;
    int ambiguous;
    unsigned flags;
    uint64_t min_bases;
    uint64_t *src_record, *src_offset;           /* per row of rows[]: the source record of the whole file, the offset in it */
    uint64_t cap_src_record, cap_src_offset;
    uint64_t first_record;                       /* source records of the whole file before the buffer's first byte */
    /* trim_reads_begin: FASTQ with its qualities, trimmed and filtered on the device; every row has its quality text */
    bool trim;
    dnagpu_quals_trim_options trim_opt;
    char **qual;                                 /* per row of rows[]: malloc'd, NUL-terminated (NULL once handed out) */
    uint64_t cap_qual;
};

CopyDna *copy_dna_begin(int format)
{
    if (format != DNAGPU_TEXT_LINES && format != DNAGPU_TEXT_FASTA) {
        ereport_error("copy_dna: the format must be 1 (one sequence per line) or 2 (FASTA)");
        return NULL;
    }
    CopyDna *c = (CopyDna *)calloc(1, sizeof *c);
    if (!c) {
        ereport_error("out of memory");
        return NULL;
    }
    c->format = format;
    c->chunk = g_copy_chunk_bytes < COPY_MAX_CHUNK ? g_copy_chunk_bytes : COPY_MAX_CHUNK;
    return c;
}

CopyDna *copy_reads_begin(int format, int ambiguous, unsigned flags, uint64_t min_bases)
{
    if (format != DNAGPU_TEXT_LINES && format != DNAGPU_TEXT_FASTA && format != DNAGPU_TEXT_FASTQ) {
        ereport_error("copy_reads: the format must be 1 (one sequence per line), 2 (FASTA) or 3 (FASTQ)");
        return NULL;
    }
    if (ambiguous < DNAGPU_AMBIG_ERROR || ambiguous > DNAGPU_AMBIG_SPLIT || (flags & ~DNAGPU_READS_FOLD_CASE)) {
        ereport_error("copy_reads: the ambiguity policy must be 0, 1 or 2 and the flags 0 or DNAGPU_READS_FOLD_CASE");
        return NULL;
    }
    CopyDna *c = copy_dna_begin(format == DNAGPU_TEXT_FASTQ ? DNAGPU_TEXT_LINES : format);
    if (!c)
        return NULL;
    c->format = format;
    c->reads = true;
    c->ambiguous = ambiguous;
    c->flags = flags;
    c->min_bases = min_bases;
    return c;
}

CopyDna *trim_reads_begin(int ambiguous, unsigned flags, uint32_t cut_front, uint32_t cut_tail, uint64_t min_bases, uint32_t min_mean_q,
                          uint32_t low_q, uint32_t low_num, uint32_t low_den)
{
    if (cut_front > 255 || cut_tail > 255 || min_mean_q > 255 || low_q > 255) {
        ereport_error("trim_reads: cut_front, cut_tail, min_mean_q and low_q must be at most 255");
        return NULL;
    }
    CopyDna *c = copy_reads_begin(DNAGPU_TEXT_FASTQ, ambiguous, flags, 0);
    if (!c)
        return NULL;
    c->trim = true;
    const dnagpu_quals_trim_options o = {cut_front, cut_tail, min_mean_q, low_q, low_num, low_den, min_bases, 0};
    c->trim_opt = o;
    return c;
}

/* trim_reads: the table d that the loader made of the first text_bytes bytes of the buffer (rec / off: its source map, n_seqs
 * entries) with its qualities, trimmed and filtered on the device: the passing reads appended as rows with their source
 * record, the offset of their first kept base in it, and their quality text.  *appended = how many. */
static bool trim_load(CopyDna *c, const dnagpu_dna *d, uint64_t text_bytes, const uint64_t *rec, const uint64_t *off, uint64_t n_seqs,
                      uint64_t *appended)
{
    dnagpu_quals *q = NULL, *tq = NULL;
    dnagpu_dna *td = NULL;
    dnagpu_quals_report qrep;
    dnagpu_quals_trim_report trep;
    uint64_t *seg = NULL, *starts = NULL;
    char *text = NULL;
    bool ok = false;
    *appended = 0;
    const int rc = dnagpu_quals_from_fastq(g_ctx, c->buf, text_bytes, 0, d, n_seqs ? rec : NULL, n_seqs ? off : NULL, &q, &qrep);
    if (rc != DNAGPU_OK) {
        if (qrep.bad_pos != UINT64_MAX) {                                 /* an input error: the library's message verbatim */
            ereport_error("%s", dnagpu_last_error());
            c->bad_line = qrep.bad_record == UINT64_MAX ? 0 : (int64_t)(c->first_record + qrep.bad_record + 1);
            return false;
        }
        return gpu_ok(rc);
    }
    if (n_seqs == 0) {
        dnagpu_quals_free(g_ctx, q);
        return true;
    }
    seg = (uint64_t *)malloc(sizeof(uint64_t) * 3 * (size_t)n_seqs);
    starts = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n_seqs + 1));
    if (!seg || !starts) {
        ereport_error("out of memory");
        goto done;
    }
    uint64_t *seg_seq = seg, *seg_first = seg + n_seqs, *seg_len = seg + 2 * n_seqs;
    if (!gpu_ok(dnagpu_quals_trim(g_ctx, d, q, &c->trim_opt, NULL, NULL, NULL, NULL, seg_seq, seg_first, seg_len, n_seqs, 0, &trep)) ||
        !gpu_ok(dnagpu_dna_sequence_starts(g_ctx, d, 0, n_seqs + 1, starts, 0)))
        goto done;
    const uint64_t m = trep.passed;
    if (m == 0) {
        ok = true;
        goto done;
    }
    if (!gpu_ok(dnagpu_dna_gather(g_ctx, d, seg_first, seg_len, NULL, m, 0, &td)) ||
        !gpu_ok(dnagpu_quals_gather(g_ctx, q, seg_first, seg_len, NULL, m, 0, &tq)))
        goto done;
    const uint64_t kept = dnagpu_quals_bases(tq);
    text = (char *)malloc((size_t)kept + 1);
    if (!text) {
        ereport_error("out of memory");
        goto done;
    }
    if (!gpu_ok(dnagpu_quals_read(g_ctx, tq, 0, kept, text, 0)) ||
        !agg_grow((void **)&c->rows, &c->cap_rows, c->n_rows + m) || !agg_grow((void **)&c->qual, &c->cap_qual, c->n_rows + m) ||
        !agg_grow((void **)&c->src_record, &c->cap_src_record, c->n_rows + m) ||
        !agg_grow((void **)&c->src_offset, &c->cap_src_offset, c->n_rows + m) || !table_rows(td, m, c->rows + c->n_rows))
        goto done;
    uint64_t at = 0;
    for (uint64_t i = 0; i < m; i++)
        c->qual[c->n_rows + i] = NULL;
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t s = seg_seq[i], len = seg_len[i];
        char *t = (char *)malloc((size_t)len + 1);
        if (!t) {
            ereport_error("out of memory");
            for (uint64_t j = 0; j < m; j++) {                            /* the rows of this load are not kept */
                dna_free(c->rows[c->n_rows + j]);
                free(c->qual[c->n_rows + j]);
            }
            goto done;
        }
        memcpy(t, text + at, (size_t)len);
        t[len] = 0;
        at += len;
        c->qual[c->n_rows + i] = t;
        c->src_record[c->n_rows + i] = c->first_record + rec[s];
        c->src_offset[c->n_rows + i] = off[s] + (seg_first[i] - starts[s]);
    }
    *appended = m;
    ok = true;
done:
    free(text);
    free(seg);
    free(starts);
    if (td)
        dnagpu_dna_free(g_ctx, td);
    if (tq)
        dnagpu_quals_free(g_ctx, tq);
    dnagpu_quals_free(g_ctx, q);
    return ok;
}

/* copy_load for copy_reads_begin: the same chunk through dnagpu_reads_from_text.  The source arrays are sized for reads of
 * 32 bytes and more; a chunk of shorter ones is loaded a second time with the size its report names */
static bool copy_load_reads(CopyDna *c, uint64_t n, bool more)
{
    const dnagpu_reads_options opt = {c->format, c->ambiguous, c->flags | (more ? DNAGPU_READS_MORE : 0u), 0u, c->min_bases};
    dnagpu_dna *d = NULL;
    dnagpu_reads_report rep;
    uint64_t cap = n / 32 + 1024, *rec = NULL, *off = NULL;
    for (;;) {
        rec = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)cap);
        off = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)cap);
        if (!rec || !off) {
            free(rec);
            free(off);
            ereport_error("out of memory");
            return false;
        }
        const int rc = dnagpu_reads_from_text(g_ctx, c->buf, n, 0, &opt, &d, NULL, 0, rec, off, cap, &rep);
        if (rc != DNAGPU_OK) {
            free(rec);
            free(off);
            if (rep.bad_pos != UINT64_MAX) {                              /* an input error: the library's message verbatim */
                ereport_error("%s", dnagpu_last_error());
                c->bad_line = rep.bad_record == UINT64_MAX ? 0 : (int64_t)(c->first_record + rep.bad_record + 1);
                return false;
            }
            return gpu_ok(rc);
        }
        if (rep.sequences <= cap)
            break;
        dnagpu_dna_free(g_ctx, d);
        free(rec);
        free(off);
        cap = rep.sequences;
    }
    if (c->next == c->n_rows)                                             /* everything served: the arrays start over */
        c->n_rows = c->next = 0;
    uint64_t added = rep.sequences;
    bool ok;
    if (c->trim) {                                                        /* the qualities of the same bytes, then the trim */
        ok = trim_load(c, d, more ? rep.consumed : n, rec, off, rep.sequences, &added);
    } else {
        ok = agg_grow((void **)&c->rows, &c->cap_rows, c->n_rows + rep.sequences) &&
             agg_grow((void **)&c->src_record, &c->cap_src_record, c->n_rows + rep.sequences) &&
             agg_grow((void **)&c->src_offset, &c->cap_src_offset, c->n_rows + rep.sequences) &&
             (rep.sequences == 0 || table_rows(d, rep.sequences, c->rows + c->n_rows));
        for (uint64_t i = 0; ok && i < rep.sequences; i++) {
            c->src_record[c->n_rows + i] = c->first_record + rec[i];
            c->src_offset[c->n_rows + i] = off[i];
        }
    }
    dnagpu_dna_free(g_ctx, d);
    free(rec);
    free(off);
    if (!ok)
        return false;
    c->n_rows += added;
    c->first_record += rep.records;
    if (rep.consumed && c->len > rep.consumed)
        memmove(c->buf, c->buf + rep.consumed, (size_t)(c->len - rep.consumed));
    c->len -= rep.consumed;
    if (more && rep.consumed == 0) {                                      /* a record longer than the chunk */
        if (c->chunk >= COPY_MAX_CHUNK) {
            ereport_error("copy_reads: a record is longer than 2^32 - 1 bytes");
            return false;
        }
        c->chunk = c->chunk > COPY_MAX_CHUNK / 2 ? COPY_MAX_CHUNK : 2 * c->chunk;
    }
    return true;
}

/* the first n bytes of the buffer through dnagpu_table_from_text; the rows appended, the bytes accounted for dropped */
static bool copy_load(CopyDna *c, uint64_t n, bool more)
{
    dnagpu_dna *d = NULL;
    dnagpu_text_report rep;
    if (!ctx())
        return false;
    if (c->reads)
        return copy_load_reads(c, n, more);
    const int rc = dnagpu_table_from_text(g_ctx, c->buf, n, 0, c->format, more ? DNAGPU_TEXT_MORE : 0u, &d, NULL, 0, &rep);
    if (rc != DNAGPU_OK) {
        if (rep.bad_pos != UINT64_MAX) {                                  /* an input error: the reference's message verbatim */
            ereport_error("%s", dnagpu_last_error());
            c->bad_line = rep.bad_record == UINT64_MAX ? 0 : (int64_t)(c->first_line + c->n_rows + rep.bad_record + 1);
            return false;
        }
        return gpu_ok(rc);
    }
    if (c->next == c->n_rows) {                                           /* everything served: the array starts over */
        c->first_line += c->n_rows;
        c->n_rows = c->next = 0;
    }
    bool ok = agg_grow((void **)&c->rows, &c->cap_rows, c->n_rows + rep.records) &&
              (rep.records == 0 || table_rows(d, rep.records, c->rows + c->n_rows));
    dnagpu_dna_free(g_ctx, d);
    if (!ok)
        return false;
    c->n_rows += rep.records;
    if (rep.consumed && c->len > rep.consumed)
        memmove(c->buf, c->buf + rep.consumed, (size_t)(c->len - rep.consumed));
    c->len -= rep.consumed;
    if (more && rep.consumed == 0) {                                      /* a record longer than the chunk */
        if (c->chunk >= COPY_MAX_CHUNK) {
            ereport_error("copy_dna: a record is longer than 2^32 - 1 bytes");
            return false;
        }
        c->chunk = c->chunk > COPY_MAX_CHUNK / 2 ? COPY_MAX_CHUNK : 2 * c->chunk;
    }
    return true;
}

bool copy_dna_feed(CopyDna *c, const char *bytes, size_t n, bool last)
{
    if (c->failed || c->finished) {
        ereport_error("copy_dna: bytes fed after the last ones or after the load failed");
        return false;
    }
    if (n && !bytes) {
        ereport_error("copy_dna: the bytes are missing");
        return false;
    }
    if (c->len + n > c->cap) {
        uint64_t cap = c->cap ? c->cap : 4096;
        while (cap < c->len + n)
            cap *= 2;
        char *grown = (char *)realloc(c->buf, (size_t)cap);
        if (!grown) {
            ereport_error("out of memory");
            c->failed = true;
            return false;
        }
        c->buf = grown;
        c->cap = cap;
    }
    if (n)
        memcpy(c->buf + c->len, bytes, n);
    c->len += n;
    while (!c->failed && c->len >= c->chunk)
        c->failed = !copy_load(c, c->chunk, true);
    if (!c->failed && last) {
        c->failed = !copy_load(c, c->len, false);
        c->finished = true;
    }
    return !c->failed;
}

bool copy_dna_next(CopyDna *c, Dna **row, int64_t *line)
{
    if (c->failed) {
        if (line)
            *line = c->bad_line;
        return false;
    }
    if (c->next >= c->n_rows)
        return false;
    const uint64_t i = c->next++;
    if (line)
        *line = (int64_t)(c->first_line + i + 1);
    if (row) {
        *row = c->rows[i];                                                /* the caller's from here on */
        c->rows[i] = NULL;
    }
    return true;
}

bool copy_reads_next(CopyDna *c, Dna **row, int64_t *record, int64_t *offset)
{
    if (c->failed || !c->reads) {
        if (record)
            *record = c->bad_line - 1;
        return false;
    }
    if (c->next >= c->n_rows)
        return false;
    const uint64_t i = c->next;
    if (record)
        *record = (int64_t)c->src_record[i];
    if (offset)
        *offset = (int64_t)c->src_offset[i];
    return copy_dna_next(c, row, NULL);
}

bool trim_reads_next(CopyDna *c, Dna **row, int64_t *record, int64_t *offset, char **quality)
{
    if (c->failed || !c->trim) {
        if (record)
            *record = c->bad_line - 1;
        return false;
    }
    if (c->next >= c->n_rows)
        return false;
    const uint64_t i = c->next;
    if (quality)
        *quality = c->qual[i];                                            /* the caller's from here on (free) */
    else
        free(c->qual[i]);
    c->qual[i] = NULL;
    return copy_reads_next(c, row, record, offset);
}

bool copy_dna_failed(const CopyDna *c) { return c->failed; }

void copy_dna_end(CopyDna *c)
{
    if (!c)
        return;
    for (uint64_t i = 0; c->qual && i < c->n_rows; i++)
        free(c->qual[i]);
    free(c->qual);
    for (uint64_t i = 0; i < c->n_rows; i++)
        dna_free(c->rows[i]);
    free(c->rows);
    free(c->src_record);
    free(c->src_offset);
    free(c->buf);
    free(c);
}

/* ------------------------------------------------------------------ COPY ... TO a text file: copy_dna_to */

struct CopyDnaTo {
    int format;
    uint32_t line_width;
    bool crlf, failed, finished;
    RowBatch b;                                  /* the open batch */
    uint64_t limit_bases, chunk;                 /* a batch is flushed at limit_bases; a chunk of text has at most `chunk` bytes */
    uint64_t rows_before;                        /* rows of the flushed batches: the first name of the next one */
    char **text;                                 /* the chunks of text formed and not yet served (NULL once served and freed) */
    uint64_t *text_len;
    uint64_t cap_text, cap_text_len, n_text, next;
    /* copy_reads_to_begin: FASTQ whose quality lines are the rows' own */
    bool reads;
    char *qual;                                  /* the quality bytes of the open batch, one per base */
    uint64_t cap_qual;
};

CopyDnaTo *copy_dna_to_begin(int format, uint32_t line_width, bool crlf)
{
    if (format != DNAGPU_TEXT_LINES && format != DNAGPU_TEXT_FASTA && format != DNAGPU_TEXT_FASTQ) {
        ereport_error("copy_dna_to: the format must be 1 (one sequence per line), 2 (FASTA) or 3 (FASTQ)");
        return NULL;
    }
    if (line_width && format != DNAGPU_TEXT_FASTA) {
        ereport_error("copy_dna_to: only FASTA (format 2) takes a line width");
        return NULL;
    }
    CopyDnaTo *c = (CopyDnaTo *)calloc(1, sizeof *c);
    if (!c) {
        ereport_error("out of memory");
        return NULL;
    }
    c->format = format;
    c->line_width = line_width;
    c->crlf = crlf;
    c->chunk = g_copy_chunk_bytes < COPY_MAX_CHUNK ? g_copy_chunk_bytes : COPY_MAX_CHUNK;
    c->limit_bases = c->chunk < ((uint64_t)1 << 30) ? 4 * c->chunk : COPY_MAX_CHUNK;      /* (packed: four bases per byte) */
    return c;
}

/* the image of the batch's table, chunk after chunk, behind the chunks that wait */
static bool copy_to_read(CopyDnaTo *c, const dnagpu_text_image *img, const dnagpu_quals *quals)
{
    const uint64_t bytes = dnagpu_text_image_bytes(img);
    for (uint64_t at = 0; at < bytes; at += c->chunk) {
        const uint64_t n = bytes - at < c->chunk ? bytes - at : c->chunk;
        if (!agg_grow((void **)&c->text, &c->cap_text, c->n_text + 1) ||
            !agg_grow((void **)&c->text_len, &c->cap_text_len, c->n_text + 1))
            return false;
        char *t = (char *)malloc((size_t)n);
        if (!t) {
            ereport_error("out of memory");
            return false;
        }
        c->text[c->n_text] = t;
        c->text_len[c->n_text++] = n;
        if (!gpu_ok(quals ? dnagpu_text_image_read_quals(g_ctx, img, quals, at, n, t, 0) : dnagpu_text_image_read(g_ctx, img, at, n, t, 0)))
            return false;
    }
    return true;
}

/* the batch so far: made resident, written out, emptied */
static bool copy_to_flush(void *self)
{
    CopyDnaTo *c = (CopyDnaTo *)self;
    bool ok = true;
    if (c->b.n_seqs > 0) {
        const dnagpu_text_out_options opt = {c->format, c->crlf ? DNAGPU_TEXT_OUT_CRLF : 0u, c->line_width, 0, NULL, c->rows_before,
                                             NULL, 0, 0, {0, 0, 0}};
        dnagpu_dna *d = NULL;
        dnagpu_text_image *img = NULL;
        dnagpu_quals *q = NULL;
        ok = batch_upload(&c->b, &d);
        if (ok && c->reads) {
            dnagpu_quals_report qrep;
            const int rc = dnagpu_quals_upload(g_ctx, c->qual, c->b.n_bases, 0, &q, &qrep);
            if (rc != DNAGPU_OK && qrep.bad_pos != UINT64_MAX) {          /* the library's message verbatim */
                ereport_error("%s", dnagpu_last_error());
                ok = false;
            } else {
                ok = gpu_ok(rc);
            }
        }
        ok = ok && gpu_ok(dnagpu_table_to_text(g_ctx, d, &opt, &img)) && copy_to_read(c, img, q);
        if (img)
            dnagpu_text_image_free(g_ctx, img);
        if (q)
            dnagpu_quals_free(g_ctx, q);
        if (d)
            dnagpu_dna_free(g_ctx, d);
        c->rows_before += c->b.n_seqs;
    }
    rb_clear(&c->b);
    return ok;
}

bool copy_dna_to_add(CopyDnaTo *c, const Dna *row)
{
    if (c->finished || c->failed) {
        ereport_error("copy_dna_to: a row added after the last one or after the COPY failed");
        return false;
    }
    if (!row) {
        ereport_error("copy_dna_to: the row is missing");
        return false;
    }
    if (rb_spills(&c->b, row->length, c->limit_bases) && !copy_to_flush(c))
        return !(c->failed = true);
    if (!rb_append(&c->b, row->bit_sequence, row->length)) {
        ereport_error("out of memory");
        return !(c->failed = true);
    }
    if (rb_full(&c->b, c->limit_bases) && !copy_to_flush(c))
        return !(c->failed = true);
    return true;
}

CopyDnaTo *copy_reads_to_begin(bool crlf)
{
    CopyDnaTo *c = copy_dna_to_begin(DNAGPU_TEXT_FASTQ, 0, crlf);
    if (c)
        c->reads = true;
    return c;
}

bool copy_reads_to_add(CopyDnaTo *c, const Dna *row, const char *quality, size_t quality_len)
{
    if (c->finished || c->failed || !c->reads) {
        ereport_error("copy_reads_to: a row added after the last one or after the COPY failed");
        return false;
    }
    if (!row || (quality_len && !quality)) {
        ereport_error("copy_reads_to: the row or its quality text is missing");
        return false;
    }
    if ((uint64_t)quality_len != row->length) {
        ereport_error("FASTQ quality line length differs from the sequence's");
        return !(c->failed = true);
    }
    if (rb_spills(&c->b, row->length, c->limit_bases) && !copy_to_flush(c))
        return !(c->failed = true);
    if (!rb_grow((void **)&c->qual, &c->cap_qual, c->b.n_bases + row->length + 1) || !rb_append(&c->b, row->bit_sequence, row->length)) {
        ereport_error("out of memory");
        return !(c->failed = true);
    }
    if (quality_len)
        memcpy(c->qual + c->b.n_bases - row->length, quality, quality_len);
    if (rb_full(&c->b, c->limit_bases) && !copy_to_flush(c))
        return !(c->failed = true);
    return true;
}

bool copy_reads_to_finish(CopyDnaTo *c) { return copy_dna_to_finish(c); }
bool copy_reads_to_next(CopyDnaTo *c, const char **bytes, size_t *n) { return copy_dna_to_next(c, bytes, n); }
bool copy_reads_to_failed(const CopyDnaTo *c) { return copy_dna_to_failed(c); }
void copy_reads_to_end(CopyDnaTo *c) { copy_dna_to_end(c); }

bool copy_dna_to_finish(CopyDnaTo *c)
{
    if (c->failed)
        return false;
    if (!c->finished && !copy_to_flush(c))
        return !(c->failed = true);
    c->finished = true;
    return true;
}

bool copy_dna_to_next(CopyDnaTo *c, const char **bytes, size_t *n)
{
    if (c->failed || c->next >= c->n_text)
        return false;
    if (c->next > 0) {                                                        /* the chunk served before this one */
        free(c->text[c->next - 1]);
        c->text[c->next - 1] = NULL;
    }
    const uint64_t i = c->next++;
    if (bytes)
        *bytes = c->text[i];
    if (n)
        *n = (size_t)c->text_len[i];
    return true;
}

bool copy_dna_to_failed(const CopyDnaTo *c) { return c->failed; }

void copy_dna_to_end(CopyDnaTo *c)
{
    if (!c)
        return;
    for (uint64_t i = 0; i < c->n_text; i++)
        free(c->text[i]);
    free(c->text);
    free(c->text_len);
    free(c->qual);
    rb_free(&c->b);
    free(c);
}

/* ------------------------------------------------------------------ the index over a stored kmer column */

struct KmerIndex {
    dnagpu_kmer_index *idx;
    int k;
};

KmerIndex *kmer_index_create(const Kmer *column, uint64_t n)
{
    int k = n ? column[0].length : 1;                /* (an empty column: any length does, no scan finds a row) */
    for (uint64_t i = 1; i < n; i++)
        if (column[i].length != k) {
            ereport_error("kmer_index_create: the column holds kmers of %d and %d bases; an index covers one length", k,
                          (int)column[i].length);
            return NULL;
        }
    KmerIndex *x = (KmerIndex *)calloc(1, sizeof *x);
    uint64_t *keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n ? n : 1));
    if (!x || !keys) {
        free(x);
        free(keys);
        ereport_error("out of memory");
        return NULL;
    }
    for (uint64_t i = 0; i < n; i++)
        keys[i] = column[i].bit_sequence;
    x->k = k;
    const bool ok = ctx() && gpu_ok(dnagpu_kmer_index_build(g_ctx, keys, n, k, 0, &x->idx));    /* a bad length: dna.c:773 */
    free(keys);
    if (!ok) {
        free(x);
        return NULL;
    }
    return x;
}

uint64_t kmer_index_rows(const KmerIndex *idx)
{
    return idx ? dnagpu_kmer_index_rows(idx->idx) : 0;
}

int64_t kmer_index_insert(KmerIndex *idx, const Kmer *rows, uint64_t n)
{
    if (!ctx())
        return -1;
    const int64_t first = (int64_t)dnagpu_kmer_index_next_row(idx->idx);
    if (n == 0)
        return first;
    int k = idx->k;
    if (first == 0)                                  /* created over an empty column: the first rows decide the length */
        k = rows[0].length;
    for (uint64_t i = 0; i < n; i++)
        if (rows[i].length != k) {
            ereport_error("kmer_index_create: the column holds kmers of %d and %d bases; an index covers one length", k,
                          (int)rows[i].length);
            return -1;
        }
    if (k != idx->k) {
        dnagpu_kmer_index *empty = NULL;
        if (!gpu_ok(dnagpu_kmer_index_build(g_ctx, NULL, 0, k, 0, &empty)))     /* a bad length: dna.c:773 */
            return -1;
        dnagpu_kmer_index_free(g_ctx, idx->idx);
        idx->idx = empty;
        idx->k = k;
    }
    uint64_t *keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n);
    if (!keys) {
        ereport_error("out of memory");
        return -1;
    }
    for (uint64_t i = 0; i < n; i++)
        keys[i] = rows[i].bit_sequence;
    const bool ok = gpu_ok(dnagpu_kmer_index_append(g_ctx, idx->idx, keys, n, 0));
    free(keys);
    return ok ? first : -1;
}

int64_t kmer_index_delete(KmerIndex *idx, const int64_t *rows, uint64_t n)
{
    if (!ctx())
        return -1;
    uint64_t gone = 0;                               /* a negative id reads as one above 2^32 - 1: ignored */
    if (!gpu_ok(dnagpu_kmer_index_delete(g_ctx, idx->idx, (const uint64_t *)rows, n, 0, &gone)))
        return -1;
    return (int64_t)gone;
}

static int cmp_i64(const void *a, const void *b)
{
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return (x > y) - (x < y);
}

/* the rows of one index scan, sorted into heap order */
static int64_t index_scan(KmerIndex *x, const dnagpu_filter *f, int64_t **rows)
{
    *rows = NULL;
    uint64_t n = 0;
    if (!ctx() || !gpu_ok(dnagpu_kmer_index_scan(g_ctx, x->idx, f, NULL, NULL, 0, &n, NULL, 0)))
        return -1;
    if (n == 0)
        return 0;
    int64_t *out = (int64_t *)malloc(sizeof(int64_t) * (size_t)n);
    if (!out) {
        ereport_error("out of memory");
        return -1;
    }
    uint64_t got = 0;
    if (!gpu_ok(dnagpu_kmer_index_scan(g_ctx, x->idx, f, (uint64_t *)out, NULL, n, &got, NULL, 0)) || got != n) {
        free(out);
        return -1;
    }
    qsort(out, (size_t)n, sizeof *out, cmp_i64);     /* row ids are < 2^32: the same order signed or unsigned */
    *rows = out;
    return (int64_t)n;
}

static int64_t index_scan_kmer(KmerIndex *x, int kind, const Kmer *rhs, int64_t **rows)
{
    dnagpu_filter f;
    memset(&f, 0, sizeof f);
    f.kind = kind;
    f.length = rhs->length;
    f.bits = rhs->bit_sequence;
    return index_scan(x, &f, rows);
}

int64_t kmer_index_scan_eq(KmerIndex *idx, const Kmer *rhs, int64_t **rows)
{
    return index_scan_kmer(idx, DNAGPU_FILTER_EQUALS, rhs, rows);
}

int64_t kmer_index_scan_starts_with(KmerIndex *idx, const Kmer *prefix, int64_t **rows)
{
    return index_scan_kmer(idx, DNAGPU_FILTER_STARTS_WITH, prefix, rows);
}

int64_t kmer_index_scan_contains(KmerIndex *idx, const Qkmer *pattern, int64_t **rows)
{
    dnagpu_filter f;
    memset(&f, 0, sizeof f);
    f.kind = DNAGPU_FILTER_CONTAINS;
    strncpy(f.pattern, pattern->sequence, sizeof f.pattern - 1);
    return index_scan(idx, &f, rows);
}

void kmer_index_end(KmerIndex *idx)
{
    if (!idx)
        return;
    if (g_ctx)
        dnagpu_kmer_index_free(g_ctx, idx->idx);
    free(idx);
}
