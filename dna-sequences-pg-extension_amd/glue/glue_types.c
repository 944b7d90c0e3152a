/*
 * glue_types.c -- the types dna, kmer and qkmer: text and binary I/O and the per-datum operators, all on the host.  Written
 * against the behaviour of the reference's dna.c (cited per function); PostgreSQL plumbing replaced by plain C.
 */
#include "glue_core.h"

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
    Dna *dna = dna_new(length);
    if (!dna)
        return NULL;
    for (uint64_t i = 0; i < length; i++) {                               /* dna.c:115-127 */
        uint64_t code = str[i] == 'A' ? 0 : str[i] == 'T' ? 1 : str[i] == 'C' ? 2 : 3;
        dna->bit_sequence[i / 32] |= code << ((i * 2) % 64);
    }
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
    Dna *dna = dna_new(length);                                           /* palloc0, dna.c:257 */
    if (!dna)
        return NULL;
    uint64_t *w = dna->bit_sequence;
    for (uint64_t i = 0; i < bit_length; i++)                             /* dna.c:263-265 */
        w[i] = get_be64(wire + 8 + 8 * i);
    if (length % 32)
        w[bit_length - 1] &= (((uint64_t)1 << (2 * (length % 32))) - 1);  /* keep the tail bits zero (dna.c:186) */
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
    Dna *out = dna_new(dna->length);
    if (!out)
        return NULL;
    for (uint64_t j = 0; j < dna->length; j++) {
        uint64_t i = dna->length - 1 - j;
        uint64_t code = ((dna->bit_sequence[i / 32] >> ((i * 2) % 64)) & 3) ^ 1;
        out->bit_sequence[j / 32] |= code << ((j * 2) % 64);
    }
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
