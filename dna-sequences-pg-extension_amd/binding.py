"""ctypes binding of include/dnagpu.h (libdnagpu.so).  One method per C entry point; numpy arrays
in and out; errors raise DnaGpuError carrying the status code and the reference's message text."""
import ctypes as C
import dataclasses
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

OK = 0
ERR_INVALID_K = 1
ERR_QKMER_LEN_MISMATCH = 2
ERR_PREFIX_TOO_LONG = 3
ERR_QKMER_INVALID = 4
ERR_BAD_ARG = 5
ERR_TOO_LARGE = 6
ERR_NO_DEVICE = 7
ERR_OOM = 8
ERR_HIP = 9
ERR_DNA_EMPTY = 11
ERR_DNA_INVALID_CHAR = 12
DEBUG_POISON_POOL = 1
DEBUG_FORCE_SUPERKMER = 2
DEBUG_HEAVY_EXPAND = 4
DEBUG_GUARD_POOL = 8
DEBUG_NO_SPEC1 = 16
DEBUG_SPEC1_OVERFLOW = 32
DEBUG_SLAB0 = 64
DEBUG_NO_SLAB0 = 128
DEBUG_SLAB0_OVERFLOW = 256
DEBUG_SAMPLE1 = 512                   # level 1: regions from a sampled histogram whatever the coarse buckets look like
DEBUG_RANK_SMALL = 1024               # rank: a class limit of 4 counts and sort chunks of 2048 rows (the tail path at small sizes)
DEBUG_JOIN_PARTITION = 2048           # dnagpu_acc_join: the partition path for any sizes
DEBUG_JOIN_DIRECT = 4096              # dnagpu_acc_join: the direct path for any sizes
DEBUG_WEAK_FINGERPRINT = 8192         # equal sequences: 2-bit fingerprints (several verify rounds, run walks in the match)
DEBUG_EARLY_L2 = 16384                # record count: level 2 behind its device-side gate after a level 1 with sampled regions too
MATCH_NONE = (1 << 64) - 1            # dnagpu_table_match: no sequence of the built table equals this one
JOIN_INNER = 0                        # JOIN .. ON a.kmer = b.kmer; INTERSECT
JOIN_ANTI = 1                         # EXCEPT; NOT IN; NOT EXISTS
JOIN_LEFT = 2                         # LEFT JOIN
HITS_CANONICAL = 1                    # dnagpu_table_hits: probe with the canonical form of the row's key
PROFILE_CANONICAL = 1                 # dnagpu_table_profile: count every row under its canonical form
PROFILE_MAX_K = 6
STRAND_REVCOMP = 0                  # dnagpu_kmer_strand: out = rc(key)
STRAND_CANONICAL = 1                  # ... out = whichever of key and rc(key) comes first under A < T < C < G
SPECTRUM_MAX_BINS = 1 << 20
TOP_MAX = 1 << 20
ORDER_COUNT_DESC = 0                  # ORDER BY count(*) DESC (test.sql:95)
ORDER_COUNT_ASC = 1                   # ORDER BY count(*): the rarest first
TEXT_LINES = 1                        # dnagpu_table_from_text: one sequence per line (COPY ... WITH (FORMAT text))
TEXT_FASTA = 2                        # ... '>' header lines open records
TEXT_MORE = 1                         # ... flags: a chunk of a longer file, the unfinished last record is held back
TEXT_FASTQ = 3                        # dnagpu_reads_from_text only: strict four-line records
TEXT_OUT_CRLF = 1                     # dnagpu_table_to_text: every terminator is "\r\n"
AMBIG_ERROR, AMBIG_DROP, AMBIG_SPLIT = 0, 1, 2      # dnagpu_reads_from_text: what an IUPAC ambiguity letter does
READS_MORE, READS_FOLD_CASE = 1, 2    # ... flags
U64_MAX = 2 ** 64 - 1


def _env_debug():
    """test-harness switches (this wrapper is test / bench tooling): DNAGPU_TEST_POISON=1 runs every context with
    DNAGPU_DEBUG_POISON_POOL (all work buffers pre-filled with 0xFF), DNAGPU_TEST_GUARD=1 with DNAGPU_DEBUG_GUARD_POOL
    (a guard band behind every work buffer, checked whenever a histogram, a sequence or a buffer is freed)"""
    f = 0
    if os.environ.get("DNAGPU_TEST_POISON", "0") not in ("", "0"):
        f |= DEBUG_POISON_POOL
    if os.environ.get("DNAGPU_TEST_GUARD", "0") not in ("", "0"):
        f |= DEBUG_GUARD_POOL
    return f

FILTER_EQUALS = 1
FILTER_STARTS_WITH = 2
FILTER_CONTAINS = 3

MAX_PHASES = 48

u64p = C.POINTER(C.c_uint64)


class _FilterC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("length", C.c_int32), ("bits", C.c_uint64),
                ("pattern", C.c_char * 36), ("reserved", C.c_int32)]


class JoinStats(C.Structure):
    """dnagpu_join_stats: the statistics of a join over all its result rows"""
    _fields_ = [(n, C.c_uint64) for n in ("rows", "sum_left", "sum_right", "sum_min", "checksum_left", "checksum_right")]

    def as_tuple(self):
        return tuple(int(getattr(self, n)) for n, _ in self._fields_)


class _TextReportC(C.Structure):
    _fields_ = [("records", C.c_uint64), ("bases", C.c_uint64), ("consumed", C.c_uint64), ("bad_pos", C.c_uint64),
                ("bad_record", C.c_uint64), ("bad_char", C.c_char), ("reserved", C.c_char * 7)]


@dataclasses.dataclass
class TextReport:
    """dnagpu_text_report.  bad_pos / bad_record are None where the C struct holds ~0, bad_char is b"" where it holds 0"""
    records: int
    bases: int
    consumed: int
    bad_pos: object = None
    bad_record: object = None
    bad_char: bytes = b""
    record_pos: object = None         # uint64[min(records, cap)] when asked for (host), else None


class _ReadsOptionsC(C.Structure):
    _fields_ = [("format", C.c_int), ("ambiguous", C.c_int), ("flags", C.c_uint), ("reserved", C.c_uint), ("min_bases", C.c_uint64)]


class _ReadsReportC(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("records", "sequences", "bases", "consumed", "ambiguous", "dropped", "short_out",
                                          "bad_pos", "bad_record")] + [("bad_char", C.c_char), ("reserved", C.c_char * 7)]


@dataclasses.dataclass
class ReadsReport:
    """dnagpu_reads_report.  bad_pos / bad_record are None where the C struct holds ~0, bad_char is b"" where it holds 0"""
    records: int
    sequences: int
    bases: int
    consumed: int
    ambiguous: int
    dropped: int
    short_out: int
    bad_pos: object = None
    bad_record: object = None
    bad_char: bytes = b""
    record_pos: object = None         # uint64[min(records, cap)] when asked for (host), else None
    src_record: object = None         # uint64[min(sequences, cap)] each when asked for (host), else None
    src_offset: object = None


class _QualsReportC(C.Structure):
    _fields_ = [("records", C.c_uint64), ("bad_pos", C.c_uint64), ("bad_record", C.c_uint64), ("bad_char", C.c_char),
                ("reserved", C.c_char * 7)]


@dataclasses.dataclass
class QualsReport:
    """dnagpu_quals_report.  bad_pos / bad_record are None where the C struct holds ~0, bad_char is b"" where it holds 0"""
    records: int = 0
    bad_pos: object = None
    bad_record: object = None
    bad_char: bytes = b""


class _NamesReportC(C.Structure):
    _fields_ = [("bad_pos", C.c_uint64), ("bad_record", C.c_uint64), ("bad_char", C.c_char), ("reserved", C.c_char * 7)]


@dataclasses.dataclass
class NamesReport:
    """dnagpu_names_report.  bad_pos / bad_record are None where the C struct holds ~0, bad_char is b"" where it holds 0"""
    bad_pos: object = None
    bad_record: object = None
    bad_char: bytes = b""


NAMES_FIRST_WORD = 1                  # dnagpu_names_from_text: a name ends before its first blank or tab


class _QualsTrimOptionsC(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("cut_front", "cut_tail", "min_mean_q", "low_q", "low_num", "low_den")] + \
               [("min_bases", C.c_uint64), ("reserved", C.c_uint64)]


_TRIM_REPORT_FIELDS = ("sequences", "passed", "bases_in", "bases_kept", "cut_front", "cut_tail", "failed_short", "failed_mean",
                       "failed_low")


class _QualsTrimReportC(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in _TRIM_REPORT_FIELDS]


@dataclasses.dataclass
class TrimResult:
    """what Context.quals_trim returns: the dnagpu_quals_trim_report's counters; first / length / qsum / low: uint64 per
    sequence; seg_seq / seg_first / seg_len: the passing sequences in table order, at most cap of them"""
    sequences: int = 0
    passed: int = 0
    bases_in: int = 0
    bases_kept: int = 0
    cut_front: int = 0
    cut_tail: int = 0
    failed_short: int = 0
    failed_mean: int = 0
    failed_low: int = 0
    first: object = None
    length: object = None
    qsum: object = None
    low: object = None
    seg_seq: object = None
    seg_first: object = None
    seg_len: object = None


ADAPTERS_DISCARD_UNTRIMMED = 1        # dnagpu_dna_adapters: the segments without a hit do not pass
ADAPTERS_DISCARD_TRIMMED = 2          # those with one do not
NO_ADAPTER = 2 ** 64 - 1              # out_adapter of a segment without a hit


class _AdaptersOptionsC(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("err_num", "err_den", "min_overlap", "flags")] + \
               [("min_bases", C.c_uint64), ("reserved", C.c_uint64)]


_ADAPTERS_REPORT_FIELDS = ("segments", "passed", "trimmed", "bases_in", "bases_kept", "bases_cut", "failed_short", "failed_discarded")


class _AdaptersReportC(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in _ADAPTERS_REPORT_FIELDS] + [("per_adapter", C.c_uint64 * 32)]


@dataclasses.dataclass
class AdaptersResult:
    """what Context.dna_adapters returns: the dnagpu_adapters_report's counters and per_adapter (32 counts); out_len /
    out_adapter / out_mismatch: uint64 per input segment; pass_seq / pass_first / pass_len: the passing segments in input
    order, at most cap of them"""
    segments: int = 0
    passed: int = 0
    trimmed: int = 0
    bases_in: int = 0
    bases_kept: int = 0
    bases_cut: int = 0
    failed_short: int = 0
    failed_discarded: int = 0
    per_adapter: object = None
    out_len: object = None
    out_adapter: object = None
    out_mismatch: object = None
    pass_seq: object = None
    pass_first: object = None
    pass_len: object = None


class _TextOutOptionsC(C.Structure):
    _fields_ = [("format", C.c_int), ("flags", C.c_uint), ("line_width", C.c_uint32), ("prefix_len", C.c_uint32),
                ("name_prefix", C.c_char_p), ("name_base", C.c_uint64), ("numbers", C.c_void_p), ("numbers_on_device", C.c_int),
                ("quality", C.c_char), ("reserved", C.c_char * 3)]


class _PhaseTimes(C.Structure):
    _fields_ = [("n", C.c_int), ("names", C.c_char_p * MAX_PHASES), ("ms", C.c_float * MAX_PHASES)]


class _MultiTimes(C.Structure):
    _fields_ = [("records_ms", C.c_double), ("exchange_ms", C.c_double), ("hidden_ms", C.c_double),
                ("count_ms", C.c_double), ("total_ms", C.c_double), ("bytes_moved", C.c_uint64), ("parts", C.c_int)]


def lib_path():
    # DNAGPU_LIB_PATH: A/B runs of two builds on one box (tools/ab.sh); this wrapper is test / bench tooling, the
    # library itself reads no environment variable
    return os.environ.get("DNAGPU_LIB_PATH") or os.path.join(_HERE, "libdnagpu.so")


def lib():
    """Loads libdnagpu.so; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.dnagpu_strerror.restype = C.c_char_p
    L.dnagpu_strerror.argtypes = [C.c_int]
    L.dnagpu_last_error.restype = C.c_char_p
    L.dnagpu_abi_version.restype = C.c_int
    L.dnagpu_init.argtypes = [C.c_int, C.POINTER(vp)]
    L.dnagpu_destroy.argtypes = [vp]
    L.dnagpu_destroy.restype = None
    L.dnagpu_synchronize.argtypes = [vp]
    L.dnagpu_stream.argtypes = [vp]
    L.dnagpu_stream.restype = vp
    L.dnagpu_trim.argtypes = [vp]
    L.dnagpu_device_bytes.argtypes = [vp]
    L.dnagpu_device_bytes.restype = C.c_uint64
    L.dnagpu_dna_upload.argtypes = [vp, u64p, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_dna_wrap.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_dna_synth.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_dna_download.argtypes = [vp, vp, u64p]
    L.dnagpu_dna_pack.argtypes = [vp, C.c_char_p, C.c_uint64, C.c_int, C.POINTER(vp), u64p, C.c_char_p]
    L.dnagpu_dna_unpack.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_dna_revcomp.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_kmers_to_text.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, C.c_int]
    L.dnagpu_dna_wire_size.argtypes = [C.c_uint64]
    L.dnagpu_dna_wire_size.restype = C.c_uint64
    L.dnagpu_dna_from_wire.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.dnagpu_dna_to_wire.argtypes = [vp, vp, vp, C.c_uint64, C.c_int]
    L.dnagpu_dna_length.argtypes = [vp]
    L.dnagpu_dna_length.restype = C.c_uint64
    L.dnagpu_dna_device_words.argtypes = [vp]
    L.dnagpu_dna_device_words.restype = vp
    L.dnagpu_dna_free.argtypes = [vp, vp]
    L.dnagpu_dna_free.restype = None
    L.dnagpu_kmer_count.argtypes = [C.c_uint64, C.c_int, u64p]
    L.dnagpu_generate_kmers.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_generate_kmers_filtered.argtypes = [vp, vp, C.c_int, C.POINTER(_FilterC), C.c_uint64,
                                                 C.c_uint64, vp, vp, C.c_uint64, u64p, C.c_int]
    L.dnagpu_count_kmers.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_count_kmers_unordered.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_hist_is_sorted.argtypes = [vp]
    L.dnagpu_count_kmers_batch.argtypes = [vp, vp, u64p, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.dnagpu_generate_kmers_table.argtypes = [vp, vp, C.c_int, C.POINTER(_FilterC), C.c_uint64, C.c_uint64, vp, vp, vp,
                                              C.c_uint64, u64p, C.c_int]
    L.dnagpu_dna_set_sequences.argtypes = [vp, vp, u64p, C.c_uint64]
    L.dnagpu_dna_sequences.argtypes = [vp]
    L.dnagpu_dna_sequences.restype = C.c_uint64
    L.dnagpu_count_kmers_table.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.dnagpu_dna_gather.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.dnagpu_dna_take.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.dnagpu_dna_sequence_starts.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_sk_buckets.argtypes = [vp, C.c_uint64, C.c_int]
    L.dnagpu_sk_records.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_records_buckets.argtypes = [vp]
    L.dnagpu_records_buckets.restype = C.c_uint32
    L.dnagpu_records_offsets.argtypes = [vp, u64p]
    L.dnagpu_records_device.argtypes = [vp]
    L.dnagpu_records_device.restype = vp
    L.dnagpu_records_free.argtypes = [vp, vp]
    L.dnagpu_records_free.restype = None
    L.dnagpu_count_records.argtypes = [vp, C.POINTER(vp), u64p, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_uint64,
                                       C.POINTER(vp)]
    L.dnagpu_count_keys.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.dnagpu_count_kmers_owned.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(vp)]
    L.dnagpu_count_keys_in_range.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_hist_distinct.argtypes = [vp]
    L.dnagpu_hist_distinct.restype = C.c_uint64
    L.dnagpu_hist_total.argtypes = [vp]
    L.dnagpu_hist_total.restype = C.c_uint64
    L.dnagpu_hist_extent.argtypes = [vp]
    L.dnagpu_hist_extent.restype = C.c_uint64
    L.dnagpu_hist_device_keys.argtypes = [vp]
    L.dnagpu_hist_device_keys.restype = vp
    L.dnagpu_hist_device_counts.argtypes = [vp]
    L.dnagpu_hist_device_counts.restype = vp
    L.dnagpu_hist_download.argtypes = [vp, vp, C.c_uint64, C.c_uint64, u64p, u64p]
    L.dnagpu_hist_summary.argtypes = [vp, vp, u64p, u64p, u64p]
    L.dnagpu_hist_sorted_view.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp]
    L.dnagpu_hist_merge.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.dnagpu_hist_free.argtypes = [vp, vp]
    L.dnagpu_hist_free.restype = None
    L.dnagpu_acc_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.dnagpu_acc_add.argtypes = [vp, vp, vp]
    L.dnagpu_acc_add_canonical.argtypes = [vp, vp, vp]
    L.dnagpu_acc_distinct.argtypes = [vp]
    L.dnagpu_acc_distinct.restype = C.c_uint64
    L.dnagpu_acc_total.argtypes = [vp]
    L.dnagpu_acc_total.restype = C.c_uint64
    L.dnagpu_acc_summary.argtypes = [vp, vp, u64p, u64p, u64p]
    L.dnagpu_acc_download.argtypes = [vp, vp, C.c_uint64, C.c_uint64, u64p, u64p]
    L.dnagpu_acc_free.argtypes = [vp, vp]
    L.dnagpu_acc_free.restype = None
    L.dnagpu_acc_join.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, C.c_uint64, u64p, C.POINTER(JoinStats), C.c_int]
    L.dnagpu_acc_partitions.argtypes = [vp]
    L.dnagpu_acc_partitions.restype = C.c_uint64
    L.dnagpu_table_hits.argtypes = [vp, vp, vp, C.c_uint, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    for f in ("sequences", "first"):
        getattr(L, f"dnagpu_seq_hits_{f}").argtypes = [vp]
        getattr(L, f"dnagpu_seq_hits_{f}").restype = C.c_uint64
    L.dnagpu_seq_hits_k.argtypes = [vp]
    L.dnagpu_seq_hits_totals.argtypes = [vp, u64p, u64p, u64p]
    for f in ("rows", "hits"):
        getattr(L, f"dnagpu_seq_hits_device_{f}").argtypes = [vp]
        getattr(L, f"dnagpu_seq_hits_device_{f}").restype = vp
    L.dnagpu_seq_hits_read.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_int]
    L.dnagpu_seq_hits_select.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, vp, C.c_uint64, u64p,
                                         C.c_int]
    L.dnagpu_seq_hits_free.argtypes = [vp, vp]
    L.dnagpu_seq_hits_free.restype = None
    L.dnagpu_profile_width.argtypes = [C.c_int]
    L.dnagpu_profile_width.restype = C.c_uint64
    L.dnagpu_table_profile.argtypes = [vp, vp, C.c_int, C.c_uint, C.c_uint64, C.c_uint64, vp, vp, C.c_int]
    L.dnagpu_profile_geometry.argtypes = [u64p, u64p]
    L.dnagpu_table_from_text.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.c_uint, C.POINTER(vp), vp, C.c_uint64,
                                         C.POINTER(_TextReportC)]
    L.dnagpu_text_geometry.argtypes = [u64p]
    L.dnagpu_reads_from_text.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(_ReadsOptionsC), C.POINTER(vp), vp, C.c_uint64,
                                         vp, vp, C.c_uint64, C.POINTER(_ReadsReportC)]
    L.dnagpu_table_to_text.argtypes = [vp, vp, C.POINTER(_TextOutOptionsC), C.POINTER(vp)]
    for f in ("bytes", "sequences", "empty"):
        getattr(L, f"dnagpu_text_image_{f}").argtypes = [vp]
        getattr(L, f"dnagpu_text_image_{f}").restype = C.c_uint64
    L.dnagpu_text_image_read.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_text_image_record_pos.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_text_image_free.argtypes = [vp, vp]
    L.dnagpu_text_image_free.restype = None
    L.dnagpu_text_out_geometry.argtypes = [u64p]
    L.dnagpu_quals_upload.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(vp), C.POINTER(_QualsReportC)]
    L.dnagpu_quals_bases.argtypes = [vp]
    L.dnagpu_quals_bases.restype = C.c_uint64
    L.dnagpu_quals_read.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_quals_free.argtypes = [vp, vp]
    L.dnagpu_quals_free.restype = None
    L.dnagpu_quals_from_fastq.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, vp, vp, C.POINTER(vp), C.POINTER(_QualsReportC)]
    L.dnagpu_quals_gather.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.dnagpu_quals_take.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.dnagpu_text_image_read_quals.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_quals_copy_geometry.argtypes = [u64p, u64p, u64p]
    L.dnagpu_quals_trim.argtypes = [vp, vp, vp, C.POINTER(_QualsTrimOptionsC), vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_int,
                                    C.POINTER(_QualsTrimReportC)]
    L.dnagpu_quals_geometry.argtypes = [u64p, u64p, u64p]
    L.dnagpu_dna_adapters.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(_AdaptersOptionsC), vp, vp, vp, C.c_uint64,
                                      C.c_int, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(_AdaptersReportC)]
    L.dnagpu_adapters_geometry.argtypes = [u64p, u64p, u64p]
    L.dnagpu_names_upload.argtypes = [vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(vp), C.POINTER(_NamesReportC)]
    L.dnagpu_names_sequences.argtypes = [vp]
    L.dnagpu_names_sequences.restype = C.c_uint64
    L.dnagpu_names_bytes.argtypes = [vp]
    L.dnagpu_names_bytes.restype = C.c_uint64
    L.dnagpu_names_offsets.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_names_read.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_int]
    L.dnagpu_names_free.argtypes = [vp, vp]
    L.dnagpu_names_free.restype = None
    L.dnagpu_names_from_text.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.c_uint, vp, C.c_uint64, vp, C.c_uint64,
                                         C.POINTER(vp), C.POINTER(_NamesReportC)]
    L.dnagpu_names_take.argtypes = [vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.dnagpu_table_to_text_named.argtypes = [vp, vp, vp, C.POINTER(_TextOutOptionsC), C.POINTER(vp)]
    L.dnagpu_names_geometry.argtypes = [u64p, u64p, u64p]
    L.dnagpu_dna_equals.argtypes = [vp, vp, vp, C.POINTER(C.c_int)]
    L.dnagpu_table_classes.argtypes = [vp, vp, C.POINTER(vp)]
    for f in ("sequences", "distinct"):
        getattr(L, f"dnagpu_seq_classes_{f}").argtypes = [vp]
        getattr(L, f"dnagpu_seq_classes_{f}").restype = C.c_uint64
    L.dnagpu_seq_classes_rounds.argtypes = [vp]
    L.dnagpu_seq_classes_rounds.restype = C.c_uint32
    L.dnagpu_seq_classes_read.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_int]
    L.dnagpu_seq_classes_select.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, u64p, C.c_int]
    L.dnagpu_seq_classes_members.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, C.c_int]
    L.dnagpu_table_match.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, vp, u64p, C.c_int]
    L.dnagpu_seq_classes_free.argtypes = [vp, vp]
    L.dnagpu_seq_classes_free.restype = None
    L.dnagpu_seq_equal_geometry.argtypes = [u64p, u64p]
    for obj in ("hist", "acc"):
        getattr(L, f"dnagpu_{obj}_spectrum").argtypes = [vp, vp, C.c_uint64, u64p]
        getattr(L, f"dnagpu_{obj}_select").argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, u64p, C.c_int]
        getattr(L, f"dnagpu_{obj}_top").argtypes = [vp, vp, C.c_uint64, vp, vp, u64p, C.c_int]
        getattr(L, f"dnagpu_{obj}_rank").argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.dnagpu_ranking_rows.argtypes = [vp]
    L.dnagpu_ranking_rows.restype = C.c_uint64
    L.dnagpu_ranking_order.argtypes = [vp]
    L.dnagpu_ranking_device_keys.argtypes = [vp]
    L.dnagpu_ranking_device_keys.restype = vp
    L.dnagpu_ranking_device_counts.argtypes = [vp]
    L.dnagpu_ranking_device_counts.restype = vp
    L.dnagpu_ranking_read.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_int]
    L.dnagpu_ranking_free.argtypes = [vp, vp]
    L.dnagpu_ranking_free.restype = None
    L.dnagpu_partition_kmers.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(vp), u64p]
    L.dnagpu_buffer_alloc.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_buffer_free.argtypes = [vp, vp]
    L.dnagpu_buffer_free.restype = None
    L.dnagpu_buffer_download.argtypes = [vp, vp, C.c_uint64, vp]
    L.dnagpu_buffer_upload.argtypes = [vp, vp, vp, C.c_uint64]
    L.dnagpu_kmer_hash.argtypes = [vp, vp, C.c_uint64, vp, C.c_int]
    L.dnagpu_kmer_strand.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, vp, vp, C.c_int]
    L.dnagpu_kmer_match.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(_FilterC), vp, C.c_int]
    L.dnagpu_kmer_index_build.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(vp)]
    for f in ("rows", "distinct", "next_row"):
        getattr(L, f"dnagpu_kmer_index_{f}").argtypes = [vp]
        getattr(L, f"dnagpu_kmer_index_{f}").restype = C.c_uint64
    L.dnagpu_kmer_index_k.argtypes = [vp]
    L.dnagpu_kmer_index_scan.argtypes = [vp, vp, C.POINTER(_FilterC), vp, vp, C.c_uint64, u64p, u64p, C.c_int]
    L.dnagpu_kmer_index_lookup.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_int]
    L.dnagpu_kmer_index_read.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_int]
    L.dnagpu_kmer_index_free.argtypes = [vp, vp]
    L.dnagpu_kmer_index_free.restype = None
    L.dnagpu_kmer_index_append.argtypes = [vp, vp, vp, C.c_uint64, C.c_int]
    L.dnagpu_kmer_index_delete.argtypes = [vp, vp, vp, C.c_uint64, C.c_int, u64p]
    L.dnagpu_multi_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(vp)]
    L.dnagpu_multi_destroy.argtypes = [vp]
    L.dnagpu_multi_destroy.restype = None
    L.dnagpu_multi_size.argtypes = [vp]
    L.dnagpu_multi_ctx.argtypes = [vp, C.c_int]
    L.dnagpu_multi_ctx.restype = vp
    L.dnagpu_multi_transport.argtypes = [vp]
    L.dnagpu_multi_transport.restype = C.c_char_p
    L.dnagpu_multi_dna_upload.argtypes = [vp, u64p, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_multi_dna_synth.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_multi_dna_length.argtypes = [vp]
    L.dnagpu_multi_dna_length.restype = C.c_uint64
    L.dnagpu_multi_dna_free.argtypes = [vp, vp]
    L.dnagpu_multi_dna_free.restype = None
    L.dnagpu_count_multi.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_count_multi_unordered.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.dnagpu_device_count.restype = C.c_int
    L.dnagpu_multi_set_option.argtypes = [vp, C.c_int, C.c_double]
    L.dnagpu_multi_last_times.argtypes = [vp, C.POINTER(_MultiTimes)]
    L.dnagpu_multi_exchange_transport.argtypes = [vp]
    L.dnagpu_multi_exchange_transport.restype = C.c_char_p
    L.dnagpu_multi_rccl_ranks.argtypes = [vp]
    L.dnagpu_multi_last_phase_times.argtypes = [vp, C.c_int, C.POINTER(_PhaseTimes)]
    L.dnagpu_hist_parts.argtypes = [vp]
    L.dnagpu_hist_parts.restype = C.c_uint32
    L.dnagpu_hist_part.argtypes = [vp, C.c_uint32]
    L.dnagpu_hist_part.restype = vp
    L.dnagpu_last_phase_times.argtypes = [vp, C.POINTER(_PhaseTimes)]
    L.dnagpu_set_profiling.argtypes = [vp, C.c_int]
    L.dnagpu_set_debug.argtypes = [vp, C.c_uint]
    _LIB = L
    return L


class DnaGpuError(Exception):
    def __init__(self, code):
        self.code = code
        self.message = lib().dnagpu_strerror(code).decode()
        detail = lib().dnagpu_last_error().decode()
        super().__init__(self.message + (f" [{detail}]" if detail and code >= ERR_BAD_ARG else ""))


def _chk(rc):
    if rc != OK:
        raise DnaGpuError(rc)


def strerror(code):
    return lib().dnagpu_strerror(code).decode()


def device_count():
    """HIP devices this process can use (no context is created)"""
    return int(lib().dnagpu_device_count())


def abi_version():
    return lib().dnagpu_abi_version()


def profile_width(k):
    """columns of a profile: 4^k for k in 1 .. 6, otherwise 0 (dnagpu_profile_width; needs no device)"""
    return int(lib().dnagpu_profile_width(k))


def text_geometry():
    """the bytes of text one workgroup of dnagpu_table_from_text sweeps (needs no device)"""
    t = C.c_uint64()
    _chk(lib().dnagpu_text_geometry(C.byref(t)))
    return t.value


def text_out_geometry():
    """the bytes of the image one workgroup of dnagpu_text_image_read forms (needs no device)"""
    t = C.c_uint64()
    _chk(lib().dnagpu_text_out_geometry(C.byref(t)))
    return t.value


def quals_copy_geometry():
    """(chunk_bytes, tile_bytes, lds_segments): the bytes one lane and one workgroup of the quality column's copy form, and
    the most segments of a tile it stages in LDS (needs no device)"""
    c, t, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _chk(lib().dnagpu_quals_copy_geometry(C.byref(c), C.byref(t), C.byref(s)))
    return c.value, t.value, s.value


def names_geometry():
    """(chunk_bytes, tile_bytes, group_tiles): the bytes of text one lane and one workgroup of dnagpu_names_from_text's sweep
    mark, and the tiles whose suffix minimum one workgroup forms (needs no device)"""
    c, t, g = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _chk(lib().dnagpu_names_geometry(C.byref(c), C.byref(t), C.byref(g)))
    return c.value, t.value, g.value


def quals_geometry():
    """(group_bases, wave_bases, tile_bases): the length limits of dnagpu_quals_trim's paths (needs no device)"""
    g, w, t = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _chk(lib().dnagpu_quals_geometry(C.byref(g), C.byref(w), C.byref(t)))
    return g.value, w.value, t.value


def adapters_geometry():
    """(group_bases, wave_bases, tile_bases): the segment lengths at which dnagpu_dna_adapters changes path (needs no device)"""
    g, w, t = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _chk(lib().dnagpu_adapters_geometry(C.byref(g), C.byref(w), C.byref(t)))
    return g.value, w.value, t.value


def profile_geometry():
    """(wave_rows, tile_rows): the row limits of dnagpu_table_profile's two sequence classes"""
    w, t = C.c_uint64(), C.c_uint64()
    _chk(lib().dnagpu_profile_geometry(C.byref(w), C.byref(t)))
    return w.value, t.value


def seq_equal_geometry():
    """(wave_bases, tile_bases): the base limits of the two sequence classes of the equality kernels"""
    w, t = C.c_uint64(), C.c_uint64()
    _chk(lib().dnagpu_seq_equal_geometry(C.byref(w), C.byref(t)))
    return w.value, t.value


def kmer_count(n_bases, k):
    out = C.c_uint64()
    _chk(lib().dnagpu_kmer_count(n_bases, k, C.byref(out)))
    return out.value


class Filter:
    """Right-hand side of a WHERE operator on generate_kmers rows."""

    def __init__(self, kind, length=0, bits=0, pattern=""):
        self.c = _FilterC()
        self.c.kind = kind
        self.c.length = length
        self.c.bits = int(bits)
        self.c.pattern = pattern.encode()[:35]

    @staticmethod
    def equals(length, bits):          # kmer = q
        return Filter(FILTER_EQUALS, length, bits)

    @staticmethod
    def starts_with(length, bits):     # kmer ^@ prefix
        return Filter(FILTER_STARTS_WITH, length, bits)

    @staticmethod
    def contains(pattern):             # qkmer @> kmer
        return Filter(FILTER_CONTAINS, 0, 0, pattern)


class Dna:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def n_bases(self):
        return int(lib().dnagpu_dna_length(self.h))

    @property
    def device_words(self):
        return lib().dnagpu_dna_device_words(self.h)

    def download(self):
        nw = (self.n_bases + 31) // 32
        out = np.empty(max(nw, 1), dtype=np.uint64)
        _chk(lib().dnagpu_dna_download(self.ctx.h, self.h, out.ctypes.data_as(u64p)))
        return out[:nw]

    def set_sequences(self, seq_starts):
        """this packed stream is a TABLE of sequences: seq_starts = the first base of each + the total (n_seqs + 1 entries),
        kept on the device beside it (dnagpu_dna_set_sequences) for Context.count_kmers_table"""
        st = np.ascontiguousarray(seq_starts, dtype=np.uint64)
        _chk(lib().dnagpu_dna_set_sequences(self.ctx.h, self.h, st.ctypes.data_as(u64p), max(len(st) - 1, 0)))

    @property
    def n_sequences(self):
        return int(lib().dnagpu_dna_sequences(self.h))

    def sequence_starts(self, first=0, count=None):
        """entries [first, first + count) of the n_sequences + 1 starts of the resident sequence set (count=None: all from
        first on; a Dna without a set has none) -> uint64[]"""
        if count is None:
            count = (self.n_sequences + 1 if self.n_sequences else 0) - first
        out = np.empty(max(count, 1), dtype=np.uint64)
        _chk(lib().dnagpu_dna_sequence_starts(self.ctx.h, self.h, first, count, out.ctypes.data, 0))
        return out[:count]

    def sequence_starts_device(self, first, count, dev_out):
        """the same into count uint64 of device memory"""
        _chk(lib().dnagpu_dna_sequence_starts(self.ctx.h, self.h, first, count, dev_out, 1))

    def free(self):
        if self.h:
            lib().dnagpu_dna_free(self.ctx.h, self.h)
            self.h = None


class Records:
    """dnagpu_records: 16-byte super-k-mer records in device memory, grouped by coarse bucket"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h
        self.n_buckets = int(lib().dnagpu_records_buckets(h))
        self.offsets = np.zeros(self.n_buckets + 1, dtype=np.uint64)
        _chk(lib().dnagpu_records_offsets(h, self.offsets.ctypes.data_as(u64p)))
        self.device_ptr = lib().dnagpu_records_device(h)
        self.n_records = int(self.offsets[-1])

    def free(self):
        if self.h:
            lib().dnagpu_records_free(self.ctx.h, self.h)
            self.h = None


class Ranking:
    """dnagpu_ranking: every group of a Hist / an Accumulator in count order, a snapshot in device memory (Hist.rank,
    Accumulator.rank)"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def rows(self):
        return int(lib().dnagpu_ranking_rows(self.h))

    @property
    def order(self):
        return int(lib().dnagpu_ranking_order(self.h))

    @property
    def device_keys(self):
        """device pointer of `rows` uint64 keys in rank order (None for an empty ranking)"""
        return lib().dnagpu_ranking_device_keys(self.h)

    @property
    def device_counts(self):
        return lib().dnagpu_ranking_device_counts(self.h)

    def read(self, first=0, count=None, on_device=False, out=None):
        """rows [first, first + count) of the order (count=None: all from first on).  host: -> (keys, counts).  on_device:
        into out=(dev_keys, dev_counts) of count uint64 each (either may be None) -> count; without out the arrays are
        allocated here (Context.buffer_free them) -> (dev_keys, dev_counts, count)"""
        if count is None:
            count = self.rows - first
        fn = lib().dnagpu_ranking_read
        if on_device:
            dk, dc = out if out is not None else (self.ctx.buffer_alloc(8 * max(count, 1)), self.ctx.buffer_alloc(8 * max(count, 1)))
            _chk(fn(self.ctx.h, self.h, first, count, dk, dc, 1))
            return count if out is not None else (dk, dc, count)
        keys = np.empty(max(count, 1), dtype=np.uint64)
        counts = np.empty(max(count, 1), dtype=np.uint64)
        _chk(fn(self.ctx.h, self.h, first, count, keys.ctypes.data, counts.ctypes.data, 0))
        return keys[:count], counts[:count]

    def free(self):
        if self.h:
            if self.ctx._base_debug & DEBUG_GUARD_POOL:
                self.ctx.synchronize()          # raises if a kernel wrote past the end of a work buffer
            lib().dnagpu_ranking_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class SeqHits:
    """dnagpu_seq_hits: for every sequence of a window of a table, its rows and how many of them occur in a counted set; a
    snapshot in device memory (Context.table_hits)"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def sequences(self):
        return int(lib().dnagpu_seq_hits_sequences(self.h))

    @property
    def first(self):
        return int(lib().dnagpu_seq_hits_first(self.h))

    @property
    def k(self):
        return int(lib().dnagpu_seq_hits_k(self.h))

    @property
    def device_rows(self):
        """device pointer of `sequences` uint32 (None for a window of 0 sequences)"""
        return lib().dnagpu_seq_hits_device_rows(self.h)

    @property
    def device_hits(self):
        return lib().dnagpu_seq_hits_device_hits(self.h)

    def totals(self):
        """-> (rows, hits, sequences with at least one hit) over the window"""
        r, h, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(lib().dnagpu_seq_hits_totals(self.h, C.byref(r), C.byref(h), C.byref(s)))
        return r.value, h.value, s.value

    def read(self, first=0, count=None, on_device=False, out=None):
        """entries [first, first + count) of the window (count=None: all from first on), as uint64.  host: -> (rows, hits).
        on_device: into out=(dev_rows, dev_hits) of count uint64 each (either may be None) -> count; without out the arrays
        are allocated here (Context.buffer_free them) -> (dev_rows, dev_hits, count)"""
        if count is None:
            count = self.sequences - first
        fn = lib().dnagpu_seq_hits_read
        if on_device:
            if out is not None:
                _chk(fn(self.ctx.h, self.h, first, count, out[0], out[1], 1))
                return count
            dr = self.ctx.buffer_alloc(8 * max(count, 1))
            dh = None
            try:
                dh = self.ctx.buffer_alloc(8 * max(count, 1))
                _chk(fn(self.ctx.h, self.h, first, count, dr, dh, 1))
            except Exception:
                self.ctx.buffer_free(dr)
                if dh is not None:
                    self.ctx.buffer_free(dh)
                raise
            return dr, dh, count
        rows = np.empty(max(count, 1), dtype=np.uint64)
        hits = np.empty(max(count, 1), dtype=np.uint64)
        _chk(fn(self.ctx.h, self.h, first, count, rows.ctypes.data, hits.ctypes.data, 0))
        return rows[:count], hits[:count]

    def select(self, min_hits=0, max_hits=U64_MAX, frac=(0, 1), cap=None, on_device=False, out=None, want=(True, True, True)):
        """the sequences with min_hits <= hits <= max_hits and hits / rows >= frac[0] / frac[1], in ascending sequence id.
        host: -> (seq, rows, hits, n_matches): at most cap rows (cap=None: all of them -- two calls); an array `want` turns
        off comes back as None.  on_device: into out=(dev_seq, dev_rows, dev_hits) of cap uint64 each (any may be None) ->
        n_matches"""
        n = C.c_uint64()
        fn = lib().dnagpu_seq_hits_select
        num, den = frac
        if cap is None:
            _chk(fn(self.ctx.h, self.h, min_hits, max_hits, num, den, None, None, None, 0, C.byref(n), 0))
            cap = n.value
        if on_device:
            ds, dr, dh = out
            _chk(fn(self.ctx.h, self.h, min_hits, max_hits, num, den, ds, dr, dh, cap, C.byref(n), 1))
            return n.value
        arrs = [np.empty(max(cap, 1), dtype=np.uint64) if w else None for w in want]
        ptrs = [a.ctypes.data if a is not None else None for a in arrs]
        _chk(fn(self.ctx.h, self.h, min_hits, max_hits, num, den, ptrs[0], ptrs[1], ptrs[2], cap, C.byref(n), 0))
        m = min(n.value, cap)
        return tuple(a[:m] if a is not None else None for a in arrs) + (n.value,)

    def free(self):
        if self.h:
            if self.ctx._base_debug & DEBUG_GUARD_POOL:
                self.ctx.synchronize()          # raises if a kernel wrote past the end of a work buffer
            lib().dnagpu_seq_hits_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class SeqClasses:
    """dnagpu_seq_classes: the classes of equal sequences of a resident table (Context.table_classes).  It borrows the table:
    keep the Dna alive and its sequence set unchanged until free()"""

    def __init__(self, ctx, handle, table):
        self.ctx, self.h, self.table = ctx, handle, table

    @property
    def sequences(self):
        return int(lib().dnagpu_seq_classes_sequences(self.h))

    @property
    def distinct(self):
        return int(lib().dnagpu_seq_classes_distinct(self.h))

    @property
    def rounds(self):
        return int(lib().dnagpu_seq_classes_rounds(self.h))

    def read(self, first=0, count=None, on_device=False, out=None):
        """entries [first, first + count) (count=None: all from first on) -> (rep, copies) as uint64: the smallest id of the
        sequence's class and the class's size.  on_device: into out=(dev_rep, dev_copies) of count uint64 each (either may be
        None) -> count"""
        if count is None:
            count = self.sequences - first
        fn = lib().dnagpu_seq_classes_read
        if on_device:
            _chk(fn(self.ctx.h, self.h, first, count, out[0], out[1], 1))
            return count
        rep = np.empty(max(count, 1), dtype=np.uint64)
        copies = np.empty(max(count, 1), dtype=np.uint64)
        _chk(fn(self.ctx.h, self.h, first, count, rep.ctypes.data, copies.ctypes.data, 0))
        return rep[:count], copies[:count]

    def select(self, min_copies=1, max_copies=U64_MAX, cap=None, on_device=False, out=None, want=(True, True)):
        """the representatives with min_copies <= copies <= max_copies in ascending id (GROUP BY sequence: min(id), count(*),
        HAVING).  host: -> (seq, copies, n_matches): at most cap rows (cap=None: all of them -- two calls); an array `want`
        turns off comes back as None.  on_device: into out=(dev_seq, dev_copies) of cap uint64 each (either may be None) ->
        n_matches; dev_seq goes straight into Context.dna_take_device"""
        n = C.c_uint64()
        fn = lib().dnagpu_seq_classes_select
        if cap is None:
            _chk(fn(self.ctx.h, self.h, min_copies, max_copies, None, None, 0, C.byref(n), 0))
            cap = n.value
        if on_device:
            _chk(fn(self.ctx.h, self.h, min_copies, max_copies, out[0], out[1], cap, C.byref(n), 1))
            return n.value
        arrs = [np.empty(max(cap, 1), dtype=np.uint64) if w else None for w in want]
        ptrs = [a.ctypes.data if a is not None else None for a in arrs]
        _chk(fn(self.ctx.h, self.h, min_copies, max_copies, ptrs[0], ptrs[1], cap, C.byref(n), 0))
        m = min(n.value, cap)
        return tuple(a[:m] if a is not None else None for a in arrs) + (n.value,)

    def members(self, seq, cap=None, on_device=False, out=None):
        """the ids of every sequence equal to sequence seq, seq included, ascending -> (ids, n_matches); on_device: into
        out = dev_seq of cap uint64 -> n_matches"""
        n = C.c_uint64()
        fn = lib().dnagpu_seq_classes_members
        if cap is None:
            _chk(fn(self.ctx.h, self.h, seq, None, 0, C.byref(n), 0))
            cap = n.value
        if on_device:
            _chk(fn(self.ctx.h, self.h, seq, out, cap, C.byref(n), 1))
            return n.value
        ids = np.empty(max(cap, 1), dtype=np.uint64)
        _chk(fn(self.ctx.h, self.h, seq, ids.ctypes.data, cap, C.byref(n), 0))
        return ids[:min(n.value, cap)], n.value

    def match(self, probe, seq_first=0, seq_count=None, on_device=False, out=None):
        """the join of the resident table probe to this one: for every sequence of [seq_first, seq_first + seq_count) of probe
        (seq_count=None: all from seq_first on) the smallest id here of a sequence equal to it (MATCH_NONE: none) and that
        class's size (0) -> (match, copies, n_matched).  on_device: into out=(dev_match, dev_copies) of seq_count uint64 each
        (either may be None) -> n_matched"""
        if seq_count is None:
            seq_count = probe.n_sequences - seq_first
        n = C.c_uint64()
        fn = lib().dnagpu_table_match
        if on_device:
            _chk(fn(self.ctx.h, self.h, probe.h, seq_first, seq_count, out[0], out[1], C.byref(n), 1))
            return n.value
        match = np.empty(max(seq_count, 1), dtype=np.uint64)
        copies = np.empty(max(seq_count, 1), dtype=np.uint64)
        _chk(fn(self.ctx.h, self.h, probe.h, seq_first, seq_count, match.ctypes.data, copies.ctypes.data, C.byref(n), 0))
        return match[:seq_count], copies[:seq_count], n.value

    def free(self):
        if self.h:
            if self.ctx._base_debug & DEBUG_GUARD_POOL:
                self.ctx.synchronize()          # raises if a kernel wrote past the end of a work buffer
            lib().dnagpu_seq_classes_free(self.ctx.h, self.h)
            self.h = None
            self.table = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class TextImage:
    """dnagpu_text_image: the text image of a resident table (Context.table_to_text), read window by window.  It borrows
    the table: keep the Dna alive and its sequence set unchanged until free()"""

    def __init__(self, ctx, handle, table):
        self.ctx, self.h, self.table = ctx, handle, table
        self.names = None                   # table_to_text_named: the borrowed Names column

    @property
    def bytes(self):
        return int(lib().dnagpu_text_image_bytes(self.h))

    @property
    def sequences(self):
        return int(lib().dnagpu_text_image_sequences(self.h))

    @property
    def empty(self):
        """sequences of 0 bases in the image (the loaders refuse such records)"""
        return int(lib().dnagpu_text_image_empty(self.h))

    def read(self, first=0, count=None):
        """bytes [first, first + count) of the image (count=None: all from first on) -> bytes; at most 2^32 - 1 per call"""
        if count is None:
            count = self.bytes - first
        buf = C.create_string_buffer(max(count, 1))
        _chk(lib().dnagpu_text_image_read(self.ctx.h, self.h, first, count, buf, 0))
        return buf.raw[:count]

    def read_device(self, first, count, dev_ptr):
        """the same into `count` bytes of device memory at any byte alignment"""
        _chk(lib().dnagpu_text_image_read(self.ctx.h, self.h, first, count, dev_ptr, 1))

    def read_quals(self, quals, first=0, count=None):
        """read() of a FASTQ image with every quality line taken from the column quals (dnagpu_text_image_read_quals)"""
        if count is None:
            count = self.bytes - first
        buf = C.create_string_buffer(max(count, 1))
        _chk(lib().dnagpu_text_image_read_quals(self.ctx.h, self.h, quals.h, first, count, buf, 0))
        return buf.raw[:count]

    def read_quals_device(self, quals, first, count, dev_ptr):
        """the same into `count` bytes of device memory at any byte alignment"""
        _chk(lib().dnagpu_text_image_read_quals(self.ctx.h, self.h, quals.h, first, count, dev_ptr, 1))

    def record_pos(self, first=0, count=None):
        """entries [first, first + count) of the sequences + 1 record offsets (the last: the image's size) -> uint64 array"""
        if count is None:
            count = (self.sequences + 1 if self.sequences else 0) - first
        out = np.empty(max(count, 1), dtype=np.uint64)
        _chk(lib().dnagpu_text_image_record_pos(self.ctx.h, self.h, first, count, out.ctypes.data, 0))
        return out[:count]

    def free(self):
        if self.h:
            lib().dnagpu_text_image_free(self.ctx.h, self.h)
            self.h = None
            self.table = None
            self.names = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class Names:
    """dnagpu_names: the names column of a resident table, one byte string per sequence; no byte is a line terminator"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def n_sequences(self):
        return int(lib().dnagpu_names_sequences(self.h))

    @property
    def n_bytes(self):
        return int(lib().dnagpu_names_bytes(self.h))

    def offsets(self, first=0, count=None):
        """entries [first, first + count) of the n_sequences + 1 offsets -> uint64 array"""
        if count is None:
            count = self.n_sequences + 1 - first
        out = np.empty(max(count, 1), dtype=np.uint64)
        _chk(lib().dnagpu_names_offsets(self.ctx.h, self.h, first, count, out.ctypes.data, 0))
        return out[:count]

    def offsets_device(self, first, count, dev_ptr):
        _chk(lib().dnagpu_names_offsets(self.ctx.h, self.h, first, count, dev_ptr, 1))

    def read(self, first=0, count=None):
        """bytes [first, first + count) of the column (count=None: all from first on) -> bytes"""
        if count is None:
            count = self.n_bytes - first
        buf = C.create_string_buffer(max(count, 1))
        _chk(lib().dnagpu_names_read(self.ctx.h, self.h, first, count, buf, 0))
        return buf.raw[:count]

    def read_device(self, first, count, dev_ptr):
        _chk(lib().dnagpu_names_read(self.ctx.h, self.h, first, count, dev_ptr, 1))

    def download(self):
        """the column as a list of bytes, one per sequence"""
        off, b = self.offsets(), self.read()
        return [b[int(off[i]):int(off[i + 1])] for i in range(self.n_sequences)]

    def free(self):
        if self.h:
            lib().dnagpu_names_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class Quals:
    """dnagpu_quals: the quality column of a resident table, one Phred+33 byte per base of its stream.  It holds no
    boundaries: the calls that need them take the table too"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def n_bases(self):
        return int(lib().dnagpu_quals_bases(self.h))

    def read(self, first=0, count=None):
        """bytes [first, first + count) of the column (count=None: all from first on) -> bytes"""
        if count is None:
            count = self.n_bases - first
        buf = C.create_string_buffer(max(count, 1))
        _chk(lib().dnagpu_quals_read(self.ctx.h, self.h, first, count, buf, 0))
        return buf.raw[:count]

    def read_device(self, first, count, dev_ptr):
        _chk(lib().dnagpu_quals_read(self.ctx.h, self.h, first, count, dev_ptr, 1))

    def free(self):
        if self.h:
            lib().dnagpu_quals_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class KmerIndex:
    """dnagpu_kmer_index: the index over a stored kmer column (Context.kmer_index): built once, asked `=`, `^@` and `@>` many
    times, kept up to date with append / delete; answers are row ids in INDEX order (text order of the key under A < T < C < G, row ids ascending inside a key)"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def rows(self):
        return int(lib().dnagpu_kmer_index_rows(self.h))

    @property
    def distinct(self):
        return int(lib().dnagpu_kmer_index_distinct(self.h))

    @property
    def k(self):
        return int(lib().dnagpu_kmer_index_k(self.h))

    @property
    def next_row(self):
        """the rows the index has ever been given = the row id of the next appended key"""
        return int(lib().dnagpu_kmer_index_next_row(self.h))

    def append(self, keys, on_device=False):
        """appends keys (row ids next_row, next_row + 1, ...).  host: an array of keys; on_device: (dev_keys, m)"""
        if on_device:
            dev_keys, m = keys
            _chk(lib().dnagpu_kmer_index_append(self.ctx.h, self.h, dev_keys, m, 1))
            return
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        _chk(lib().dnagpu_kmer_index_append(self.ctx.h, self.h, a.ctypes.data if a.size else None, a.size, 0))

    def delete(self, rows, on_device=False):
        """removes the entries of the listed row ids (ids the index does not hold are ignored) -> the entries removed.
        host: an array of ids; on_device: (dev_rows, m)"""
        n_deleted = C.c_uint64()
        if on_device:
            dev_rows, m = rows
            _chk(lib().dnagpu_kmer_index_delete(self.ctx.h, self.h, dev_rows, m, 1, C.byref(n_deleted)))
            return n_deleted.value
        a = np.ascontiguousarray(rows, dtype=np.uint64)
        _chk(lib().dnagpu_kmer_index_delete(self.ctx.h, self.h, a.ctypes.data if a.size else None, a.size, 0, C.byref(n_deleted)))
        return n_deleted.value

    def scan(self, flt, cap=None, want_rows=True, want_keys=True, on_device=False, out=None):
        """the rows that satisfy flt.  host: -> (rows, keys, n_out, visited), rows / keys the first min(cap, n_out) matches
        (None where not wanted; cap=None: all of them, found with a counting call first).  on_device: into
        out=(dev_rows, dev_keys) of cap uint64 each (either may be None) -> (n_out, visited)"""
        fn = lib().dnagpu_kmer_index_scan
        n_out, visited = C.c_uint64(), C.c_uint64()
        if on_device:
            dr, dk = out
            _chk(fn(self.ctx.h, self.h, C.byref(flt.c), dr, dk, cap or 0, C.byref(n_out), C.byref(visited), 1))
            return n_out.value, visited.value
        if cap is None:
            _chk(fn(self.ctx.h, self.h, C.byref(flt.c), None, None, 0, C.byref(n_out), C.byref(visited), 0))
            cap = n_out.value
        rows = np.empty(max(cap, 1), dtype=np.uint64) if want_rows else None
        keys = np.empty(max(cap, 1), dtype=np.uint64) if want_keys else None
        _chk(fn(self.ctx.h, self.h, C.byref(flt.c), rows.ctypes.data if want_rows else None,
                keys.ctypes.data if want_keys else None, cap, C.byref(n_out), C.byref(visited), 0))
        m = min(cap, n_out.value)
        return (rows[:m] if want_rows else None, keys[:m] if want_keys else None, n_out.value, visited.value)

    def lookup(self, keys):
        """batch equality: -> (first, count) per query key: its window of the index order (count 0: absent)"""
        q = np.ascontiguousarray(keys, dtype=np.uint64)
        first = np.empty(max(q.size, 1), dtype=np.uint64)
        count = np.empty(max(q.size, 1), dtype=np.uint64)
        _chk(lib().dnagpu_kmer_index_lookup(self.ctx.h, self.h, q.ctypes.data, q.size, first.ctypes.data, count.ctypes.data, 0))
        return first[:q.size], count[:q.size]

    def lookup_device(self, dev_keys, m, dev_first, dev_count):
        _chk(lib().dnagpu_kmer_index_lookup(self.ctx.h, self.h, dev_keys, m, dev_first, dev_count, 1))

    def read(self, first=0, count=None, want_rows=True, want_keys=True):
        """entries [first, first + count) of the index order (count=None: all from first on) -> (rows, keys)"""
        if count is None:
            count = self.rows - first
        rows = np.empty(max(count, 1), dtype=np.uint64) if want_rows else None
        keys = np.empty(max(count, 1), dtype=np.uint64) if want_keys else None
        _chk(lib().dnagpu_kmer_index_read(self.ctx.h, self.h, first, count, rows.ctypes.data if want_rows else None,
                                          keys.ctypes.data if want_keys else None, 0))
        return (rows[:count] if want_rows else None, keys[:count] if want_keys else None)

    def read_device(self, first, count, dev_rows, dev_keys):
        _chk(lib().dnagpu_kmer_index_read(self.ctx.h, self.h, first, count, dev_rows, dev_keys, 1))

    def free(self):
        if self.h:
            if self.ctx._base_debug & DEBUG_GUARD_POOL:
                self.ctx.synchronize()          # raises if a kernel wrote past the end of a work buffer
            lib().dnagpu_kmer_index_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class _CountQueries:
    """the count-ordered queries Hist and Accumulator share (dnagpu_hist_* / dnagpu_acc_* spectrum, select, top, rank)"""

    _obj = None                       # "hist" / "acc"

    def _q(self, name):
        return getattr(lib(), f"dnagpu_{self._obj}_{name}")

    def spectrum(self, n_bins):
        """the k-mer spectrum: bins[c - 1] = groups with count c, bins[n_bins - 1] = groups with count >= n_bins"""
        bins = np.zeros(max(int(n_bins), 1), dtype=np.uint64)
        _chk(self._q("spectrum")(self.ctx.h, self.h, n_bins, bins.ctypes.data_as(u64p)))
        return bins[:n_bins]

    def select(self, min_count, max_count=U64_MAX, cap=None, on_device=False, out=None):
        """GROUP BY kmer HAVING count(*) BETWEEN min_count AND max_count, order unspecified.
        host: -> (keys, counts, n_matches): at most cap rows (cap=None: all of them -- two calls, the first with cap 0 sizes
        the arrays).  on_device: the rows go to device arrays of cap uint64 each -- out=(dev_keys, dev_counts) (either may
        be None) -> n_matches; without out they are allocated here (Context.buffer_free them) -> (dev_keys, dev_counts,
        n_matches)"""
        n = C.c_uint64()
        fn = self._q("select")
        if cap is None:
            _chk(fn(self.ctx.h, self.h, min_count, max_count, None, None, 0, C.byref(n), 0))
            cap = n.value
        if on_device:
            dk, dc = out if out is not None else (self.ctx.buffer_alloc(8 * max(cap, 1)), self.ctx.buffer_alloc(8 * max(cap, 1)))
            _chk(fn(self.ctx.h, self.h, min_count, max_count, dk, dc, cap, C.byref(n), 1))
            return n.value if out is not None else (dk, dc, n.value)
        keys = np.empty(max(cap, 1), dtype=np.uint64)
        counts = np.empty(max(cap, 1), dtype=np.uint64)
        _chk(fn(self.ctx.h, self.h, min_count, max_count, keys.ctypes.data, counts.ctypes.data, cap, C.byref(n), 0))
        m = min(n.value, cap)
        return keys[:m], counts[:m], n.value

    def top(self, n, on_device=False, out=None):
        """GROUP BY kmer ORDER BY count(*) DESC LIMIT n: min(n, distinct) rows, counts descending, keys ascending among equal
        counts.  host: -> (keys, counts).  on_device: into out=(dev_keys, dev_counts) of n uint64 each -> rows written;
        without out the arrays are allocated here (Context.buffer_free them) -> (dev_keys, dev_counts, rows)"""
        got = C.c_uint64()
        fn = self._q("top")
        if on_device:
            dk, dc = out if out is not None else (self.ctx.buffer_alloc(8 * max(n, 1)), self.ctx.buffer_alloc(8 * max(n, 1)))
            _chk(fn(self.ctx.h, self.h, n, dk, dc, C.byref(got), 1))
            return got.value if out is not None else (dk, dc, got.value)
        rows = min(n, self.distinct)
        keys = np.empty(max(rows, 1), dtype=np.uint64)
        counts = np.empty(max(rows, 1), dtype=np.uint64)
        _chk(fn(self.ctx.h, self.h, n, keys.ctypes.data, counts.ctypes.data, C.byref(got), 0))
        return keys[:got.value], counts[:got.value]


    def rank(self, order=ORDER_COUNT_DESC):
        """GROUP BY kmer ORDER BY count(*) [DESC] without a LIMIT: every group in count order -> Ranking (free it)"""
        r = C.c_void_p()
        _chk(self._q("rank")(self.ctx.h, self.h, order, C.byref(r)))
        return Ranking(self.ctx, r)


class Hist(_CountQueries):
    _obj = "hist"

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def distinct(self):
        return int(lib().dnagpu_hist_distinct(self.h))

    @property
    def total(self):
        return int(lib().dnagpu_hist_total(self.h))

    @property
    def extent(self):
        """slots of device_keys / device_counts in use (an unordered histogram may hold count-0 padding slots)"""
        return int(lib().dnagpu_hist_extent(self.h))

    @property
    def device_keys(self):
        return lib().dnagpu_hist_device_keys(self.h)

    @property
    def device_counts(self):
        return lib().dnagpu_hist_device_counts(self.h)

    @property
    def n_parts(self):
        """device-array sets this histogram consists of (the pipelined multi-GPU count makes several)"""
        return int(lib().dnagpu_hist_parts(self.h))

    def part_arrays(self, i):
        """(device keys pointer, device counts pointer, extent) of part i"""
        ph = C.c_void_p(lib().dnagpu_hist_part(self.h, i))
        return (lib().dnagpu_hist_device_keys(ph), lib().dnagpu_hist_device_counts(ph), int(lib().dnagpu_hist_extent(ph)))

    @property
    def is_sorted(self):
        return bool(lib().dnagpu_hist_is_sorted(self.h))

    def download(self, first=0, count=None, want_keys=True, want_counts=True):
        """groups [first, first+count) of the read order as (keys, counts) uint64 arrays; an array not wanted is passed as
        NULL and comes back as None"""
        if count is None:
            count = self.distinct - first
        keys = np.empty(max(count, 1), dtype=np.uint64) if want_keys else None
        counts = np.empty(max(count, 1), dtype=np.uint64) if want_counts else None
        _chk(lib().dnagpu_hist_download(self.ctx.h, self.h, first, count,
                                        keys.ctypes.data_as(u64p) if want_keys else None,
                                        counts.ctypes.data_as(u64p) if want_counts else None))
        return (keys[:count] if want_keys else None, counts[:count] if want_counts else None)

    def sorted_view_device(self, dev_keys, dev_counts, first=0, count=None):
        """ascending-key groups [first, first+count) into caller-owned device arrays of uint64"""
        if count is None:
            count = self.distinct - first
        _chk(lib().dnagpu_hist_sorted_view(self.ctx.h, self.h, first, count, dev_keys, dev_counts))

    def summary(self):
        """(total, distinct, unique, checksum) -- same tuple as the oracle's hist_summary"""
        t, u, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(lib().dnagpu_hist_summary(self.ctx.h, self.h, C.byref(t), C.byref(u), C.byref(c)))
        return t.value, self.distinct, u.value, c.value

    def merge(self, other):
        """-> a new Hist: the groups of self and other added up (dnagpu_hist_merge)"""
        h = C.c_void_p()
        _chk(lib().dnagpu_hist_merge(self.ctx.h, self.h, other.h, C.byref(h)))
        return Hist(self.ctx, h)

    def free(self):
        if self.h:
            if self.ctx._base_debug & DEBUG_GUARD_POOL:
                self.ctx.synchronize()          # raises if a kernel wrote past the end of a work buffer
            lib().dnagpu_hist_free(self.ctx.h, self.h)
            self.h = None


class Accumulator(_CountQueries):
    """dnagpu_acc: histograms added up on the device into 64-bit counts (no 2^32 limit); Context.accumulator(k)"""

    _obj = "acc"

    def __init__(self, ctx, k):
        self.ctx, self.h = ctx, C.c_void_p()
        _chk(lib().dnagpu_acc_create(ctx.h, k, C.byref(self.h)))

    def add(self, hist, canonical=False):
        """adds the groups of hist; canonical=True: under the canonical form of every key (dnagpu_acc_add_canonical), so
        that a k-mer and its reverse complement are one group"""
        fn = lib().dnagpu_acc_add_canonical if canonical else lib().dnagpu_acc_add
        _chk(fn(self.ctx.h, self.h, hist.h))

    @property
    def distinct(self):
        return int(lib().dnagpu_acc_distinct(self.h))

    @property
    def total(self):
        return int(lib().dnagpu_acc_total(self.h))

    @property
    def partitions(self):
        """partitions of the table, a power of two (0: no table yet)"""
        return int(lib().dnagpu_acc_partitions(self.h))

    def summary(self):
        """(total, distinct, unique, checksum) -- same tuple as Hist.summary and the oracle's hist_summary"""
        t, u, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(lib().dnagpu_acc_summary(self.ctx.h, self.h, C.byref(t), C.byref(u), C.byref(c)))
        return t.value, self.distinct, u.value, c.value

    def join(self, other, kind=JOIN_INNER, cap=None, on_device=False, out=None, want_rows=True):
        """the hash join with `other` on the k-mer (dnagpu_acc_join), self = the left side: JOIN_INNER the groups both hold,
        JOIN_ANTI those only self holds, JOIN_LEFT every group of self; order unspecified -> (keys, left, right, stats):
        at most cap rows (cap=None: all of them -- two calls, the first takes the statistics and sizes the arrays),
        stats = JoinStats over ALL result rows.  want_rows=False: the statistics only, the arrays are None.
        on_device: the rows go to device arrays of cap uint64 each -- out=(dev_keys, dev_left, dev_right) (any may be
        None); without out they are allocated here (Context.buffer_free them)"""
        n, st = C.c_uint64(), JoinStats()
        fn = lib().dnagpu_acc_join
        if not want_rows or cap is None:
            _chk(fn(self.ctx.h, self.h, other.h, kind, None, None, None, 0, C.byref(n), C.byref(st), 0))
            if not want_rows:
                return None, None, None, st
            cap = n.value
        if on_device:
            bufs = out if out is not None else tuple(self.ctx.buffer_alloc(8 * max(cap, 1)) for _ in range(3))
            _chk(fn(self.ctx.h, self.h, other.h, kind, bufs[0], bufs[1], bufs[2], cap, C.byref(n), C.byref(st), 1))
            return bufs[0], bufs[1], bufs[2], st
        arrs = [np.empty(max(cap, 1), dtype=np.uint64) for _ in range(3)]
        _chk(fn(self.ctx.h, self.h, other.h, kind, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, cap,
                C.byref(n), C.byref(st), 0))
        m = min(n.value, cap)
        return arrs[0][:m], arrs[1][:m], arrs[2][:m], st

    def download(self, first=0, count=None):
        """groups [first, first+count) as (keys, counts) uint64 arrays; order unspecified but fixed until the next add"""
        if count is None:
            count = self.distinct - first
        keys = np.empty(max(count, 1), dtype=np.uint64)
        counts = np.empty(max(count, 1), dtype=np.uint64)
        _chk(lib().dnagpu_acc_download(self.ctx.h, self.h, first, count, keys.ctypes.data_as(u64p),
                                       counts.ctypes.data_as(u64p)))
        return keys[:count], counts[:count]

    def free(self):
        if self.h:
            if self.ctx._base_debug & DEBUG_GUARD_POOL:
                self.ctx.synchronize()          # raises if a kernel wrote past the end of a work buffer
            lib().dnagpu_acc_free(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class Context:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(lib().dnagpu_init(device, C.byref(self.h)))
        # test harness switch (this wrapper is test/bench tooling): DNAGPU_TEST_POISON=1 runs every context
        # with DNAGPU_DEBUG_POISON_POOL, i.e. all work buffers pre-filled with 0xFF
        self._base_debug = _env_debug()
        if self._base_debug:
            self.set_debug(0)

    def set_debug(self, flags):
        """flags on top of what the environment asked for"""
        _chk(lib().dnagpu_set_debug(self.h, int(flags) | self._base_debug))

    def close(self):
        if self.h:
            lib().dnagpu_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        _chk(lib().dnagpu_synchronize(self.h))

    @property
    def stream(self):
        return lib().dnagpu_stream(self.h)

    def trim(self):
        _chk(lib().dnagpu_trim(self.h))

    def device_bytes(self):
        return int(lib().dnagpu_device_bytes(self.h))

    def set_profiling(self, on):
        _chk(lib().dnagpu_set_profiling(self.h, int(bool(on))))

    def last_phase_times(self):
        pt = _PhaseTimes()
        _chk(lib().dnagpu_last_phase_times(self.h, C.byref(pt)))
        return [(pt.names[i].decode(), float(pt.ms[i])) for i in range(pt.n)]

    # ---- dna
    def upload(self, words, n_bases):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if w.size < (n_bases + 31) // 32:
            raise ValueError("words shorter than n_bases")
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_upload(self.h, w.ctypes.data_as(u64p), n_bases, C.byref(h)))
        return Dna(self, h)

    def wrap(self, dev_ptr, n_words, n_bases):
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_wrap(self.h, dev_ptr, n_words, n_bases, C.byref(h)))
        return Dna(self, h)

    def _pack(self, text, n_bases, on_device):
        h = C.c_void_p()
        pos, ch = C.c_uint64(), C.create_string_buffer(1)
        rc = lib().dnagpu_dna_pack(self.h, text, n_bases, on_device, C.byref(h), C.byref(pos), ch)
        if rc == ERR_DNA_INVALID_CHAR:
            e = DnaGpuError(rc)
            e.message = f"{e.message}: {ch.raw.decode(errors='replace')}"
            e.bad_pos = pos.value
            e.bad_char = ch.raw
            e.args = (e.message,)
            raise e
        _chk(rc)
        return Dna(self, h)

    def pack(self, text):
        """dna_in on the device: text (str/bytes of A/T/C/G) -> Dna"""
        b = text.encode() if isinstance(text, str) else bytes(text)
        return self._pack(b, len(b), 0)

    def pack_device(self, dev_text, n_bases):
        """the same from n_bases characters already in device memory (any byte alignment)"""
        return self._pack(C.cast(C.c_void_p(dev_text), C.c_char_p), n_bases, 1)

    def _table_from_text(self, text, n_bytes, on_device, format, more, pos_ptr, cap):
        h, rep = C.c_void_p(), _TextReportC()
        rc = lib().dnagpu_table_from_text(self.h, text, n_bytes, on_device, format, TEXT_MORE if more else 0, C.byref(h), pos_ptr,
                                          cap, C.byref(rep))
        none = lambda v: None if v == U64_MAX else int(v)
        report = TextReport(int(rep.records), int(rep.bases), int(rep.consumed), none(rep.bad_pos), none(rep.bad_record),
                            rep.bad_char if rep.bad_char != b"\0" else b"")
        if rc != OK:
            e = DnaGpuError(rc)
            e.report = report
            raise e
        return Dna(self, h), report

    def table_from_text(self, data, format=TEXT_LINES, more=False, record_pos=False):
        """the raw bytes of a text file of sequences -- TEXT_LINES: one per line, TEXT_FASTA: '>' headers open records -- as
        a resident table -> (Dna, TextReport); record_pos: True for every record's byte offset in report.record_pos, or a cap.
        An input error raises DnaGpuError with the report as .report (dnagpu_table_from_text)"""
        b = bytes(data)
        cap = 0 if record_pos is False else (len(b) + 1 if record_pos is True else int(record_pos))
        pos = np.empty(max(cap, 1), dtype=np.uint64)
        d, report = self._table_from_text(b if b else None, len(b), 0, format, more, pos.ctypes.data if cap else None, cap)
        if record_pos is not False:
            report.record_pos = pos[:min(cap, report.records)].copy()
        return d, report

    def table_from_text_device(self, ptr, n_bytes, format=TEXT_LINES, more=False, dev_record_pos=None, record_cap=0):
        """the same from n_bytes of device memory at any byte alignment; dev_record_pos: record_cap uint64 of device memory"""
        return self._table_from_text(ptr, n_bytes, 1, format, more, dev_record_pos, record_cap)

    def _reads_from_text(self, text, n_bytes, on_device, format, ambiguous, fold_case, min_bases, more, pos_ptr, cap, rec_ptr,
                         off_ptr, seq_cap):
        h, rep = C.c_void_p(), _ReadsReportC()
        opt = _ReadsOptionsC(format, ambiguous, (READS_MORE if more else 0) | (READS_FOLD_CASE if fold_case else 0), 0, min_bases)
        rc = lib().dnagpu_reads_from_text(self.h, text, n_bytes, on_device, C.byref(opt), C.byref(h), pos_ptr, cap, rec_ptr, off_ptr,
                                          seq_cap, C.byref(rep))
        none = lambda v: None if v == U64_MAX else int(v)
        report = ReadsReport(int(rep.records), int(rep.sequences), int(rep.bases), int(rep.consumed), int(rep.ambiguous),
                             int(rep.dropped), int(rep.short_out), none(rep.bad_pos), none(rep.bad_record),
                             rep.bad_char if rep.bad_char != b"\0" else b"")
        if rc != OK:
            e = DnaGpuError(rc)
            e.report = report
            raise e
        return Dna(self, h), report

    def reads_from_text(self, data, format=TEXT_FASTQ, ambiguous=AMBIG_ERROR, fold_case=False, min_bases=0, more=False,
                        record_pos=False, source=False):
        """the raw bytes of a FASTQ (TEXT_FASTQ), FASTA or one-per-line file as a resident table -> (Dna, ReadsReport).
        ambiguous: AMBIG_ERROR / AMBIG_DROP / AMBIG_SPLIT, what an IUPAC ambiguity letter does; fold_case: lower case counts as
        upper; min_bases: shorter sequences are left out.  record_pos: True for every source record's byte offset in
        report.record_pos, or a cap; source: True for report.src_record / report.src_offset of every sequence, or a cap.
        An input error raises DnaGpuError with the report as .report (dnagpu_reads_from_text)"""
        b = bytes(data)
        cap = 0 if record_pos is False else (len(b) + 1 if record_pos is True else int(record_pos))
        seq_cap = 0 if source is False else (len(b) + 1 if source is True else int(source))
        pos = np.empty(max(cap, 1), dtype=np.uint64)
        rec, off = np.empty(max(seq_cap, 1), dtype=np.uint64), np.empty(max(seq_cap, 1), dtype=np.uint64)
        d, report = self._reads_from_text(b if b else None, len(b), 0, format, ambiguous, fold_case, min_bases, more,
                                          pos.ctypes.data if cap else None, cap, rec.ctypes.data if seq_cap else None,
                                          off.ctypes.data if seq_cap else None, seq_cap)
        if record_pos is not False:
            report.record_pos = pos[:min(cap, report.records)].copy()
        if source is not False:
            report.src_record = rec[:min(seq_cap, report.sequences)].copy()
            report.src_offset = off[:min(seq_cap, report.sequences)].copy()
        return d, report

    def reads_from_text_device(self, ptr, n_bytes, format=TEXT_FASTQ, ambiguous=AMBIG_ERROR, fold_case=False, min_bases=0,
                               more=False, dev_record_pos=None, record_cap=0, dev_src_record=None, dev_src_offset=None, seq_cap=0):
        """the same from n_bytes of device memory at any byte alignment; dev_record_pos: record_cap uint64 of device memory,
        dev_src_record / dev_src_offset: seq_cap uint64 of device memory each"""
        return self._reads_from_text(ptr, n_bytes, 1, format, ambiguous, fold_case, min_bases, more, dev_record_pos, record_cap,
                                     dev_src_record, dev_src_offset, seq_cap)

    def table_to_text(self, dna, format, *, crlf=False, line_width=0, prefix=b"", name_base=0, numbers=None, quality=b"I"):
        """the text image of the resident table dna -> TextImage (dnagpu_table_to_text): LINES, FASTA in lines of line_width
        bases (0: one line) or FASTQ with `quality` in every quality line; names are prefix + a number, name_base + s or
        numbers[s].  numbers: a uint64 array of one entry per sequence, or the address of one in device memory"""
        prefix = bytes(prefix)
        opt = _TextOutOptionsC(format=format, flags=TEXT_OUT_CRLF if crlf else 0, line_width=line_width, prefix_len=len(prefix),
                               name_prefix=prefix if prefix else None, name_base=name_base % (1 << 64),
                               quality=bytes(quality)[:1] if quality else b"\0")
        keep = None
        if numbers is not None:
            if isinstance(numbers, int):
                opt.numbers, opt.numbers_on_device = numbers, 1
            else:
                keep = np.ascontiguousarray(numbers, dtype=np.uint64)
                if keep.size != dna.n_sequences:
                    raise ValueError("numbers must hold one entry per sequence")
                opt.numbers = keep.ctypes.data if keep.size else None
        h = C.c_void_p()
        _chk(lib().dnagpu_table_to_text(self.h, dna.h, C.byref(opt), C.byref(h)))
        return TextImage(self, h, dna)

    def table_to_text_named(self, dna, names, format, *, crlf=False, line_width=0, quality=b"I"):
        """table_to_text where the name of sequence s is string s of the Names column (dnagpu_table_to_text_named): FASTA or
        FASTQ.  The image borrows the column as it borrows the table"""
        opt = _TextOutOptionsC(format=format, flags=TEXT_OUT_CRLF if crlf else 0, line_width=line_width, prefix_len=0,
                               name_prefix=None, name_base=0, quality=bytes(quality)[:1] if quality else b"\0")
        h = C.c_void_p()
        _chk(lib().dnagpu_table_to_text_named(self.h, dna.h, names.h, C.byref(opt), C.byref(h)))
        img = TextImage(self, h, dna)
        img.names = names
        return img

    @staticmethod
    def _names_result(rc, rep):
        none = lambda v: None if v == U64_MAX else int(v)
        report = NamesReport(none(rep.bad_pos), none(rep.bad_record), rep.bad_char if rep.bad_char != b"\0" else b"")
        if rc != OK:
            e = DnaGpuError(rc)
            e.report = report
            raise e
        return report

    def names_upload(self, names):
        """a names column from a list of byte strings -> Names; a CR or LF raises DnaGpuError with the NamesReport as .report
        (dnagpu_names_upload)"""
        names = [bytes(x) for x in names]
        off = np.zeros(len(names) + 1, dtype=np.uint64)
        if names:
            off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        return self.names_upload_raw(b"".join(names), off, len(names))

    def names_upload_raw(self, data, offsets, n):
        """the same from the bytes and the n + 1 uint64 offsets as they are (the offsets are checked by the library)"""
        b = bytes(data)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        h, rep = C.c_void_p(), _NamesReportC()
        rc = lib().dnagpu_names_upload(self.h, b if b else None, off.ctypes.data if off.size else None, n, 0, C.byref(h), C.byref(rep))
        self._names_result(rc, rep)
        return Names(self, h)

    def names_upload_device(self, dev_bytes, dev_offsets, n):
        h, rep = C.c_void_p(), _NamesReportC()
        rc = lib().dnagpu_names_upload(self.h, dev_bytes, dev_offsets, n, 1, C.byref(h), C.byref(rep))
        self._names_result(rc, rep)
        return Names(self, h)

    def names_from_text(self, data, format, record_pos, src_record=None, first_word=False):
        """the names of the table that reads_from_text made from the bytes `data` -> Names; record_pos / src_record: what the
        loader reported (src_record None: sequence s is record s).  A CR inside a name raises DnaGpuError with the
        NamesReport as .report (dnagpu_names_from_text)"""
        b = bytes(data)
        pos = np.ascontiguousarray(record_pos, dtype=np.uint64)
        rec = None if src_record is None else np.ascontiguousarray(src_record, dtype=np.uint64)
        ptr = lambda a: None if a is None or not a.size else a.ctypes.data
        return self.names_from_text_device(b if b else None, len(b), format, ptr(pos), pos.size, ptr(rec),
                                           pos.size if rec is None else rec.size, first_word=first_word, on_device=0)

    def names_from_text_device(self, ptr, n_bytes, format, dev_record_pos, n_records, dev_src_record, n_seqs, first_word=False,
                               on_device=1):
        """the same from n_bytes of device memory at any byte alignment; the two arrays in device memory"""
        h, rep = C.c_void_p(), _NamesReportC()
        rc = lib().dnagpu_names_from_text(self.h, ptr, n_bytes, on_device, format, NAMES_FIRST_WORD if first_word else 0,
                                          dev_record_pos, n_records, dev_src_record, n_seqs, C.byref(h), C.byref(rep))
        self._names_result(rc, rep)
        return Names(self, h)

    def names_take(self, names, ids, on_device=False):
        """the names of dna_take(table, ids): string i of the result is string ids[i] of names -> Names; on_device: ids =
        (dev_ids, n)"""
        h = C.c_void_p()
        if on_device:
            _chk(lib().dnagpu_names_take(self.h, names.h, ids[0], ids[1], 1, C.byref(h)))
            return Names(self, h)
        a = np.ascontiguousarray(ids, dtype=np.uint64)
        _chk(lib().dnagpu_names_take(self.h, names.h, a.ctypes.data if a.size else None, a.size, 0, C.byref(h)))
        return Names(self, h)

    @staticmethod
    def _quals_result(rc, h, rep):
        none = lambda v: None if v == U64_MAX else int(v)
        report = QualsReport(int(rep.records), none(rep.bad_pos), none(rep.bad_record), rep.bad_char if rep.bad_char != b"\0" else b"")
        if rc != OK:
            e = DnaGpuError(rc)
            e.report = report
            raise e
        return report

    def quals_upload(self, data):
        """a quality column from Phred+33 bytes -> Quals; a byte outside 33 .. 126 raises DnaGpuError with the QualsReport
        as .report (dnagpu_quals_upload)"""
        b = bytes(data)
        h, rep = C.c_void_p(), _QualsReportC()
        rc = lib().dnagpu_quals_upload(self.h, b if b else None, len(b), 0, C.byref(h), C.byref(rep))
        self._quals_result(rc, h, rep)
        return Quals(self, h)

    def quals_upload_device(self, ptr, n):
        h, rep = C.c_void_p(), _QualsReportC()
        rc = lib().dnagpu_quals_upload(self.h, ptr, n, 1, C.byref(h), C.byref(rep))
        self._quals_result(rc, h, rep)
        return Quals(self, h)

    def quals_from_fastq(self, data, table, src_record=None, src_offset=None):
        """the quality column of the table that reads_from_text made from the FASTQ bytes `data` -> (Quals, QualsReport);
        src_record / src_offset: what the loader reported for every sequence (None: sequence s is record s, offset 0).  An
        input error raises DnaGpuError with the report as .report (dnagpu_quals_from_fastq)"""
        b = bytes(data)
        rec = None if src_record is None else np.ascontiguousarray(src_record, dtype=np.uint64)
        off = None if src_offset is None else np.ascontiguousarray(src_offset, dtype=np.uint64)
        if rec is not None and off is not None and (rec.size != table.n_sequences or off.size != table.n_sequences):
            raise ValueError("src_record and src_offset must hold one entry per sequence")
        ptr = lambda a: None if a is None else (a.ctypes.data if a.size else self._one.ctypes.data)
        return self.quals_from_fastq_device(b if b else None, len(b), table, ptr(rec), ptr(off), on_device=0)

    _one = np.zeros(1, dtype=np.uint64)

    def quals_from_fastq_device(self, ptr, n_bytes, table, dev_src_record=None, dev_src_offset=None, on_device=1):
        """the same from n_bytes of device memory at any byte alignment; the src arrays in device memory"""
        h, rep = C.c_void_p(), _QualsReportC()
        rc = lib().dnagpu_quals_from_fastq(self.h, ptr, n_bytes, on_device, table.h, dev_src_record, dev_src_offset, C.byref(h),
                                           C.byref(rep))
        report = self._quals_result(rc, h, rep)
        return Quals(self, h), report

    def quals_take(self, table, quals, ids, flip=None, on_device=False):
        """the column of dna_take(table, ids, flip): the qualities of the sequences ids, reversed where flipped -> Quals"""
        h = C.c_void_p()
        if on_device:
            _chk(lib().dnagpu_quals_take(self.h, table.h, quals.h, ids[0], flip, ids[1], 1, C.byref(h)))
            return Quals(self, h)
        a = np.ascontiguousarray(ids, dtype=np.uint64)
        f = None if flip is None else np.ascontiguousarray(np.asarray(flip) != 0, dtype=np.uint8)
        if f is not None and f.size != a.size:
            raise ValueError("flip must hold one flag per id")
        _chk(lib().dnagpu_quals_take(self.h, table.h, quals.h, a.ctypes.data if a.size else None,
                                     f.ctypes.data if f is not None and f.size else None, a.size, 0, C.byref(h)))
        return Quals(self, h)

    def quals_gather(self, quals, first, length, flip=None, on_device=False):
        """the column of dna_gather(dna, first, length, flip) -> Quals; on_device: first = (dev_first, n), length and flip
        device pointers"""
        h = C.c_void_p()
        if on_device:
            _chk(lib().dnagpu_quals_gather(self.h, quals.h, first[0], length, flip, first[1], 1, C.byref(h)))
            return Quals(self, h)
        a = np.ascontiguousarray(first, dtype=np.uint64)
        b = np.ascontiguousarray(length, dtype=np.uint64)
        f = None if flip is None else np.ascontiguousarray(np.asarray(flip) != 0, dtype=np.uint8)
        if b.size != a.size or (f is not None and f.size != a.size):
            raise ValueError("first, length and flip must be of one size")
        _chk(lib().dnagpu_quals_gather(self.h, quals.h, a.ctypes.data if a.size else None, b.ctypes.data if b.size else None,
                                       f.ctypes.data if f is not None and f.size else None, a.size, 0, C.byref(h)))
        return Quals(self, h)

    def quals_trim(self, table, quals, cut_front=0, cut_tail=0, min_bases=0, min_mean_q=0, low_q=0, low_frac=(0, 0), cap=None,
                   want=True):
        """quality trimming and filtering of every sequence of table, whose column quals is -> TrimResult
        (dnagpu_quals_trim).  low_frac = (low_num, low_den): passes iff low * low_den <= low_num * len, (x, 0) = no such
        test; cap: at most so many passing sequences are written (None: all); want=False: the report only"""
        n = table.n_sequences
        cap = n if cap is None else int(cap)
        opt = _QualsTrimOptionsC(cut_front, cut_tail, min_mean_q, low_q, low_frac[0], low_frac[1], min_bases, 0)
        rep = _QualsTrimReportC()
        per = [np.empty(max(n, 1), dtype=np.uint64) for _ in range(4)] if want else [None] * 4
        seg = [np.empty(max(cap, 1), dtype=np.uint64) for _ in range(3)] if want else [None] * 3
        ptr = lambda a: None if a is None else a.ctypes.data
        _chk(lib().dnagpu_quals_trim(self.h, table.h, quals.h, C.byref(opt), *[ptr(a) for a in per], *[ptr(a) for a in seg],
                                     cap if want else 0, 0, C.byref(rep)))
        r = TrimResult(**{f: int(getattr(rep, f)) for f in _TRIM_REPORT_FIELDS})
        if want:
            r.first, r.length, r.qsum, r.low = (a[:n] for a in per)
            m = min(r.passed, cap)
            r.seg_seq, r.seg_first, r.seg_len = (a[:m] for a in seg)
        return r

    def quals_trim_device(self, table, quals, opt, dev_per=(None,) * 4, dev_seg=(None,) * 3, cap=0):
        """the same with every output in device memory: dev_per = (first, len, qsum, low), dev_seg = (seq, first, len)
        pointers or None; opt: the keyword arguments of quals_trim as a dict -> TrimResult with the counters only"""
        lf = opt.get("low_frac", (0, 0))
        o = _QualsTrimOptionsC(opt.get("cut_front", 0), opt.get("cut_tail", 0), opt.get("min_mean_q", 0), opt.get("low_q", 0), lf[0], lf[1],
                               opt.get("min_bases", 0), 0)
        rep = _QualsTrimReportC()
        _chk(lib().dnagpu_quals_trim(self.h, table.h, quals.h, C.byref(o), *dev_per, *dev_seg, cap, 1, C.byref(rep)))
        return TrimResult(**{f: int(getattr(rep, f)) for f in _TRIM_REPORT_FIELDS})

    @staticmethod
    def _adapters_args(adapters, err, min_overlap, min_bases, flags):
        texts = [a.encode() if isinstance(a, str) else bytes(a) for a in adapters]
        arr = (C.c_char_p * max(len(texts), 1))(*texts)
        return arr, len(texts), _AdaptersOptionsC(err[0], err[1], min_overlap, flags, min_bases, 0)

    @staticmethod
    def _adapters_result(rep):
        r = AdaptersResult(**{f: int(getattr(rep, f)) for f in _ADAPTERS_REPORT_FIELDS})
        r.per_adapter = [int(x) for x in rep.per_adapter]
        return r

    def dna_adapters(self, dna, adapters, seg_first=None, seg_len=None, seg_seq=None, n_segs=None, err=(0, 1), min_overlap=1,
                     min_bases=0, flags=0, cap=None, want=True):
        """the 3' adapter cut of the segments (seg_first[i], seg_len[i]) of dna's stream -- both None: of every sequence of
        the table -- under the adapters (texts of the qkmer alphabet), the error rate err = (num, den) and min_overlap ->
        AdaptersResult (dnagpu_dna_adapters).  seg_seq: ids carried to pass_seq (None: i); cap: at most so many passing
        segments are written (None: all); want=False: the report only"""
        f = None if seg_first is None else np.ascontiguousarray(seg_first, dtype=np.uint64)
        ln = None if seg_len is None else np.ascontiguousarray(seg_len, dtype=np.uint64)
        sq = None if seg_seq is None else np.ascontiguousarray(seg_seq, dtype=np.uint64)
        n = int(n_segs) if n_segs is not None else (f.size if f is not None else ln.size if ln is not None else dna.n_sequences)
        for a in (f, ln, sq):
            if a is not None and a.size != n:
                raise ValueError("seg_first, seg_len and seg_seq must hold one entry per segment")
        cap = n if cap is None else int(cap)
        arr, n_ad, opt = self._adapters_args(adapters, err, min_overlap, min_bases, flags)
        rep = _AdaptersReportC()
        per = [np.empty(max(n, 1), dtype=np.uint64) for _ in range(3)] if want else [None] * 3
        seg = [np.empty(max(cap, 1), dtype=np.uint64) for _ in range(3)] if want else [None] * 3
        ptr = lambda a: None if a is None else (a.ctypes.data if a.size else self._one.ctypes.data)
        _chk(lib().dnagpu_dna_adapters(self.h, dna.h, arr, n_ad, C.byref(opt), ptr(sq), ptr(f), ptr(ln), n, 0, *[ptr(a) for a in per],
                                       *[ptr(a) for a in seg], cap if want else 0, 0, C.byref(rep)))
        r = self._adapters_result(rep)
        if want:
            r.out_len, r.out_adapter, r.out_mismatch = (a[:n] for a in per)
            m = min(r.passed, cap)
            r.pass_seq, r.pass_first, r.pass_len = (a[:m] for a in seg)
        return r

    def dna_adapters_device(self, dna, adapters, n_segs, dev_in=(None,) * 3, in_on_device=1, dev_per=(None,) * 3, dev_pass=(None,) * 3,
                            cap=0, out_on_device=1, err=(0, 1), min_overlap=1, min_bases=0, flags=0):
        """the same over raw pointers: dev_in = (seg_seq, seg_first, seg_len), dev_per = (out_len, out_adapter, out_mismatch),
        dev_pass = (pass_seq, pass_first, pass_len), each a pointer or None, in device memory where the flag beside it says so
        -> AdaptersResult with the counters only"""
        arr, n_ad, opt = self._adapters_args(adapters, err, min_overlap, min_bases, flags)
        rep = _AdaptersReportC()
        _chk(lib().dnagpu_dna_adapters(self.h, dna.h, arr, n_ad, C.byref(opt), *dev_in, n_segs, in_on_device, *dev_per, *dev_pass, cap,
                                       out_on_device, C.byref(rep)))
        return self._adapters_result(rep)

    def unpack(self, dna, first=0, count=None):
        if count is None:
            count = dna.n_bases - first
        buf = C.create_string_buffer(max(count, 1))
        _chk(lib().dnagpu_dna_unpack(self.h, dna.h, first, count, buf, 0))
        return buf.raw[:count].decode()

    def unpack_device(self, dna, first, count, dev_text):
        """bases [first, first+count) as `count` characters into device memory (any byte alignment)"""
        _chk(lib().dnagpu_dna_unpack(self.h, dna.h, first, count, dev_text, 1))

    def dna_revcomp(self, dna, first=0, count=None):
        """bases [first, first+count) of dna reverse-complemented -> a new Dna"""
        if count is None:
            count = dna.n_bases - first
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_revcomp(self.h, dna.h, first, count, C.byref(h)))
        return Dna(self, h)

    def dna_take(self, dna, ids, flip=None, on_device=False):
        """the sequences ids (global, 0-based, any order, repeats allowed) of the resident table dna as a new resident table
        -> Dna; flip: one flag per id, non-zero = that sequence reverse-complemented.  host: arrays; on_device: ids =
        (dev_ids, n) of uint64 -- what SeqHits.select(on_device=True) leaves in dev_seq -- and flip a device pointer of n
        uint8 or None"""
        if on_device:
            return self.dna_take_device(dna, ids[0], ids[1], flip)
        a = np.ascontiguousarray(ids, dtype=np.uint64)
        f = None if flip is None else np.ascontiguousarray(np.asarray(flip) != 0, dtype=np.uint8)
        if f is not None and f.size != a.size:
            raise ValueError("flip must hold one flag per id")
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_take(self.h, dna.h, a.ctypes.data if a.size else None, f.ctypes.data if f is not None and f.size else None,
                                   a.size, 0, C.byref(h)))
        return Dna(self, h)

    def dna_take_device(self, dna, dev_ids, n, dev_flip=None):
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_take(self.h, dna.h, dev_ids, dev_flip, n, 1, C.byref(h)))
        return Dna(self, h)

    def dna_gather(self, dna, first, length, flip=None, on_device=False):
        """segments [first[i], first[i] + length[i]) of dna's stream, back to back, as a new resident table of one sequence
        per segment -> Dna; flip as in dna_take.  host: arrays; on_device: first = (dev_first, n), length and flip device
        pointers"""
        if on_device:
            return self.dna_gather_device(dna, first[0], length, first[1], flip)
        a = np.ascontiguousarray(first, dtype=np.uint64)
        b = np.ascontiguousarray(length, dtype=np.uint64)
        f = None if flip is None else np.ascontiguousarray(np.asarray(flip) != 0, dtype=np.uint8)
        if b.size != a.size or (f is not None and f.size != a.size):
            raise ValueError("first, length and flip must be of one size")
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_gather(self.h, dna.h, a.ctypes.data if a.size else None, b.ctypes.data if b.size else None,
                                     f.ctypes.data if f is not None and f.size else None, a.size, 0, C.byref(h)))
        return Dna(self, h)

    def dna_gather_device(self, dna, dev_first, dev_len, n, dev_flip=None):
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_gather(self.h, dna.h, dev_first, dev_len, dev_flip, n, 1, C.byref(h)))
        return Dna(self, h)

    def from_wire_device(self, dev_wire, wire_bytes):
        """dna_recv from a wire image in device memory (8-byte aligned) -> Dna"""
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_from_wire(self.h, dev_wire, wire_bytes, 1, C.byref(h)))
        return Dna(self, h)

    def to_wire_device(self, dna, dev_wire, wire_cap):
        """dna_send into device memory (8-byte aligned, wire_cap bytes of room)"""
        _chk(lib().dnagpu_dna_to_wire(self.h, dna.h, dev_wire, wire_cap, 1))

    def kmers_to_text_device(self, dev_keys, n, k, dev_text):
        """n keys in device memory -> n records of k characters + NUL in device memory"""
        _chk(lib().dnagpu_kmers_to_text(self.h, dev_keys, n, k, dev_text, 1))

    def from_wire(self, wire):
        """dna_recv on the device: the binary wire image (bytes) -> Dna"""
        b = bytes(wire)
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_from_wire(self.h, b, len(b), 0, C.byref(h)))
        return Dna(self, h)

    def to_wire(self, dna):
        """dna_send on the device: Dna -> the binary wire image (bytes)"""
        n = lib().dnagpu_dna_wire_size(dna.n_bases)
        buf = C.create_string_buffer(int(n))
        _chk(lib().dnagpu_dna_to_wire(self.h, dna.h, buf, n, 0))
        return buf.raw

    def kmers_to_text(self, keys, k):
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        buf = C.create_string_buffer(max(a.size * (k + 1), 1))
        _chk(lib().dnagpu_kmers_to_text(self.h, a.ctypes.data, a.size, k, buf, 0))
        raw = buf.raw
        return [raw[i * (k + 1): i * (k + 1) + k].decode() for i in range(a.size)]

    def synth(self, seed, n_bases, motif_len=0):
        h = C.c_void_p()
        _chk(lib().dnagpu_dna_synth(self.h, seed, n_bases, motif_len, C.byref(h)))
        return Dna(self, h)

    # ---- generate_kmers
    def generate_kmers(self, dna, k, first=0, count=None):
        total = kmer_count(dna.n_bases, k)
        if count is None:
            count = max(total - first, 0)
        out = np.empty(max(count, 1), dtype=np.uint64)
        _chk(lib().dnagpu_generate_kmers(self.h, dna.h, k, first, count, out.ctypes.data, 0))
        return out[:count]

    def generate_kmers_device(self, dna, k, first, count, dev_out):
        _chk(lib().dnagpu_generate_kmers(self.h, dna.h, k, first, count, dev_out, 1))

    def generate_kmers_filtered(self, dna, k, flt, first=0, count=None, cap=None, want_keys=True,
                                want_pos=True):
        """-> (keys, positions, n_total_matches)"""
        total = kmer_count(dna.n_bases, k)
        if count is None:
            count = max(total - first, 0)
        if cap is None:
            cap = count
        keys = np.empty(max(cap, 1), dtype=np.uint64) if want_keys else None
        pos = np.empty(max(cap, 1), dtype=np.uint64) if want_pos else None
        n = C.c_uint64()
        _chk(lib().dnagpu_generate_kmers_filtered(
            self.h, dna.h, k, C.byref(flt.c), first, count,
            keys.ctypes.data if want_keys else None, pos.ctypes.data if want_pos else None,
            cap, C.byref(n), 0))
        m = min(n.value, cap)
        return (keys[:m] if want_keys else None, pos[:m] if want_pos else None, n.value)

    def count_matches_device(self, dna, k, flt, first, count, dev_keys=None, dev_pos=None, cap=0):
        n = C.c_uint64()
        _chk(lib().dnagpu_generate_kmers_filtered(self.h, dna.h, k, C.byref(flt.c), first, count,
                                                  dev_keys, dev_pos, cap, C.byref(n), 1))
        return n.value

    def generate_kmers_table(self, dna, k, flt=None, first=0, count=None, cap=None, want_keys=True, want_seq=True,
                             want_pos=True):
        """rows of a table made resident with Dna.set_sequences (FROM table, LATERAL generate_kmers(sequence, k) [WHERE flt])
        among stream rows [first, first + count), in table order -> (keys, seq, pos, n_total)"""
        total = kmer_count(dna.n_bases, k)
        if count is None:
            count = max(total - first, 0)
        if cap is None:
            cap = count
        arrs = [np.empty(max(cap, 1), dtype=np.uint64) if w else None for w in (want_keys, want_seq, want_pos)]
        n = C.c_uint64()
        _chk(lib().dnagpu_generate_kmers_table(
            self.h, dna.h, k, C.byref(flt.c) if flt is not None else None, first, count,
            *[a.ctypes.data if a is not None else None for a in arrs], cap, C.byref(n), 0))
        m = min(n.value, cap)
        return tuple(a[:m] if a is not None else None for a in arrs) + (n.value,)

    def generate_kmers_table_device(self, dna, k, flt, first, count, dev_keys=None, dev_seq=None, dev_pos=None, cap=0):
        """the same into device memory (8-byte aligned addresses or None) -> n_total"""
        n = C.c_uint64()
        _chk(lib().dnagpu_generate_kmers_table(self.h, dna.h, k, C.byref(flt.c) if flt is not None else None, first, count,
                                               dev_keys, dev_seq, dev_pos, cap, C.byref(n), 1))
        return n.value

    # ---- GROUP BY
    def count_kmers(self, dna, k, first=0, count=None):
        total = kmer_count(dna.n_bases, k)
        if count is None:
            count = max(total - first, 0)
        h = C.c_void_p()
        _chk(lib().dnagpu_count_kmers(self.h, dna.h, k, first, count, C.byref(h)))
        return Hist(self, h)

    def count_kmers_unordered(self, dna, k, first=0, count=None):
        """same groups, order unspecified (as PostgreSQL's GROUP BY): long k-mers go through super-k-mer partitioning"""
        total = kmer_count(dna.n_bases, k)
        if count is None:
            count = max(total - first, 0)
        h = C.c_void_p()
        _chk(lib().dnagpu_count_kmers_unordered(self.h, dna.h, k, first, count, C.byref(h)))
        return Hist(self, h)

    def count_kmers_batch(self, dna, seq_starts, k):
        """GROUP BY over a table of sequences (test.sql:140-150): dna = the sequences back to back, seq_starts = the first
        base of each + the total (n_seqs + 1 entries)"""
        st = np.ascontiguousarray(seq_starts, dtype=np.uint64)
        h = C.c_void_p()
        _chk(lib().dnagpu_count_kmers_batch(self.h, dna.h, st.ctypes.data_as(u64p), max(len(st) - 1, 0), k, C.byref(h)))
        return Hist(self, h)

    def count_kmers_table(self, dna, k):
        """the same over a table made resident with Dna.set_sequences: nothing crosses the bus per count"""
        h = C.c_void_p()
        _chk(lib().dnagpu_count_kmers_table(self.h, dna.h, k, C.byref(h)))
        return Hist(self, h)

    def table_hits(self, dna, acc, canonical=False, min_count=1, max_count=U64_MAX, seq_first=0, seq_count=None):
        """for every sequence of [seq_first, seq_first + seq_count) of the resident table dna (seq_count=None: all from
        seq_first on): its rows and how many of them are groups of the Accumulator acc with min_count <= count <= max_count
        (canonical: looked up by the canonical form of the key) -> SeqHits (free it)"""
        if seq_count is None:
            seq_count = dna.n_sequences - seq_first
        out = C.c_void_p()
        _chk(lib().dnagpu_table_hits(self.h, dna.h, acc.h, HITS_CANONICAL if canonical else 0, min_count, max_count, seq_first,
                                     seq_count, C.byref(out)))
        return SeqHits(self, out)

    def table_profile(self, dna, k, canonical=False, seq_first=0, seq_count=None, out_counts_dev=None, out_rows_dev=None):
        """the k-mer profile of every sequence of [seq_first, seq_first + seq_count) of the resident table dna (seq_count=None:
        all from seq_first on), k <= 6 -> (counts uint32[n, 4^k], rows uint64[n]): counts[i, key] = the rows of sequence
        seq_first + i whose key is `key` (canonical: under their canonical form).  With out_counts_dev (device memory of
        n * 4^k uint32, 4-byte aligned) the result is written there instead, the rows to out_rows_dev (n uint64, or None) ->
        None"""
        if seq_count is None:
            seq_count = dna.n_sequences - seq_first
        flags = PROFILE_CANONICAL if canonical else 0
        fn = lib().dnagpu_table_profile
        if out_counts_dev is not None:
            _chk(fn(self.h, dna.h, k, flags, seq_first, seq_count, out_counts_dev, out_rows_dev, 1))
            return None
        width = profile_width(k)
        counts = np.empty((max(seq_count, 0), width), dtype=np.uint32)
        rows = np.empty(max(seq_count, 0), dtype=np.uint64)
        _chk(fn(self.h, dna.h, k, flags, seq_first, seq_count, counts.ctypes.data, rows.ctypes.data, 0))
        return counts, rows

    def dna_equals(self, a, b):
        """dna = dna (dna.c:334-350) of two device-resident values: the same number of bases and every base equal -> bool"""
        eq = C.c_int(-1)
        _chk(lib().dnagpu_dna_equals(self.h, a.h, b.h, C.byref(eq)))
        return bool(eq.value)

    def table_classes(self, dna):
        """the classes of equal sequences of the resident table dna -> SeqClasses (free it before dna)"""
        out = C.c_void_p()
        _chk(lib().dnagpu_table_classes(self.h, dna.h, C.byref(out)))
        return SeqClasses(self, out, dna)

    def accumulator(self, k):
        """an empty k-mer accumulator on this context (dnagpu_acc_create): add histograms batch by batch, 64-bit counts"""
        return Accumulator(self, k)

    # ---- the unordered count in two halves (rows on several GPUs: sharded.count_sharded_exchange_records)
    def sk_buckets(self, global_rows, k):
        return int(lib().dnagpu_sk_buckets(self.h, global_rows, k))

    def sk_records(self, dna, k, first, count, global_rows):
        """super-k-mer records of rows [first, first+count), grouped by coarse bucket -> Records"""
        r = C.c_void_p()
        _chk(lib().dnagpu_sk_records(self.h, dna.h, k, first, count, global_rows, C.byref(r)))
        return Records(self, r)

    def count_records(self, pieces, k, global_rows):
        """pieces: [(device pointer, n_records, bucket)] -> Hist (unordered) of the k-mers in them"""
        n = len(pieces)
        ptrs = (C.c_void_p * max(n, 1))(*[C.c_void_p(int(p[0])) for p in pieces])
        lens = np.asarray([int(p[1]) for p in pieces], dtype=np.uint64)
        bks = np.asarray([int(p[2]) for p in pieces], dtype=np.uint32)
        h = C.c_void_p()
        _chk(lib().dnagpu_count_records(self.h, ptrs, lens.ctypes.data_as(u64p), bks.ctypes.data_as(C.POINTER(C.c_uint32)), n, k,
                                        global_rows, C.byref(h)))
        return Hist(self, h)

    def count_kmers_owned(self, dna, k, owner, n_owners, first=0, count=None):
        total = kmer_count(dna.n_bases, k)
        if count is None:
            count = max(total - first, 0)
        h = C.c_void_p()
        _chk(lib().dnagpu_count_kmers_owned(self.h, dna.h, k, first, count, owner, n_owners, C.byref(h)))
        return Hist(self, h)

    def count_keys_device(self, dev_keys, n, k):
        h = C.c_void_p()
        _chk(lib().dnagpu_count_keys(self.h, dev_keys, n, k, C.byref(h)))
        return Hist(self, h)

    def count_keys_device_in_range(self, dev_keys, n, k, key_min, key_max):
        h = C.c_void_p()
        _chk(lib().dnagpu_count_keys_in_range(self.h, dev_keys, n, k, key_min, key_max, C.byref(h)))
        return Hist(self, h)

    def partition_kmers(self, dna, k, first, count, n_owners):
        """-> (device pointer to `count` keys grouped by owner, offsets[n_owners+1])"""
        ptr = C.c_void_p()
        offs = np.zeros(n_owners + 1, dtype=np.uint64)
        _chk(lib().dnagpu_partition_kmers(self.h, dna.h, k, first, count, n_owners, C.byref(ptr),
                                          offs.ctypes.data_as(u64p)))
        return ptr.value, offs

    def buffer_alloc(self, nbytes):
        p = C.c_void_p()
        _chk(lib().dnagpu_buffer_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def buffer_free(self, ptr):
        lib().dnagpu_buffer_free(self.h, ptr)

    def download_bytes(self, ptr, n):
        out = np.empty(max(n, 1), dtype=np.uint8)
        _chk(lib().dnagpu_buffer_download(self.h, ptr, n, out.ctypes.data))
        return out[:n]

    def upload_bytes(self, ptr, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint8)
        _chk(lib().dnagpu_buffer_upload(self.h, ptr, a.ctypes.data, a.size))

    def download_u64(self, ptr, n):
        out = np.empty(max(n, 1), dtype=np.uint64)
        _chk(lib().dnagpu_buffer_download(self.h, ptr, n * 8, out.ctypes.data))
        return out[:n]

    def upload_u64(self, ptr, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        _chk(lib().dnagpu_buffer_upload(self.h, ptr, a.ctypes.data, a.size * 8))

    # ---- batched operators
    def kmer_hash(self, keys):
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.empty(max(k.size, 1), dtype=np.uint32)
        _chk(lib().dnagpu_kmer_hash(self.h, k.ctypes.data, k.size, out.ctypes.data, 0))
        return out[:k.size]

    def kmer_hash_device(self, dev_keys, n, dev_out):
        """n keys in device memory -> n uint32 hashes in device memory"""
        _chk(lib().dnagpu_kmer_hash(self.h, dev_keys, n, dev_out, 1))

    def kmer_strand(self, keys, k, mode=STRAND_CANONICAL, want_flipped=True):
        """rc (STRAND_REVCOMP) or the canonical form (STRAND_CANONICAL) of every key -> (out uint64[], flipped bool[] or None)"""
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.empty(max(a.size, 1), dtype=np.uint64)
        fl = np.empty(max(a.size, 1), dtype=np.uint8) if want_flipped else None
        _chk(lib().dnagpu_kmer_strand(self.h, a.ctypes.data, a.size, k, mode, out.ctypes.data,
                                      fl.ctypes.data if want_flipped else None, 0))
        return out[:a.size], (fl[:a.size].astype(bool) if want_flipped else None)

    def kmer_strand_device(self, dev_keys, n, k, mode, dev_out, dev_flipped=None):
        """n keys in device memory -> n keys in device memory (dev_out may be dev_keys), n uint8 flags if dev_flipped"""
        _chk(lib().dnagpu_kmer_strand(self.h, dev_keys, n, k, mode, dev_out, dev_flipped, 1))

    def kmer_match_device(self, dev_keys, n, k, flt, dev_flags):
        """n keys in device memory -> n uint8 flags in device memory"""
        _chk(lib().dnagpu_kmer_match(self.h, dev_keys, n, k, C.byref(flt.c), dev_flags, 1))

    # ---- the index over a stored kmer column
    def kmer_index(self, keys, k):
        """CREATE INDEX over a column of n keys of k bases (host array; row id = position) -> KmerIndex"""
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        h = C.c_void_p()
        _chk(lib().dnagpu_kmer_index_build(self.h, a.ctypes.data if a.size else None, a.size, k, 0, C.byref(h)))
        return KmerIndex(self, h)

    def kmer_index_device(self, dev_keys, n, k):
        """the same over n keys already in device memory (left as they are)"""
        h = C.c_void_p()
        _chk(lib().dnagpu_kmer_index_build(self.h, dev_keys, n, k, 1, C.byref(h)))
        return KmerIndex(self, h)

    def kmer_match(self, keys, k, flt):
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.empty(max(a.size, 1), dtype=np.uint8)
        _chk(lib().dnagpu_kmer_match(self.h, a.ctypes.data, a.size, k, C.byref(flt.c), out.ctypes.data, 0))
        return out[:a.size].astype(bool)


MULTI_AUTO, MULTI_RCCL, MULTI_COPY = 0, 1, 2
MULTI_OPT_PARTS, MULTI_OPT_EMULATE_LINK_GBS, MULTI_OPT_PROBE_OWNER, MULTI_OPT_EXCHANGE_RCCL = 1, 2, 3, 4


class _BorrowedContext(Context):
    """a rank's context owned by a Multi: same methods, never destroyed from here"""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)
        # the same test-harness switch as Context: the rank contexts of a Multi are created in C, so the poison flag
        # is set on them here
        self._base_debug = _env_debug()
        if self._base_debug:
            self.set_debug(0)

    def close(self):
        self.h = None


class Multi:
    """dnagpu_multi: N ranks driven from this one process (dnagpu_count_multi)."""

    def __init__(self, devices, transport=MULTI_AUTO):
        n = len(devices)
        arr = (C.c_int * n)(*devices)
        self.h = C.c_void_p()
        _chk(lib().dnagpu_multi_init(arr, n, transport, C.byref(self.h)))
        self.n = n
        self.ranks = [_BorrowedContext(lib().dnagpu_multi_ctx(self.h, r)) for r in range(n)]

    @property
    def transport(self):
        return lib().dnagpu_multi_transport(self.h).decode()

    @property
    def exchange_transport(self):
        """what the most recent count moved its data between ranks with ("peer-copy", "rccl-sendrecv", ...)"""
        return lib().dnagpu_multi_exchange_transport(self.h).decode()

    @property
    def rccl_ranks(self):
        return int(lib().dnagpu_multi_rccl_ranks(self.h))

    def set_exchange_rccl(self, mode):
        """record exchange of count_unordered: 0 = peer copies, 1 = ncclSend / ncclRecv, 2 = own pieces through RCCL too"""
        _chk(lib().dnagpu_multi_set_option(self.h, MULTI_OPT_EXCHANGE_RCCL, float(mode)))

    def rank_phase_times(self, rank):
        """device phases of rank `rank` in the most recent count_unordered: its record pass, then its owner phase"""
        pt = _PhaseTimes()
        _chk(lib().dnagpu_multi_last_phase_times(self.h, rank, C.byref(pt)))
        return [(pt.names[i].decode(), float(pt.ms[i])) for i in range(pt.n)]

    def set_parts(self, parts):
        """bucket groups per owner of count_unordered's pipelined exchange (1 = no overlap)"""
        _chk(lib().dnagpu_multi_set_option(self.h, MULTI_OPT_PARTS, float(parts)))

    def emulate_link(self, gb_per_s):
        """rehearsal on one device: inbound pieces are held to this rate on the transfer stream (0 = off)"""
        _chk(lib().dnagpu_multi_set_option(self.h, MULTI_OPT_EMULATE_LINK_GBS, float(gb_per_s)))

    def probe_owner(self, owner):
        """rehearsal on one device: only this owner pulls and counts (-1: all), so that last_times() are its own"""
        _chk(lib().dnagpu_multi_set_option(self.h, MULTI_OPT_PROBE_OWNER, float(owner)))

    def last_times(self):
        t = _MultiTimes()
        _chk(lib().dnagpu_multi_last_times(self.h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in _MultiTimes._fields_}

    def upload(self, words, n_bases):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        d = C.c_void_p()
        _chk(lib().dnagpu_multi_dna_upload(self.h, w.ctypes.data_as(u64p), n_bases, C.byref(d)))
        return d

    def synth(self, seed, n_bases, motif_len=0):
        d = C.c_void_p()
        _chk(lib().dnagpu_multi_dna_synth(self.h, seed, n_bases, motif_len, C.byref(d)))
        return d

    def dna_free(self, d):
        lib().dnagpu_multi_dna_free(self.h, d)

    def count(self, mdna, k, first=0, count=None):
        """-> [Hist per rank]; their ascending downloads concatenated in rank order are the global result"""
        n_bases = int(lib().dnagpu_multi_dna_length(mdna))
        total = kmer_count(n_bases, k)
        if count is None:
            count = max(total - first, 0)
        hs = (C.c_void_p * self.n)()
        _chk(lib().dnagpu_count_multi(self.h, mdna, k, first, count, hs))
        return [Hist(self.ranks[r], C.c_void_p(hs[r])) for r in range(self.n)]

    def count_unordered(self, mdna, k, first=0, count=None):
        """-> [Hist per rank]: the same groups, disjoint between ranks, in no key order (long k-mers: record exchange)"""
        n_bases = int(lib().dnagpu_multi_dna_length(mdna))
        total = kmer_count(n_bases, k)
        if count is None:
            count = max(total - first, 0)
        hs = (C.c_void_p * self.n)()
        _chk(lib().dnagpu_count_multi_unordered(self.h, mdna, k, first, count, hs))
        return [Hist(self.ranks[r], C.c_void_p(hs[r])) for r in range(self.n)]

    def close(self):
        if self.h:
            lib().dnagpu_multi_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
