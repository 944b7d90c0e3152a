"""ctypes binding of libdna_glue.so (glue/dna_glue.h): the reference's SQL-visible functions on the
k-mer path, spelled the way test.sql spells them.  An ereport(ERROR) becomes GlueError(text)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class GlueError(Exception):
    pass


class _Kmer(C.Structure):
    _fields_ = [("length", C.c_int32), ("bit_sequence", C.c_uint64)]


class _Qkmer(C.Structure):
    _fields_ = [("sequence", C.c_char * 33)]


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libdna_glue.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: run __graft_entry__.build()")
        L = C.CDLL(path)
        vp = C.c_void_p
        L.dna_glue_errmsg.restype = C.c_char_p
        L.dna_in.restype = vp
        L.dna_in.argtypes = [C.c_char_p]
        L.dna_out.restype = vp
        L.dna_out.argtypes = [vp]
        L.dna_free.argtypes = [vp]
        L.dna_length.restype = C.c_uint64
        L.dna_length.argtypes = [vp]
        L.kmer_in.restype = C.c_bool
        L.kmer_in.argtypes = [C.c_char_p, C.POINTER(_Kmer)]
        L.kmer_out.restype = vp
        L.kmer_out.argtypes = [C.POINTER(_Kmer)]
        L.qkmer_in.restype = C.c_bool
        L.qkmer_in.argtypes = [C.c_char_p, C.POINTER(_Qkmer)]
        L.kmer_eq.restype = C.c_bool
        L.kmer_eq.argtypes = [C.POINTER(_Kmer)] * 2
        L.kmer_ne.restype = C.c_bool
        L.kmer_ne.argtypes = [C.POINTER(_Kmer)] * 2
        L.kmer_hash.restype = C.c_int32
        L.kmer_hash.argtypes = [C.POINTER(_Kmer)]
        L.starts_with.argtypes = [C.POINTER(_Kmer)] * 2
        L.contains.argtypes = [C.POINTER(_Qkmer), C.POINTER(_Kmer)]
        L.generate_kmers_begin.restype = vp
        L.generate_kmers_begin.argtypes = [vp, C.c_int]
        L.generate_kmers_where_begin.restype = vp
        L.generate_kmers_where_begin.argtypes = [vp, C.c_int, C.c_char, C.POINTER(_Kmer), C.POINTER(_Qkmer)]
        L.generate_kmers_next.restype = C.c_bool
        L.generate_kmers_next.argtypes = [vp, C.POINTER(_Kmer)]
        L.generate_kmers_failed.restype = C.c_bool
        L.generate_kmers_failed.argtypes = [vp]
        L.generate_kmers_end.argtypes = [vp]
        L.count_kmers_begin.restype = vp
        L.count_kmers_begin.argtypes = [vp, C.c_int]
        L.count_kmers_next.restype = C.c_bool
        L.count_kmers_next.argtypes = [vp, C.POINTER(_Kmer), C.POINTER(C.c_int64)]
        L.count_kmers_totals.argtypes = [vp] + [C.POINTER(C.c_int64)] * 3
        L.count_kmers_end.argtypes = [vp]
        L.dna_send.restype = vp
        L.dna_send.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.dna_recv.restype = vp
        L.dna_recv.argtypes = [C.c_char_p, C.c_size_t]
        L.kmer_send.restype = None
        L.kmer_send.argtypes = [C.POINTER(_Kmer), C.c_char_p]
        L.kmer_recv.restype = C.c_bool
        L.kmer_recv.argtypes = [C.c_char_p, C.POINTER(_Kmer)]
        L.dna_glue_shutdown.restype = None
        L.dna_glue_set_gpus.restype = None
        L.dna_glue_set_gpus.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
        L.count_kmers_agg_begin.restype = vp
        L.count_kmers_agg_begin.argtypes = [C.c_int]
        L.count_kmers_agg_begin_canonical.restype = vp
        L.count_kmers_agg_begin_canonical.argtypes = [C.c_int]
        L.reverse_complement.restype = vp
        L.reverse_complement.argtypes = [vp]
        L.kmer_reverse_complement.restype = None
        L.kmer_reverse_complement.argtypes = [C.POINTER(_Kmer)] * 2
        L.kmer_canonical.restype = None
        L.kmer_canonical.argtypes = [C.POINTER(_Kmer)] * 2
        L.count_kmers_agg_add.restype = C.c_bool
        L.count_kmers_agg_add.argtypes = [vp, vp]
        L.count_kmers_agg_next.restype = C.c_bool
        L.count_kmers_agg_next.argtypes = [vp, C.POINTER(_Kmer), C.POINTER(C.c_int64)]
        L.count_kmers_agg_failed.restype = C.c_bool
        L.count_kmers_agg_failed.argtypes = [vp]
        L.count_kmers_agg_totals.restype = None
        L.count_kmers_agg_totals.argtypes = [vp] + [C.POINTER(C.c_int64)] * 3
        L.count_kmers_agg_end.restype = None
        L.count_kmers_agg_end.argtypes = [vp]
        L.dna_glue_set_agg_flush_bases.restype = None
        L.dna_glue_set_agg_flush_bases.argtypes = [C.c_uint64]
        L.count_kmers_top_begin.restype = vp
        L.count_kmers_top_begin.argtypes = [vp, C.c_int, C.c_int64]
        L.count_kmers_spectrum.restype = C.c_bool
        L.count_kmers_spectrum.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
        L.count_kmers_agg_top.restype = C.c_bool
        L.count_kmers_agg_top.argtypes = [vp, C.c_int64]
        L.count_kmers_ordered_begin.restype = vp
        L.count_kmers_ordered_begin.argtypes = [vp, C.c_int, C.c_bool]
        L.count_kmers_agg_order.restype = C.c_bool
        L.count_kmers_agg_order.argtypes = [vp, C.c_bool]
        L.count_kmers_join_begin.restype = vp
        L.count_kmers_join_begin.argtypes = [vp, vp, C.c_char]
        L.count_kmers_join_next.restype = C.c_bool
        L.count_kmers_join_next.argtypes = [vp, C.POINTER(_Kmer), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.count_kmers_join_failed.restype = C.c_bool
        L.count_kmers_join_failed.argtypes = [vp]
        L.count_kmers_join_stats.restype = None
        L.count_kmers_join_stats.argtypes = [vp] + [C.POINTER(C.c_int64)] * 4
        L.count_kmers_join_end.restype = None
        L.count_kmers_join_end.argtypes = [vp]
        L.table_kmers_begin.restype = vp
        L.table_kmers_begin.argtypes = [C.c_int, C.c_char, C.POINTER(_Kmer), C.POINTER(_Qkmer)]
        L.table_kmers_add.restype = C.c_bool
        L.table_kmers_add.argtypes = [vp, vp]
        L.table_kmers_next.restype = C.c_bool
        L.table_kmers_next.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(_Kmer)]
        L.table_kmers_failed.restype = C.c_bool
        L.table_kmers_failed.argtypes = [vp]
        L.table_kmers_end.restype = None
        L.table_kmers_end.argtypes = [vp]
        L.table_hits_begin.restype = vp
        L.table_hits_begin.argtypes = [vp, C.c_bool, C.c_int64, C.c_int64]
        L.table_hits_add.restype = C.c_bool
        L.table_hits_add.argtypes = [vp, vp]
        L.table_hits_next.restype = C.c_bool
        L.table_hits_next.argtypes = [vp] + [C.POINTER(C.c_int64)] * 3
        L.table_hits_totals.restype = None
        L.table_hits_totals.argtypes = [vp] + [C.POINTER(C.c_int64)] * 3
        L.table_hits_failed.restype = C.c_bool
        L.table_hits_failed.argtypes = [vp]
        L.table_hits_end.restype = None
        L.table_hits_end.argtypes = [vp]
        L.table_profile_begin.restype = vp
        L.table_profile_begin.argtypes = [C.c_int, C.c_bool]
        L.table_profile_add.restype = C.c_bool
        L.table_profile_add.argtypes = [vp, vp]
        L.table_profile_next.restype = C.c_bool
        L.table_profile_next.argtypes = [vp] + [C.POINTER(C.c_int64)] * 3
        L.table_profile_width.restype = C.c_int64
        L.table_profile_width.argtypes = [vp]
        L.table_profile_failed.restype = C.c_bool
        L.table_profile_failed.argtypes = [vp]
        L.table_profile_end.restype = None
        L.table_profile_end.argtypes = [vp]
        L.dna_equals.restype = C.c_bool
        L.dna_equals.argtypes = [vp, vp]
        L.dna_ne.restype = C.c_bool
        L.dna_ne.argtypes = [vp, vp]
        L.table_distinct_begin.restype = vp
        L.table_distinct_begin.argtypes = []
        L.table_distinct_add.restype = C.c_bool
        L.table_distinct_add.argtypes = [vp, vp]
        L.table_distinct_next.restype = C.c_bool
        L.table_distinct_next.argtypes = [vp] + [C.POINTER(C.c_int64)] * 2
        L.table_distinct_failed.restype = C.c_bool
        L.table_distinct_failed.argtypes = [vp]
        L.table_distinct_end.restype = None
        L.table_distinct_end.argtypes = [vp]
        L.table_match_begin.restype = vp
        L.table_match_begin.argtypes = []
        for side in ("build", "probe"):
            getattr(L, f"table_match_add_{side}").restype = C.c_bool
            getattr(L, f"table_match_add_{side}").argtypes = [vp, vp]
        L.table_match_next.restype = C.c_bool
        L.table_match_next.argtypes = [vp] + [C.POINTER(C.c_int64)] * 3
        L.table_match_failed.restype = C.c_bool
        L.table_match_failed.argtypes = [vp]
        L.table_match_end.restype = None
        L.table_match_end.argtypes = [vp]
        L.table_screen_begin.restype = vp
        L.table_screen_begin.argtypes = [vp, C.c_bool] + [C.c_int64] * 6
        L.table_screen_add.restype = C.c_bool
        L.table_screen_add.argtypes = [vp, vp]
        L.table_screen_next.restype = C.c_bool
        L.table_screen_next.argtypes = [vp] + [C.POINTER(C.c_int64)] * 3 + [C.POINTER(vp)]
        L.table_screen_failed.restype = C.c_bool
        L.table_screen_failed.argtypes = [vp]
        L.table_screen_end.restype = None
        L.table_screen_end.argtypes = [vp]
        L.copy_dna_begin.restype = vp
        L.copy_dna_begin.argtypes = [C.c_int]
        L.copy_dna_feed.restype = C.c_bool
        L.copy_dna_feed.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_bool]
        L.copy_dna_next.restype = C.c_bool
        L.copy_dna_next.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
        L.copy_reads_begin.restype = vp
        L.copy_reads_begin.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_uint64]
        L.copy_reads_next.restype = C.c_bool
        L.copy_reads_next.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.copy_dna_failed.restype = C.c_bool
        L.copy_dna_failed.argtypes = [vp]
        L.copy_dna_end.restype = None
        L.copy_dna_end.argtypes = [vp]
        L.dna_glue_set_copy_chunk_bytes.restype = None
        L.dna_glue_set_copy_chunk_bytes.argtypes = [C.c_uint64]
        L.copy_dna_to_begin.restype = vp
        L.copy_dna_to_begin.argtypes = [C.c_int, C.c_uint32, C.c_bool]
        for f in (L.copy_dna_to_add, L.copy_dna_to_finish, L.copy_dna_to_next, L.copy_dna_to_failed):
            f.restype = C.c_bool
        L.copy_dna_to_add.argtypes = [vp, vp]
        L.copy_dna_to_finish.argtypes = [vp]
        L.copy_dna_to_next.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.copy_dna_to_failed.argtypes = [vp]
        L.copy_dna_to_end.restype = None
        L.copy_dna_to_end.argtypes = [vp]
        L.trim_reads_begin.restype = vp
        L.trim_reads_begin.argtypes = [C.c_int, C.c_uint, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.trim_reads_next.restype = C.c_bool
        L.trim_reads_next.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(vp)]
        L.trim_reads_add_adapter.restype = C.c_bool
        L.trim_reads_add_adapter.argtypes = [vp, C.c_char_p]
        L.trim_reads_adapter_options.restype = C.c_bool
        L.trim_reads_adapter_options.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint]
        L.copy_reads_to_begin.restype = vp
        L.copy_reads_to_begin.argtypes = [C.c_bool]
        for f in (L.copy_reads_to_add, L.copy_reads_to_finish, L.copy_reads_to_next, L.copy_reads_to_failed):
            f.restype = C.c_bool
        L.copy_reads_to_add.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
        L.copy_reads_to_finish.argtypes = [vp]
        L.copy_reads_to_next.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.copy_reads_to_failed.argtypes = [vp]
        L.copy_reads_to_end.restype = None
        L.copy_reads_to_end.argtypes = [vp]
        L.copy_reads_keep_names.restype = C.c_bool
        L.copy_reads_keep_names.argtypes = [vp, C.c_bool]
        L.copy_reads_name.restype = vp
        L.copy_reads_name.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.copy_reads_to_add_named.restype = C.c_bool
        L.copy_reads_to_add_named.argtypes = [vp, vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.copy_dna_to_add_named.restype = C.c_bool
        L.copy_dna_to_add_named.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
        L.kmer_index_create.restype = vp
        L.kmer_index_create.argtypes = [C.POINTER(_Kmer), C.c_uint64]
        L.kmer_index_rows.restype = C.c_uint64
        L.kmer_index_rows.argtypes = [vp]
        for f in (L.kmer_index_scan_eq, L.kmer_index_scan_starts_with):
            f.restype = C.c_int64
            f.argtypes = [vp, C.POINTER(_Kmer), C.POINTER(C.POINTER(C.c_int64))]
        L.kmer_index_scan_contains.restype = C.c_int64
        L.kmer_index_scan_contains.argtypes = [vp, C.POINTER(_Qkmer), C.POINTER(C.POINTER(C.c_int64))]
        L.kmer_index_insert.restype = C.c_int64
        L.kmer_index_insert.argtypes = [vp, C.POINTER(_Kmer), C.c_uint64]
        L.kmer_index_delete.restype = C.c_int64
        L.kmer_index_delete.argtypes = [vp, C.POINTER(C.c_int64), C.c_uint64]
        L.kmer_index_end.restype = None
        L.kmer_index_end.argtypes = [vp]
        _LIB = L
    return _LIB


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _err():
    return GlueError(lib().dna_glue_errmsg().decode())


def _take_str(p):
    if not p:
        raise _err()
    s = C.string_at(p).decode()
    _libc.free(p)
    return s


class dna:
    """the `dna` type: dna('ATCG') is dna_in"""

    def __init__(self, text=None, p=None):
        self.p = p if p is not None else lib().dna_in(text.encode())
        if not self.p:
            raise _err()

    def __str__(self):
        return _take_str(lib().dna_out(self.p))

    def send(self):
        """dna_send: the binary wire image"""
        n = C.c_size_t()
        buf = lib().dna_send(self.p, C.byref(n))
        if not buf:
            raise _err()
        raw = C.string_at(buf, n.value)
        _libc.free(buf)
        return raw

    @classmethod
    def recv(cls, wire):
        """dna_recv"""
        b = bytes(wire)
        p = lib().dna_recv(b, len(b))
        if not p:
            raise _err()
        return cls(p=p)

    def __len__(self):
        return int(lib().dna_length(self.p))

    def __del__(self):
        if getattr(self, "p", None) and _LIB is not None:
            _LIB.dna_free(self.p)
            self.p = None


class kmer:
    def __init__(self, text=None, c=None):
        self.c = c if c is not None else _Kmer()
        if text is not None and not lib().kmer_in(text.encode(), C.byref(self.c)):
            raise _err()

    def __str__(self):
        return _take_str(lib().kmer_out(C.byref(self.c)))

    def __eq__(self, other):                       # kmer = kmer
        return bool(lib().kmer_eq(C.byref(self.c), C.byref(other.c)))

    def __ne__(self, other):
        return bool(lib().kmer_ne(C.byref(self.c), C.byref(other.c)))

    def __hash__(self):
        return kmer_hash(self)

    def send(self):
        buf = C.create_string_buffer(12)
        lib().kmer_send(C.byref(self.c), buf)
        return buf.raw

    @classmethod
    def recv(cls, wire):
        c = _Kmer()
        if not lib().kmer_recv(bytes(wire), C.byref(c)):
            raise _err()
        return cls(c=c)


class qkmer:
    def __init__(self, text):
        self.c = _Qkmer()
        if not lib().qkmer_in(text.encode(), C.byref(self.c)):
            raise _err()

    def __str__(self):
        return self.c.sequence.decode()


def kmer_hash(k):
    return int(lib().kmer_hash(C.byref(k.c)))


def reverse_complement(x):
    """reverse_complement(dna) -> dna, reverse_complement(kmer) -> kmer"""
    if isinstance(x, dna):
        p = lib().reverse_complement(x.p)
        if not p:
            raise _err()
        return dna(p=p)
    out = _Kmer()
    lib().kmer_reverse_complement(C.byref(x.c), C.byref(out))
    return kmer(c=out)


def canonical(k):
    """canonical(kmer): whichever of k and its reverse complement comes first as text under A < T < C < G"""
    out = _Kmer()
    lib().kmer_canonical(C.byref(k.c), C.byref(out))
    return kmer(c=out)


def starts_with(k, prefix):                        # k ^@ prefix
    r = lib().starts_with(C.byref(k.c), C.byref(prefix.c))
    if r < 0:
        raise _err()
    return bool(r)


def contains(pattern, k):                          # pattern @> k
    r = lib().contains(C.byref(pattern.c), C.byref(k.c))
    if r < 0:
        raise _err()
    return bool(r)


def _drain(g):
    if not g:
        raise _err()
    rows, c = [], _Kmer()
    while lib().generate_kmers_next(g, C.byref(c)):
        rows.append(kmer(c=_Kmer(c.length, c.bit_sequence)))
    failed = lib().generate_kmers_failed(g)
    lib().generate_kmers_end(g)
    if failed:
        raise _err()
    return rows


def generate_kmers(d, k):
    """SELECT generate_kmers(d, k)"""
    if isinstance(d, str):
        d = dna(d)                                 # the implicit text -> dna cast of test.sql:46-47
    return _drain(lib().generate_kmers_begin(d.p, k))


def generate_kmers_where(d, k, op, rhs):
    """SELECT k.kmer FROM generate_kmers(d, k) AS k(kmer) WHERE <op>, op in '=', '^@', '@>'"""
    if isinstance(d, str):
        d = dna(d)
    if op == "@>":
        return _drain(lib().generate_kmers_where_begin(d.p, k, b"@", None, C.byref(rhs.c)))
    return _drain(lib().generate_kmers_where_begin(d.p, k, b"=" if op == "=" else b"^", C.byref(rhs.c), None))


def set_gpus(devices, transport=0):
    """count_kmers shards over these HIP devices from now on (dna_glue_set_gpus); [0] = single GPU"""
    n = len(devices)
    lib().dna_glue_set_gpus(n, (C.c_int * n)(*devices), transport)


def count_kmers(d, k, _begin=None):
    """SELECT k.kmer, count(*) FROM generate_kmers(d, k) AS k(kmer) GROUP BY k.kmer
    -> ([(kmer, count)...], (total, distinct, unique))"""
    if isinstance(d, str):
        d = dna(d)
    c = _begin(d) if _begin else lib().count_kmers_begin(d.p, k)
    if not c:
        raise _err()
    rows, km, cnt = [], _Kmer(), C.c_int64()
    while lib().count_kmers_next(c, C.byref(km), C.byref(cnt)):
        rows.append((kmer(c=_Kmer(km.length, km.bit_sequence)), cnt.value))
    t, dd, u = C.c_int64(), C.c_int64(), C.c_int64()
    lib().count_kmers_totals(c, C.byref(t), C.byref(dd), C.byref(u))
    lib().count_kmers_end(c)
    return rows, (t.value, dd.value, u.value)


def count_kmers_top(d, k, n):
    """SELECT k.kmer, count(*) FROM generate_kmers(d, k) AS k(kmer) GROUP BY k.kmer ORDER BY count(*) DESC LIMIT n
    (test.sql:95; sorted and cut on the device) -> ([(kmer, count)...] in that order, (total, distinct, unique) of all groups)"""
    return count_kmers(d, k, _begin=lambda dd: lib().count_kmers_top_begin(dd.p, k, n))


def count_kmers_ordered(d, k, descending=True):
    """SELECT k.kmer, count(*) FROM generate_kmers(d, k) AS k(kmer) GROUP BY k.kmer ORDER BY count(*) [DESC] -- no LIMIT
    (test.sql:95 as written; ranked on the device) -> ([(kmer, count)...] every group in that order, (total, distinct, unique))"""
    return count_kmers(d, k, _begin=lambda dd: lib().count_kmers_ordered_begin(dd.p, k, descending))


def count_kmers_spectrum(d, k, n_bins):
    """the k-mer spectrum of generate_kmers(d, k): [groups with count 1, with count 2, ..., with count >= n_bins]"""
    if isinstance(d, str):
        d = dna(d)
    c = lib().count_kmers_begin(d.p, k)
    if not c:
        raise _err()
    try:
        bins = (C.c_int64 * max(n_bins, 1))()
        if not lib().count_kmers_spectrum(c, bins, n_bins):
            raise _err()
        return [int(b) for b in bins[:n_bins]]
    finally:
        lib().count_kmers_end(c)


def set_agg_flush_bases(n):
    """bases per batch of count_kmers_agg (dna_glue_set_agg_flush_bases; default 2^30)"""
    lib().dna_glue_set_agg_flush_bases(int(n))


def count_kmers_agg_top(rows, k, n):
    """count_kmers_agg ... ORDER BY count(*) DESC LIMIT n: the rows in that order, the totals over all groups"""
    return count_kmers_agg(rows, k, _top=n)


def count_kmers_agg_ordered(rows, k, descending=True):
    """count_kmers_agg ... ORDER BY count(*) [DESC] without a LIMIT: every group in that order, the totals"""
    return count_kmers_agg(rows, k, _order=descending)


def count_kmers_agg_canonical(rows, k):
    """count_kmers_agg with a kmer and its reverse complement as one group (count_kmers_agg_begin_canonical)"""
    return count_kmers_agg(rows, k, _canonical=True)


def count_kmers_agg(rows, k, _top=None, _order=None, _canonical=False):
    """SELECT k.kmer, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) GROUP BY k.kmer
    (test.sql:140-150) through the aggregate: rows = the table's `dna` values (or their text)
    -> ([(kmer, count)...], (total, distinct, unique))"""
    a = (lib().count_kmers_agg_begin_canonical if _canonical else lib().count_kmers_agg_begin)(k)
    if not a:
        raise _err()
    try:
        if _top is not None and not lib().count_kmers_agg_top(a, _top):
            raise _err()
        if _order is not None and not lib().count_kmers_agg_order(a, bool(_order)):
            raise _err()
        for r in rows:
            if isinstance(r, str):
                r = dna(r)
            if not lib().count_kmers_agg_add(a, r.p):
                raise _err()
        out, km, cnt = [], _Kmer(), C.c_int64()
        while lib().count_kmers_agg_next(a, C.byref(km), C.byref(cnt)):
            out.append((kmer(c=_Kmer(km.length, km.bit_sequence)), cnt.value))
        if lib().count_kmers_agg_failed(a):
            raise _err()
        t, dd, u = C.c_int64(), C.c_int64(), C.c_int64()
        lib().count_kmers_agg_totals(a, C.byref(t), C.byref(dd), C.byref(u))
        return out, (t.value, dd.value, u.value)
    finally:
        lib().count_kmers_agg_end(a)


class count_kmers_table_agg:
    """one count_kmers_agg aggregate kept open (count_kmers_agg_begin .. _end): rows added with add(), the groups read
    with groups(), two of them paired with count_kmers_join()"""

    def __init__(self, k, rows=(), canonical=False):
        self.a = (lib().count_kmers_agg_begin_canonical if canonical else lib().count_kmers_agg_begin)(k)
        if not self.a:
            raise _err()
        self.keep = []
        for r in rows:
            self.add(r)

    def add(self, row):
        row = row if isinstance(row, dna) else dna(row)
        self.keep.append(row)
        if not lib().count_kmers_agg_add(self.a, row.p):
            raise _err()

    def groups(self):
        """the remaining FINALFUNC rows: [(kmer, count)]"""
        out = []
        km, cnt = _Kmer(), C.c_int64()
        while lib().count_kmers_agg_next(self.a, C.byref(km), C.byref(cnt)):
            out.append((kmer(c=_Kmer(km.length, km.bit_sequence)), cnt.value))
        if lib().count_kmers_agg_failed(self.a):
            raise _err()
        return out

    def end(self):
        if self.a:
            lib().count_kmers_agg_end(self.a)
            self.a = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.end()


def count_kmers_join(left, right, kind="i"):
    """two count_kmers_table_agg paired on the k-mer: kind 'i' JOIN / INTERSECT, 'a' EXCEPT / NOT IN, 'l' LEFT JOIN ->
    ([(kmer, count_left, count_right)], (rows, sum_left, sum_right, sum_min))"""
    j = lib().count_kmers_join_begin(left.a, right.a, kind.encode()[:1] or b"\0")
    if not j:
        raise _err()
    try:
        out = []
        km, cl, cr = _Kmer(), C.c_int64(), C.c_int64()
        while lib().count_kmers_join_next(j, C.byref(km), C.byref(cl), C.byref(cr)):
            out.append((kmer(c=_Kmer(km.length, km.bit_sequence)), cl.value, cr.value))
        if lib().count_kmers_join_failed(j):
            raise _err()
        st = [C.c_int64() for _ in range(4)]
        lib().count_kmers_join_stats(j, *[C.byref(x) for x in st])
        return out, tuple(x.value for x in st)
    finally:
        lib().count_kmers_join_end(j)


def table_kmers(rows, k, op=None, rhs=None):
    """SELECT <row ordinal>, k.kmer FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) [WHERE <op>]
    (test.sql:172-176; op in None, '=', '^@', '@>' as generate_kmers_where): rows = the table's `dna` values (or their text)
    -> (seq int64[], pos int64[], keys uint64[]) in table order"""
    import numpy as np
    if op is None:
        t = lib().table_kmers_begin(k, b"\0", None, None)
    elif op == "@>":
        t = lib().table_kmers_begin(k, b"@", None, C.byref(rhs.c))
    else:
        t = lib().table_kmers_begin(k, b"=" if op == "=" else b"^", C.byref(rhs.c), None)
    if not t:
        raise _err()
    try:
        for r in rows:
            if isinstance(r, str):
                r = dna(r)
            if not lib().table_kmers_add(t, r.p):
                raise _err()
        seq, pos, keys = [], [], []
        sq, ps, km = C.c_int64(), C.c_int64(), _Kmer()
        while lib().table_kmers_next(t, C.byref(sq), C.byref(ps), C.byref(km)):
            seq.append(sq.value)
            pos.append(ps.value)
            keys.append(km.bit_sequence)
        if lib().table_kmers_failed(t):
            raise _err()
        return np.array(seq, dtype=np.int64), np.array(pos, dtype=np.int64), np.array(keys, dtype=np.uint64)
    finally:
        lib().table_kmers_end(t)


def table_hits(rows, set_agg, canonical=False, min_count=1, max_count=None):
    """SELECT <row ordinal>, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) g JOIN counts_b b ON g.kmer =
    b.kmer WHERE b.count BETWEEN min_count AND max_count GROUP BY 1, with the rows that have no hit too: rows = the table's
    `dna` values (or their text), set_agg = a count_kmers_table_agg (None: the NULL aggregate's ERROR) -> (seq int64[],
    rows int64[], hits int64[], (sum rows, sum hits, rows with a hit)) in table order"""
    import numpy as np
    t = lib().table_hits_begin(set_agg.a if set_agg is not None else None, bool(canonical), int(min_count),
                               -1 if max_count is None else int(max_count))
    if not t:
        raise _err()
    try:
        for r in rows:
            if isinstance(r, str):
                r = dna(r)
            if not lib().table_hits_add(t, r.p):
                raise _err()
        seq, nrows, hits = [], [], []
        sq, nr, nh = C.c_int64(), C.c_int64(), C.c_int64()
        while lib().table_hits_next(t, C.byref(sq), C.byref(nr), C.byref(nh)):
            seq.append(sq.value)
            nrows.append(nr.value)
            hits.append(nh.value)
        if lib().table_hits_failed(t):
            raise _err()
        tot = [C.c_int64() for _ in range(3)]
        lib().table_hits_totals(t, *[C.byref(x) for x in tot])
        return (np.array(seq, dtype=np.int64), np.array(nrows, dtype=np.int64), np.array(hits, dtype=np.int64),
                tuple(x.value for x in tot))
    finally:
        lib().table_hits_end(t)


def table_profile(rows, k, canonical=False):
    """SELECT <row ordinal>, k.kmer, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) GROUP BY
    1, 2 as a dense profile, k <= 6: rows = the table's `dna` values (or their text).  A generator of (seq, rows, counts
    int64[4^k]) in table order; counts[key] = the row's k-mers of that key (canonical: under their canonical form).  A bad k
    raises before the first row is taken."""
    import numpy as np
    t = lib().table_profile_begin(int(k), bool(canonical))
    if not t:
        raise _err()

    def gen():
        try:
            for r in rows:
                if isinstance(r, str):
                    r = dna(r)
                if not lib().table_profile_add(t, r.p):
                    raise _err()
            width = lib().table_profile_width(t)
            sq, nr = C.c_int64(), C.c_int64()
            while True:
                counts = np.empty(width, dtype=np.int64)
                if not lib().table_profile_next(t, C.byref(sq), C.byref(nr), counts.ctypes.data_as(C.POINTER(C.c_int64))):
                    break
                yield sq.value, nr.value, counts
            if lib().table_profile_failed(t):
                raise _err()
        finally:
            lib().table_profile_end(t)
    return gen()


def _as_dna(x):
    return dna(x) if isinstance(x, str) else x


def equals(a, b):                                  # dna = dna (equals, dna.c:352-367); host: a length test and a memcmp
    a, b = _as_dna(a), _as_dna(b)
    return bool(lib().dna_equals(a.p, b.p))


def dna_ne(a, b):                                  # dna <> dna (dna_ne, dna.c:369-384)
    a, b = _as_dna(a), _as_dna(b)
    return bool(lib().dna_ne(a.p, b.p))


def table_distinct(rows):
    """SELECT min(<row ordinal>), count(*) FROM t GROUP BY sequence: rows = the table's `dna` values (or their text) ->
    (seq int64[], copies int64[]): the ordinal of the first row of every distinct content, ascending, and how many rows equal
    it.  The rows are ONE resident table: more than 2^32 - 1 bases is an ERROR."""
    import numpy as np
    t = lib().table_distinct_begin()
    if not t:
        raise _err()
    try:
        for r in rows:
            r = _as_dna(r)
            if not lib().table_distinct_add(t, r.p):
                raise _err()
        seq, copies = [], []
        sq, cp = C.c_int64(), C.c_int64()
        while lib().table_distinct_next(t, C.byref(sq), C.byref(cp)):
            seq.append(sq.value)
            copies.append(cp.value)
        if lib().table_distinct_failed(t):
            raise _err()
        return np.array(seq, dtype=np.int64), np.array(copies, dtype=np.int64)
    finally:
        lib().table_distinct_end(t)


def table_match(probe_rows, build_rows):
    """SELECT a.id, min(b.id), count(*) FROM a JOIN b ON a.sequence = b.sequence GROUP BY a.id over row ordinals: the matched
    probe rows only -> (probe_seq int64[], build_seq int64[], copies int64[]) in ascending probe ordinal; build_seq = the
    first build row equal to the probe row, copies = the build rows equal to it.  Either side is ONE resident table."""
    import numpy as np
    t = lib().table_match_begin()
    if not t:
        raise _err()
    try:
        for r in build_rows:
            r = _as_dna(r)
            if not lib().table_match_add_build(t, r.p):
                raise _err()
        for r in probe_rows:
            r = _as_dna(r)
            if not lib().table_match_add_probe(t, r.p):
                raise _err()
        out = ([], [], [])
        vals = [C.c_int64() for _ in range(3)]
        while lib().table_match_next(t, *[C.byref(v) for v in vals]):
            for o, v in zip(out, vals):
                o.append(v.value)
        if lib().table_match_failed(t):
            raise _err()
        return tuple(np.array(o, dtype=np.int64) for o in out)
    finally:
        lib().table_match_end(t)


def table_screen(rows, set_agg, canonical=False, min_count=1, max_count=None, min_hits=0, max_hits=None, frac=(0, 1)):
    """SELECT <row ordinal>, d.sequence, count(*) ... JOIN counts_b b ... GROUP BY 1, 2 HAVING min_hits <= hits <= max_hits AND
    hits / rows >= frac[0] / frac[1]: the rows of the table that pass the screen, themselves.  rows / set_agg / canonical /
    min_count / max_count as table_hits -> (seq int64[], rows int64[], hits int64[], [dna]) in table order"""
    import numpy as np
    t = lib().table_screen_begin(set_agg.a if set_agg is not None else None, bool(canonical), int(min_count),
                                 -1 if max_count is None else int(max_count), int(min_hits),
                                 -1 if max_hits is None else int(max_hits), int(frac[0]), int(frac[1]))
    if not t:
        raise _err()
    try:
        for r in rows:
            if isinstance(r, str):
                r = dna(r)
            if not lib().table_screen_add(t, r.p):
                raise _err()
        seq, nrows, hits, out = [], [], [], []
        sq, nr, nh, p = C.c_int64(), C.c_int64(), C.c_int64(), C.c_void_p()
        while lib().table_screen_next(t, C.byref(sq), C.byref(nr), C.byref(nh), C.byref(p)):
            seq.append(sq.value)
            nrows.append(nr.value)
            hits.append(nh.value)
            out.append(dna(p=p.value))
        if lib().table_screen_failed(t):
            raise _err()
        return np.array(seq, dtype=np.int64), np.array(nrows, dtype=np.int64), np.array(hits, dtype=np.int64), out
    finally:
        lib().table_screen_end(t)


def set_copy_chunk_bytes(n):
    """bytes per chunk of copy_dna (dna_glue_set_copy_chunk_bytes; default 2^26)"""
    lib().dna_glue_set_copy_chunk_bytes(int(n))


def copy_dna(pieces, format=1):
    """COPY ... FROM a text file: pieces = the file's bytes in order, in pieces of any size; format 1 = one sequence per line,
    2 = FASTA -> ([dna], [line]) in file order, line = the 1-based row of the whole file.  An input ERROR raises GlueError with
    the reference's message and .line = the row of the whole file it belongs to"""
    c = lib().copy_dna_begin(int(format))
    if not c:
        raise _err()
    try:
        rows, lines = [], []
        p, ln = C.c_void_p(), C.c_int64()

        def drain():
            while lib().copy_dna_next(c, C.byref(p), C.byref(ln)):
                rows.append(dna(p=p.value))
                lines.append(ln.value)

        def check(ok):
            if not ok:
                e = _err()
                lib().copy_dna_next(c, None, C.byref(ln))
                e.line = ln.value
                raise e
        for piece in pieces:
            b = bytes(piece)
            check(lib().copy_dna_feed(c, b, len(b), False))
            drain()
        check(lib().copy_dna_feed(c, None, 0, True))
        drain()
        return rows, lines
    finally:
        lib().copy_dna_end(c)


def copy_dna_to(rows, fmt, line_width=0, crlf=False):
    """COPY ... TO a text file: the rows (dna) as one sequence per line (1), FASTA in lines of line_width bases (2) or FASTQ
    (3) -> the file's bytes.  FASTA and FASTQ name row r of the COPY r"""
    c = lib().copy_dna_to_begin(int(fmt), int(line_width), bool(crlf))
    if not c:
        raise _err()
    try:
        out = []
        p, n = C.c_void_p(), C.c_size_t()

        def drain():
            while lib().copy_dna_to_next(c, C.byref(p), C.byref(n)):
                out.append(C.string_at(p.value, n.value))
        for row in rows:
            if not lib().copy_dna_to_add(c, _as_dna(row).p):
                raise _err()
            drain()
        if not lib().copy_dna_to_finish(c):
            raise _err()
        drain()
        return b"".join(out)
    finally:
        lib().copy_dna_to_end(c)


def copy_reads(pieces, format=3, ambiguous=0, fold_case=False, min_bases=0):
    """COPY reads (record, start, sequence) FROM a FASTQ (3), FASTA (2) or one-per-line (1) file: pieces = the file's bytes in
    order, in pieces of any size; ambiguous 0 / 1 / 2 = an ambiguity letter is an ERROR / drops its record / splits it ->
    ([dna], [record], [offset]) in file order, record = the 0-based source record of the whole file.  An input ERROR raises
    GlueError with the library's message and .record = the source record it belongs to (-1: none)"""
    c = lib().copy_reads_begin(int(format), int(ambiguous), 2 if fold_case else 0, int(min_bases))
    if not c:
        raise _err()
    try:
        rows, records, offsets = [], [], []
        p, rec, off = C.c_void_p(), C.c_int64(), C.c_int64()

        def drain():
            while lib().copy_reads_next(c, C.byref(p), C.byref(rec), C.byref(off)):
                rows.append(dna(p=p.value))
                records.append(rec.value)
                offsets.append(off.value)

        def check(ok):
            if not ok:
                e = _err()
                lib().copy_reads_next(c, None, C.byref(rec), None)
                e.record = rec.value
                raise e
        for piece in pieces:
            b = bytes(piece)
            check(lib().copy_dna_feed(c, b, len(b), False))
            drain()
        check(lib().copy_dna_feed(c, None, 0, True))
        drain()
        return rows, records, offsets
    finally:
        lib().copy_dna_end(c)


def _set_adapters(c, adapters, adapter_opt):
    """trim_reads_add_adapter for every text of adapters and trim_reads_adapter_options(*adapter_opt) on the handle c;
    adapter_opt = (err_num, err_den, min_overlap, flags) or None: the handle's defaults"""
    for a in adapters or ():
        if not lib().trim_reads_add_adapter(c, a.encode() if isinstance(a, str) else bytes(a)):
            raise _err()
    if adapter_opt is not None and not lib().trim_reads_adapter_options(c, *[int(x) for x in adapter_opt]):
        raise _err()


def trim_reads(pieces, ambiguous=0, fold_case=False, cut_front=0, cut_tail=0, min_bases=0, min_mean_q=0, low_q=0, low_frac=(0, 0),
               adapters=None, adapter_opt=None):
    """FASTQ with its qualities, quality-trimmed and filtered on the device: pieces = the file's bytes in order, in pieces of
    any size -> ([dna], [record], [offset], [quality bytes]) of the passing reads in file order; offset = the index of the
    read's first kept base in its source record's sequence.  With all thresholds 0 it is the plain load with qualities.
    adapters: 3' adapters (qkmer texts) cut behind the quality trim, adapter_opt = (err_num, err_den, min_overlap, flags).  An
    input ERROR raises GlueError with the library's message and .record = the source record it belongs to (-1: none)"""
    c = lib().trim_reads_begin(int(ambiguous), 2 if fold_case else 0, int(cut_front), int(cut_tail), int(min_bases), int(min_mean_q),
                               int(low_q), int(low_frac[0]), int(low_frac[1]))
    if not c:
        raise _err()
    try:
        _set_adapters(c, adapters, adapter_opt)
        rows, records, offsets, quals = [], [], [], []
        p, rec, off, q = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_void_p()

        def drain():
            while lib().trim_reads_next(c, C.byref(p), C.byref(rec), C.byref(off), C.byref(q)):
                rows.append(dna(p=p.value))
                records.append(rec.value)
                offsets.append(off.value)
                quals.append(C.string_at(q.value))
                _libc.free(q.value)

        def check(ok):
            if not ok:
                e = _err()
                lib().trim_reads_next(c, None, C.byref(rec), None, None)
                e.record = rec.value
                raise e
        for piece in pieces:
            b = bytes(piece)
            check(lib().copy_dna_feed(c, b, len(b), False))
            drain()
        check(lib().copy_dna_feed(c, None, 0, True))
        drain()
        return rows, records, offsets, quals
    finally:
        lib().copy_dna_end(c)


def copy_reads_to(rows, quals, crlf=False):
    """rows (dna) with their quality texts (bytes, one per base) -> the FASTQ file's bytes; row r of the COPY is named r"""
    c = lib().copy_reads_to_begin(bool(crlf))
    if not c:
        raise _err()
    try:
        out = []
        p, n = C.c_void_p(), C.c_size_t()

        def drain():
            while lib().copy_reads_to_next(c, C.byref(p), C.byref(n)):
                out.append(C.string_at(p.value, n.value))
        for row, q in zip(rows, quals):
            q = bytes(q)
            if not lib().copy_reads_to_add(c, _as_dna(row).p, q, len(q)):
                raise _err()
            drain()
        if not lib().copy_reads_to_finish(c):
            raise _err()
        drain()
        return b"".join(out)
    finally:
        lib().copy_reads_to_end(c)


def _served_name(c):
    n = C.c_size_t()
    p = lib().copy_reads_name(c, C.byref(n))
    return C.string_at(p, n.value) if p else None


def copy_reads_named(pieces, format=3, ambiguous=0, fold_case=False, min_bases=0, first_word=False):
    """copy_reads where every row carries the name of its source record (copy_reads_keep_names; FASTA or FASTQ) ->
    ([dna], [record], [offset], [name bytes])"""
    c = lib().copy_reads_begin(int(format), int(ambiguous), 2 if fold_case else 0, int(min_bases))
    if not c:
        raise _err()
    try:
        if not lib().copy_reads_keep_names(c, bool(first_word)):
            raise _err()
        rows, records, offsets, names = [], [], [], []
        p, rec, off = C.c_void_p(), C.c_int64(), C.c_int64()

        def drain():
            while lib().copy_reads_next(c, C.byref(p), C.byref(rec), C.byref(off)):
                rows.append(dna(p=p.value))
                records.append(rec.value)
                offsets.append(off.value)
                names.append(_served_name(c))

        def check(ok):
            if not ok:
                e = _err()
                lib().copy_reads_next(c, None, C.byref(rec), None)
                e.record = rec.value
                raise e
        for piece in pieces:
            b = bytes(piece)
            check(lib().copy_dna_feed(c, b, len(b), False))
            drain()
        check(lib().copy_dna_feed(c, None, 0, True))
        drain()
        return rows, records, offsets, names
    finally:
        lib().copy_dna_end(c)


def trim_reads_named(pieces, first_word=False, ambiguous=0, fold_case=False, cut_front=0, cut_tail=0, min_bases=0, min_mean_q=0,
                     low_q=0, low_frac=(0, 0), adapters=None, adapter_opt=None):
    """trim_reads where every passing read carries its own name (copy_reads_keep_names) ->
    ([dna], [record], [offset], [quality bytes], [name bytes])"""
    c = lib().trim_reads_begin(int(ambiguous), 2 if fold_case else 0, int(cut_front), int(cut_tail), int(min_bases), int(min_mean_q),
                               int(low_q), int(low_frac[0]), int(low_frac[1]))
    if not c:
        raise _err()
    try:
        if not lib().copy_reads_keep_names(c, bool(first_word)):
            raise _err()
        _set_adapters(c, adapters, adapter_opt)
        rows, records, offsets, quals, names = [], [], [], [], []
        p, rec, off, q = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_void_p()

        def drain():
            while lib().trim_reads_next(c, C.byref(p), C.byref(rec), C.byref(off), C.byref(q)):
                rows.append(dna(p=p.value))
                records.append(rec.value)
                offsets.append(off.value)
                quals.append(C.string_at(q.value))
                _libc.free(q.value)
                names.append(_served_name(c))

        def check(ok):
            if not ok:
                e = _err()
                lib().trim_reads_next(c, None, C.byref(rec), None, None)
                e.record = rec.value
                raise e
        for piece in pieces:
            b = bytes(piece)
            check(lib().copy_dna_feed(c, b, len(b), False))
            drain()
        check(lib().copy_dna_feed(c, None, 0, True))
        drain()
        return rows, records, offsets, quals, names
    finally:
        lib().copy_dna_end(c)


def copy_reads_to_named(rows, names, quals, crlf=False):
    """rows (dna) with their names and quality texts (bytes each) -> the FASTQ file's bytes, every header the row's own name"""
    c = lib().copy_reads_to_begin(bool(crlf))
    if not c:
        raise _err()
    try:
        out = []
        p, n = C.c_void_p(), C.c_size_t()

        def drain():
            while lib().copy_reads_to_next(c, C.byref(p), C.byref(n)):
                out.append(C.string_at(p.value, n.value))
        for row, nm, q in zip(rows, names, quals):
            nm, q = bytes(nm), bytes(q)
            if not lib().copy_reads_to_add_named(c, _as_dna(row).p, nm, len(nm), q, len(q)):
                raise _err()
            drain()
        if not lib().copy_reads_to_finish(c):
            raise _err()
        drain()
        return b"".join(out)
    finally:
        lib().copy_reads_to_end(c)


def copy_dna_to_named(rows, names, format=2, line_width=0, crlf=False):
    """rows (dna) with their names -> the FASTA (2) or FASTQ (3) file's bytes, every header the row's own name"""
    c = lib().copy_dna_to_begin(int(format), int(line_width), bool(crlf))
    if not c:
        raise _err()
    try:
        out = []
        p, n = C.c_void_p(), C.c_size_t()

        def drain():
            while lib().copy_dna_to_next(c, C.byref(p), C.byref(n)):
                out.append(C.string_at(p.value, n.value))
        for row, nm in zip(rows, names):
            nm = bytes(nm)
            if not lib().copy_dna_to_add_named(c, _as_dna(row).p, nm, len(nm)):
                raise _err()
            drain()
        if not lib().copy_dna_to_finish(c):
            raise _err()
        drain()
        return b"".join(out)
    finally:
        lib().copy_dna_to_end(c)


class kmer_index:
    """CREATE INDEX ... USING spgist (kmer_sequence spgist_kmer_ops) over a stored column (a list of kmer; row id = position),
    then SELECT ... WHERE kmer_sequence <op> rhs as an index scan: scan('=', kmer), scan('^@', kmer), scan('@>', qkmer) ->
    the row ids, ascending (test.sql:156-270)"""

    def __init__(self, column):
        arr = (_Kmer * max(len(column), 1))()
        for i, x in enumerate(column):
            arr[i].length, arr[i].bit_sequence = x.c.length, x.c.bit_sequence
        self.p = lib().kmer_index_create(arr, len(column))
        if not self.p:
            raise _err()

    def __len__(self):
        return int(lib().kmer_index_rows(self.p))

    def scan(self, op, rhs):
        fn = {"=": lib().kmer_index_scan_eq, "^@": lib().kmer_index_scan_starts_with, "@>": lib().kmer_index_scan_contains}[op]
        rows = C.POINTER(C.c_int64)()
        n = fn(self.p, C.byref(rhs.c), C.byref(rows))
        if n < 0:
            raise _err()
        out = [int(rows[i]) for i in range(n)]
        if n:
            _libc.free(C.cast(rows, C.c_void_p))
        return out

    def insert(self, rows):
        """INSERT of a batch of kmer: they become rows first, first + 1, ... -> first"""
        arr = (_Kmer * max(len(rows), 1))()
        for i, x in enumerate(rows):
            arr[i].length, arr[i].bit_sequence = x.c.length, x.c.bit_sequence
        first = lib().kmer_index_insert(self.p, arr, len(rows))
        if first < 0:
            raise _err()
        return int(first)

    def delete(self, rows):
        """VACUUM after DELETE: drops the entries of the listed row ids -> the entries removed"""
        arr = (C.c_int64 * max(len(rows), 1))(*rows)
        n = lib().kmer_index_delete(self.p, arr, len(rows))
        if n < 0:
            raise _err()
        return int(n)

    def end(self):
        if self.p:
            lib().kmer_index_end(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.end()
