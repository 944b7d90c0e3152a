"""The contract of the quality column (dnagpu_quals_* of include/dnagpu.h) as plain Python loops: what the tests of
tests/test_read_quals.py compare the device against.  It runs no code of the project and shares nothing with the C++.

parse(data) -> Parsed: the sequence line and the quality line of every record, or the input error with the lowest offset
(at one offset a length error comes before a character error).  column() places the qualities of a table's sequences,
gather() / take() follow dnagpu_dna_gather / dnagpu_dna_take, cut_points() is cutadapt's two walks written as loops and
trim() dnagpu_quals_trim over a whole table, render() writes the FASTQ image with its quality lines taken from a column."""
import dataclasses

import export_model

BAD_ARG = 5
MSG_TRUNCATED = "truncated FASTQ record"
MSG_LENGTH = "FASTQ quality line length differs from the sequence's"
MSG_CHAR = "invalid FASTQ quality character"
_LENGTH, _CHAR, _TRUNC = 0, 1, 3                                    # the order of errors at equal offsets


@dataclasses.dataclass
class Parsed:
    sequences: list = dataclasses.field(default_factory=list)      # bytes: the sequence line of every record
    qualities: list = dataclasses.field(default_factory=list)      # bytes: its quality line
    error: tuple = None                                            # (offset, record, char bytes)
    message: str = None

    @property
    def records(self):
        return len(self.qualities)


def lines_of(data):
    """(offset, content) of every line.  A line ends at '\\n'; a '\\r' directly before that '\\n' belongs to the terminator; a
    last line without a '\\n' is a line (and a '\\r' at its end is content); text that ends in '\\n' has no extra empty line"""
    out, a = [], 0
    while a < len(data):
        e = a
        while e < len(data) and data[e] != 10:
            e += 1
        if e == len(data):
            out.append((a, data[a:]))
            break
        c = e
        if c > a and data[c - 1] == 13:
            c -= 1
        out.append((a, data[a:c]))
        a = e + 1
    return out


def valid(byte):
    return 33 <= byte <= 126


def parse(data):
    data = bytes(data)
    lines = lines_of(data)
    p = Parsed()
    errors = []                                                    # (offset, order, record, char, message)
    whole = len(lines) // 4
    for r in range(whole):
        (_, seq), (at, qual) = lines[4 * r + 1], lines[4 * r + 3]
        p.sequences.append(seq)
        p.qualities.append(qual)
        if len(qual) != len(seq):
            errors.append((at, _LENGTH, r, b"", MSG_LENGTH))
        for i, byte in enumerate(qual):
            if not valid(byte):
                errors.append((at + i, _CHAR, r, bytes([byte]), MSG_CHAR))
    if len(lines) % 4:
        errors.append((lines[4 * whole][0], _TRUNC, whole, b"", MSG_TRUNCATED))
    if errors:
        at, _, rec, ch, msg = min(errors, key=lambda e: e[:2])
        return Parsed(error=(at, rec, ch), message=msg)
    return p


class SourceError(Exception):
    """an argument error of dnagpu_quals_from_fastq: it has no offset"""


def column(data, lengths, src_record=None, src_offset=None):
    """the column of a table whose sequence s has lengths[s] bases and came from offset src_offset[s] of record src_record[s]
    (both None: record s, offset 0); parse(data) must have succeeded"""
    p = parse(data)
    assert p.error is None
    out = bytearray()
    for s, n in enumerate(lengths):
        r = s if src_record is None else int(src_record[s])
        off = 0 if src_offset is None else int(src_offset[s])
        if r >= p.records or off + n > len(p.qualities[r]):
            raise SourceError(s)
        for i in range(n):
            out.append(p.qualities[r][off + i])
    return bytes(out)


def split(col, starts):
    """the quality text of every sequence of a table with these starts"""
    return [col[int(a):int(b)] for a, b in zip(starts[:-1], starts[1:])]


def gather(col, first, length, flip=None):
    """the column of dnagpu_dna_gather's table: a flipped segment is reversed, qualities have no complement"""
    out = bytearray()
    for i, (a, n) in enumerate(zip(first, length)):
        piece = col[int(a):int(a) + int(n)]
        assert len(piece) == int(n)
        if flip is not None and flip[i]:
            piece = piece[::-1]
        out += piece
    return bytes(out)


def take(col, starts, ids, flip=None):
    return gather(col, [starts[int(i)] for i in ids], [starts[int(i) + 1] - starts[int(i)] for i in ids], flip)


def cut_points(q, F=0, T=0):
    """cutadapt's / BWA's cut points of the Phred values q, each walk over the whole sequence -> (start, stop)"""
    n = len(q)
    start, stop = 0, n
    if F:
        s, best = 0, 0
        for i in range(n):
            s += F - q[i]
            if s < 0:
                break
            if s > best:
                best, start = s, i + 1
    if T:
        s, best = 0, 0
        for i in range(n - 1, -1, -1):
            s += T - q[i]
            if s < 0:
                break
            if s > best:
                best, stop = s, i
    if start >= stop:
        start = stop = 0
    return start, stop


@dataclasses.dataclass
class Trimmed:
    first: list = dataclasses.field(default_factory=list)          # per sequence: stream coordinate of the kept range
    length: list = dataclasses.field(default_factory=list)
    qsum: list = dataclasses.field(default_factory=list)
    low: list = dataclasses.field(default_factory=list)
    seg_seq: list = dataclasses.field(default_factory=list)        # the passing sequences, in table order
    seg_first: list = dataclasses.field(default_factory=list)
    seg_len: list = dataclasses.field(default_factory=list)
    report: dict = None


def trim(col, starts, cut_front=0, cut_tail=0, min_bases=0, min_mean_q=0, low_q=0, low_frac=(0, 0), cap=None):
    """dnagpu_quals_trim over the column col of a table with these starts"""
    t = Trimmed()
    rep = dict(sequences=len(starts) - 1, passed=0, bases_in=int(starts[-1]) if len(starts) else 0, bases_kept=0, cut_front=0,
               cut_tail=0, failed_short=0, failed_mean=0, failed_low=0)
    for s in range(len(starts) - 1):
        a, b = int(starts[s]), int(starts[s + 1])
        q = [byte - 33 for byte in col[a:b]]
        start, stop = cut_points(q, cut_front, cut_tail)
        kept = q[start:stop]
        length, qsum, low = len(kept), sum(kept), sum(1 for v in kept if v < low_q)
        t.first.append(a + start)
        t.length.append(length)
        t.qsum.append(qsum)
        t.low.append(low)
        rep["bases_kept"] += length
        rep["cut_front"] += start
        rep["cut_tail"] += len(q) - stop
        if length == 0 or length < min_bases:
            rep["failed_short"] += 1
        elif qsum < min_mean_q * length:
            rep["failed_mean"] += 1
        elif low_frac[1] != 0 and low * low_frac[1] > low_frac[0] * length:
            rep["failed_low"] += 1
        else:
            rep["passed"] += 1
            if cap is None or len(t.seg_seq) < cap:
                t.seg_seq.append(s)
                t.seg_first.append(a + start)
                t.seg_len.append(length)
    t.report = rep
    return t


def render(records, quals, opt):
    """the FASTQ image of records (str each) under opt (export_model.Options) with the quality line of record s = quals[s]"""
    assert opt.format == export_model.FASTQ
    term = b"\r\n" if opt.crlf else b"\n"
    out = bytearray()
    for s, (seq, q) in enumerate(zip(records, quals)):
        assert len(q) == len(seq)
        out += b"@" + export_model.name(opt, s) + term + seq.encode() + term + b"+" + term + bytes(q) + term
    return bytes(out)
