"""The contract of the names column (dnagpu_names_*, dnagpu_table_to_text_named; include/dnagpu.h) as plain Python loops: what
the tests of tests/test_read_names.py compare the device against.  It runs no code of the project.

names_of(text, format, record_pos, src_record, first_word) -> the name of every sequence, or raises NamesError / SourceError;
take(names, ids) -> the names of the sequences ids; render_named(seqs, names, quals, opt) -> the image of
dnagpu_table_to_text_named, built on export_model's records with the header's name replaced."""
import export_model

FASTA, FASTQ = export_model.FASTA, export_model.FASTQ
MSG_CHAR = "invalid character in a read name"


class SourceError(Exception):
    """a record_pos entry that is not its record's marker inside the text, or a src_record entry that is no record"""


class NamesError(Exception):
    """a '\\r' that remains inside a name: the text offset of the first one in the lowest-numbered sequence, and its record"""

    def __init__(self, pos, record):
        Exception.__init__(self, MSG_CHAR)
        self.pos, self.record = pos, record


def header_span(text, at, first_word):
    """[start, end) of the name whose marker is the byte at `at`"""
    start = at + 1
    end = start
    while end < len(text) and text[end] != 0x0A:                       # the line ends before the first '\n', or at the text's end
        end += 1
    if end < len(text) and end > start and text[end - 1] == 0x0D:      # a '\r' directly before that '\n' is the terminator's
        end -= 1
    if first_word:
        cut = start
        while cut < end and text[cut] not in (0x20, 0x09):
            cut += 1
        end = cut
    return start, end


def names_of(text, format, record_pos, src_record=None, first_word=False):
    text = bytes(text)
    marker = {FASTA: ord(">"), FASTQ: ord("@")}[format]
    if src_record is None:
        src_record = list(range(len(record_pos)))
    spans = []
    for r in src_record:
        if r >= len(record_pos):
            raise SourceError(f"record {r} of {len(record_pos)}")
        at = record_pos[r]
        if at >= len(text) or text[at] != marker:
            raise SourceError(f"record {r} at {at}")
        spans.append(header_span(text, at, first_word))
    for (start, end), r in zip(spans, src_record):
        for i in range(start, end):
            if text[i] == 0x0D:
                raise NamesError(i, r)
    return [text[a:b] for a, b in spans]


def take(names, ids):
    out = []
    for i in ids:
        if not 0 <= i < len(names):
            raise IndexError(i)
        out.append(names[i])
    return out


def offsets_of(names):
    off = [0]
    for x in names:
        off.append(off[-1] + len(x))
    return off


def render_named(seqs, names, quals, opt):
    """the image of seqs (str each) under opt (export_model.Options; FASTA or FASTQ) where the name of sequence s is names[s];
    quals: None, or the quality line of every record (FASTQ)"""
    assert opt.format in (FASTA, FASTQ) and len(names) == len(seqs)
    term = b"\r\n" if opt.crlf else b"\n"
    out = bytearray()
    for s, seq in enumerate(seqs):
        rec = export_model.render_record(seq, opt, s)
        head = 1 + len(export_model.name(opt, s))                      # the marker and the numbered name it replaces
        body = rec[head:]
        if quals is not None:
            assert opt.format == FASTQ and len(quals[s]) == len(seq)
            body = body[:len(body) - len(seq) - len(term)] + bytes(quals[s]) + term
        out += rec[:1] + bytes(names[s]) + body
    return bytes(out)
