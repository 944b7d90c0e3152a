"""The contract of dnagpu_reads_from_text (include/dnagpu.h) as a plain Python loop over the lines of a text: what the tests of
tests/test_reads_from_text.py compare the device against.  It runs no code of the project.

parse(data, opt, more) -> Parsed: on success the source records' offsets, the sequences of the result with the record and the
offset in that record's sequence text each came from, the bytes consumed and the counters; on an input error the error (code,
offset, 0-based record, character) with the lowest offset -- at equal offsets a bad '@' or '+' before empty, before invalid
character, before truncated."""
import dataclasses
import re

from text_model import BAD_ARG, DNA_EMPTY, DNA_INVALID_CHAR, FASTA, LINES, cut, lines_of

FASTQ = 3
ERROR, DROP, SPLIT = 0, 1, 2
BASES = b"ATCG"
AMBIGUITY = b"NRYKMSWBDHV"
MSG_AT = "FASTQ record does not begin with '@'"
MSG_PLUS = "FASTQ separator line does not begin with '+'"
MSG_TRUNCATED = "truncated FASTQ record"
MSG_ORPHAN = "sequence data before the first header"
MSG_EMPTY = "DNA sequence cannot be empty"
_OPEN, _EMPTY, _CHAR, _TRUNC = 0, 1, 2, 3                          # the order of errors at equal offsets


@dataclasses.dataclass
class Options:
    format: int = LINES
    ambiguous: int = ERROR
    fold_case: bool = False
    min_bases: int = 0


@dataclasses.dataclass
class Parsed:
    records: int = 0                                              # source records accounted for
    pos: list = dataclasses.field(default_factory=list)           # byte offset of every source record's first byte
    sequences: list = dataclasses.field(default_factory=list)     # str per sequence of the result
    src_record: list = dataclasses.field(default_factory=list)
    src_offset: list = dataclasses.field(default_factory=list)
    consumed: int = 0
    ambiguous: int = 0
    dropped: int = 0
    short_out: int = 0
    error: tuple = None                                           # (code, offset, record or None, char bytes)
    message: str = None


def fastq_cut(data):
    """one past the newline that ends the last complete four-line record (0: there is none)"""
    at, count = 0, data.count(b"\n") // 4 * 4
    for _ in range(count):
        at = data.index(b"\n", at) + 1
    return at


def parse(data, opt=Options(), more=False):
    data = bytes(data)
    p = Parsed()
    fmt = opt.format
    if more:
        p.consumed = fastq_cut(data) if fmt == FASTQ else cut(data, fmt)
    else:
        p.consumed = len(data)
    errors = []                                                   # (offset, order, code, record, char, message)
    texts = []                                                    # per record: its sequence text S, folded
    lines = lines_of(data[:p.consumed])

    def sequence_line(a, content, record):
        for i, ch in enumerate(content):
            c = bytes([ch])
            up = c.upper() if opt.fold_case else c
            if record is None:
                errors.append((a + i, _OPEN, BAD_ARG, None, b"", MSG_ORPHAN))
            elif up in BASES or (up in AMBIGUITY and opt.ambiguous != ERROR):
                texts[record].append(up.decode())
            else:
                errors.append((a + i, _CHAR, DNA_INVALID_CHAR, record, c, "Invalid character in DNA sequence: " + c.decode("latin-1")))

    for i, (a, content) in enumerate(lines):
        first = data[a:a + 1]
        if fmt == LINES:
            if not content:
                errors.append((a, _EMPTY, DNA_EMPTY, len(texts), b"", MSG_EMPTY))
            texts.append([])
            p.pos.append(a)
            sequence_line(a, content, len(texts) - 1)
        elif fmt == FASTA:
            if first == b">":
                texts.append([])
                p.pos.append(a)
            else:
                sequence_line(a, content, len(texts) - 1 if texts else None)
        else:
            record, role = divmod(i, 4)
            if role == 0:
                texts.append([])
                p.pos.append(a)
                if first != b"@":
                    errors.append((a, _OPEN, BAD_ARG, record, b"", MSG_AT))
            elif role == 1:
                if not content:
                    errors.append((a, _EMPTY, DNA_EMPTY, record, b"", MSG_EMPTY))
                sequence_line(a, content, record)
            elif role == 2 and first != b"+":
                errors.append((a, _OPEN, BAD_ARG, record, b"", MSG_PLUS))
    if fmt == FASTQ and len(lines) % 4:
        whole = len(lines) // 4
        errors.append((lines[4 * whole][0], _TRUNC, BAD_ARG, whole, b"", MSG_TRUNCATED))
    if fmt == FASTA:
        errors += [(at, _EMPTY, DNA_EMPTY, r, b"", MSG_EMPTY) for r, (at, t) in enumerate(zip(p.pos, texts)) if not t]
    if errors:
        at, _, code, rec, ch, msg = min(errors, key=lambda e: e[:2])
        return Parsed(error=(code, at, rec, ch), message=msg)

    p.records = len(texts)
    for r, t in enumerate(texts):
        s = "".join(t)
        n_amb = sum(1 for ch in s if ch not in "ATCG")
        p.ambiguous += n_amb
        if opt.ambiguous == DROP and n_amb:
            p.dropped += 1
            continue
        pieces = [(m.start(), m.group()) for m in re.finditer("[ATCG]+", s)] if opt.ambiguous == SPLIT else [(0, s)]
        for off, piece in pieces:
            if len(piece) < opt.min_bases:
                p.short_out += 1
                continue
            p.sequences.append(piece)
            p.src_record.append(r)
            p.src_offset.append(off)
    return p
