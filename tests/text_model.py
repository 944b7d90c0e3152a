"""The contract of dnagpu_table_from_text (include/dnagpu.h) as a plain Python loop over the lines of a text: what the tests of
tests/test_table_from_text.py compare the device against.  It runs no code of the project.

parse(data, fmt, more) -> Parsed: on success the records' texts, the byte offset of every record's first byte and the
bytes consumed; on an input error the error (code, offset, 0-based record, character) with the lowest offset."""
import dataclasses

LINES, FASTA = 1, 2
BAD_ARG, DNA_EMPTY, DNA_INVALID_CHAR = 5, 11, 12          # DNAGPU_ERR_*
MESSAGES = {DNA_EMPTY: "DNA sequence cannot be empty", BAD_ARG: "sequence data before the first header"}


def message(code, char):
    """dnagpu_last_error() after the error: the reference's text verbatim (dna.c:160-166)"""
    return "Invalid character in DNA sequence: " + char.decode("latin-1") if code == DNA_INVALID_CHAR else MESSAGES[code]


@dataclasses.dataclass
class Parsed:
    records: list = dataclasses.field(default_factory=list)       # str per record
    pos: list = dataclasses.field(default_factory=list)           # byte offset of every record's first byte
    consumed: int = 0
    error: tuple = None                                           # (code, offset, record or None, char bytes)


def cut(data, fmt):
    """where a chunk that more text follows is cut: LINES one past the last newline (0: none); FASTA the '>' of the last
    header (no header: everything counts, there is no record to hold back)"""
    if fmt == LINES:
        return data.rfind(b"\n") + 1
    at = len(data)
    for i in range(len(data)):
        if data[i:i + 1] == b">" and (i == 0 or data[i - 1:i] == b"\n"):
            at = i
    return at


def lines_of(data):
    """(offset, content) of every line: a line ends at a newline, a carriage return directly before it belongs to the
    terminator; a last line without a terminator is a line, text that ends in a newline has no extra empty one"""
    out, a = [], 0
    while a < len(data):
        e = data.find(b"\n", a)
        if e < 0:
            out.append((a, data[a:]))
            break
        c = e - 1 if e > a and data[e - 1:e] == b"\r" else e
        out.append((a, data[a:c]))
        a = e + 1
    return out


def parse(data, fmt=LINES, more=False):
    data = bytes(data)
    p = Parsed()
    p.consumed = cut(data, fmt) if more else len(data)
    errors = []                                                   # (offset, code, record, char)
    texts = []
    for a, content in lines_of(data[:p.consumed]):
        if fmt == LINES:
            if not content:
                errors.append((a, DNA_EMPTY, len(texts), b""))
            texts.append([])
            p.pos.append(a)
        elif content[:1] == b">" or data[a:a + 1] == b">":
            texts.append([])
            p.pos.append(a)
            continue                                              # the whole header line is ignored
        for i, ch in enumerate(content):
            c = bytes([ch])
            if not texts:
                errors.append((a + i, BAD_ARG, None, b""))
            elif c in (b"A", b"T", b"C", b"G"):
                texts[-1].append(c.decode())
            else:
                errors.append((a + i, DNA_INVALID_CHAR, len(texts) - 1, c))
    p.records = ["".join(t) for t in texts]
    if fmt == FASTA:
        errors += [(at, DNA_EMPTY, r, b"") for r, (at, t) in enumerate(zip(p.pos, p.records)) if not t]
    if errors:
        at, code, rec, ch = min(errors, key=lambda e: e[0])
        p.error = (code, at, rec, ch)
        p.records, p.pos, p.consumed = [], [], 0
    return p
