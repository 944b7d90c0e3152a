"""The contract of dnagpu_table_to_text (include/dnagpu.h) as a plain Python loop over records and lines: what the tests of
tests/test_table_to_text.py compare the device against.  It runs no code of the project.

render(records, opt) -> bytes: the whole image; record_pos(records, opt) -> the offset of every record's first byte and, last,
the image's size; window_of_one(length, opt, first, count, bases) -> the bytes of a window of the image of ONE sequence,
byte by byte from the offset alone, with bases(i, n) giving bases [i, i + n) of the sequence as a str."""
import dataclasses

LINES, FASTA, FASTQ = 1, 2, 3


@dataclasses.dataclass
class Options:
    format: int = LINES
    crlf: bool = False
    line_width: int = 0
    prefix: bytes = b""
    name_base: int = 0
    numbers: list = None
    quality: bytes = b"I"


def name(opt, s):
    number = opt.numbers[s] if opt.numbers is not None else (opt.name_base + s) % (1 << 64)
    return opt.prefix + str(int(number)).encode()


def render_record(seq, opt, s):
    t = b"\r\n" if opt.crlf else b"\n"
    bases = seq.encode()
    if opt.format == LINES:
        return bases + t
    if opt.format == FASTA:
        out = b">" + name(opt, s) + t
        width = opt.line_width if 0 < opt.line_width < len(bases) else len(bases)
        at = 0
        while at < len(bases):                   # (a sequence of 0 bases: a header with no sequence line)
            out += bases[at:at + width] + t
            at += width
        return out
    return b"@" + name(opt, s) + t + bases + t + b"+" + t + opt.quality * len(bases) + t


def render(records, opt):
    return b"".join(render_record(seq, opt, s) for s, seq in enumerate(records))


def record_pos(records, opt):
    pos = [0]
    for s, seq in enumerate(records):
        pos.append(pos[-1] + len(render_record(seq, opt, s)))
    return pos


def empties(records):
    return sum(1 for seq in records if not seq)


def window_of_one(length, opt, first, count, bases):
    """bytes [first, first + count) of the image of one sequence of `length` >= 1 bases (record 0)"""
    t = b"\r\n" if opt.crlf else b"\n"
    head = b"" if opt.format == LINES else (b">" if opt.format == FASTA else b"@") + name(opt, 0) + t
    width = opt.line_width if opt.format == FASTA and 0 < opt.line_width < length else length
    pitch = width + len(t)
    n_lines = -(-length // width)
    body = length + n_lines * len(t)
    out = bytearray()
    for p in range(first, first + count):
        if p < len(head):
            out += head[p:p + 1]
            continue
        q = p - len(head)
        if q < body:
            line, col = divmod(q, pitch)
            line_len = min(width, length - line * width)
            out += bases(line * width + col, 1).encode() if col < line_len else t[col - line_len:col - line_len + 1]
            continue
        q -= body
        assert opt.format == FASTQ, "the window leaves the image"
        tail_head = b"+" + t
        if q < len(tail_head):
            out += tail_head[q:q + 1]
        elif q < len(tail_head) + length:
            out += opt.quality
        else:
            q -= len(tail_head) + length
            assert q < len(t), "the window leaves the image"
            out += t[q:q + 1]
    return bytes(out)


def size_of_one(length, opt):
    t = 2 if opt.crlf else 1
    if opt.format == LINES:
        return length + t
    head = 1 + len(name(opt, 0)) + t
    if opt.format == FASTA:
        width = opt.line_width if 0 < opt.line_width < length else length
        return head + length + -(-length // width) * t
    return head + 2 * length + 3 * t + 1
