"""The contract of dnagpu_dna_adapters (include/dnagpu.h) as plain Python loops: what tests/test_adapters.py and
tests/test_glue_adapters.py compare the device against.  It runs no code of the project and shares nothing with the C++.

first_hit(bases, adapters, ...) -> (p, m, a) of one segment's cut or None; trim() is the call over segment lists of a
stream's text with its report; trim_after_quals() is the composition with quals_model.trim that the glue's trim_reads runs."""
import dataclasses

import quals_model

BAD_ARG, QKMER_INVALID, TOO_LARGE = 5, 4, 6
DISCARD_UNTRIMMED, DISCARD_TRIMMED = 1, 2
NO_ADAPTER = 2 ** 64 - 1

# the qkmer alphabet: the bases every letter stands for ('U' stands for none)
IUPAC = {"A": "A", "T": "T", "C": "C", "G": "G", "U": "", "W": "AT", "S": "CG", "M": "AC", "K": "GT", "R": "AG", "Y": "CT",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


def first_hit(bases, adapters, err=(0, 1), min_overlap=1):
    """the cut of the segment with these bases (str): the hit with the least (p, m, a), or None"""
    n = len(bases)
    for p in range(n):
        hits = []
        for a, ad in enumerate(adapters):
            L = len(ad)
            o = min(L, n - p)
            m = 0
            for j in range(o):
                if bases[p + j] not in IUPAC[ad[j]]:
                    m += 1
            if o >= min(min_overlap, L) and m * err[1] <= err[0] * o:
                hits.append((p, m, a))
        if hits:
            return min(hits)
    return None


@dataclasses.dataclass
class Trimmed:
    out_len: list = dataclasses.field(default_factory=list)        # per input segment
    out_adapter: list = dataclasses.field(default_factory=list)
    out_mismatch: list = dataclasses.field(default_factory=list)
    pass_seq: list = dataclasses.field(default_factory=list)       # the passing segments, in input order
    pass_first: list = dataclasses.field(default_factory=list)
    pass_len: list = dataclasses.field(default_factory=list)
    report: dict = None


def empty_report():
    return dict(segments=0, passed=0, trimmed=0, bases_in=0, bases_kept=0, bases_cut=0, failed_short=0, failed_discarded=0,
                per_adapter=[0] * 32)


def trim(stream, seg_first, seg_len, adapters, err=(0, 1), min_overlap=1, min_bases=0, flags=0, seg_seq=None, cap=None, memo=None):
    """dnagpu_dna_adapters over the segments (seg_first[i], seg_len[i]) of the stream's text; memo: a dict shared between
    calls with the same adapters and options, bases -> cut"""
    t = Trimmed(report=empty_report())
    rep = t.report
    for i, (a, n) in enumerate(zip(seg_first, seg_len)):
        a, n = int(a), int(n)
        bases = stream[a:a + n]
        assert len(bases) == n
        if memo is not None and bases in memo:
            hit = memo[bases]
        else:
            hit = first_hit(bases, adapters, err, min_overlap)
            if memo is not None:
                memo[bases] = hit
        kept = n if hit is None else hit[0]
        t.out_len.append(kept)
        t.out_adapter.append(NO_ADAPTER if hit is None else hit[2])
        t.out_mismatch.append(0 if hit is None else hit[1])
        rep["segments"] += 1
        rep["bases_in"] += n
        rep["bases_kept"] += kept
        rep["bases_cut"] += n - kept
        if hit is not None:
            rep["trimmed"] += 1
            rep["per_adapter"][hit[2]] += 1
        if kept == 0 or kept < min_bases:
            rep["failed_short"] += 1
        elif (hit is None and flags & DISCARD_UNTRIMMED) or (hit is not None and flags & DISCARD_TRIMMED):
            rep["failed_discarded"] += 1
        else:
            rep["passed"] += 1
            if cap is None or len(t.pass_seq) < cap:
                t.pass_seq.append(i if seg_seq is None else int(seg_seq[i]))
                t.pass_first.append(a)
                t.pass_len.append(kept)
    return t


def trim_after_quals(stream, col, starts, adapters, err=(0, 1), min_overlap=1, flags=0, **quals_opt):
    """quals_model.trim over the table, then trim() over its passing list with min_bases applied again to the final length ->
    (quals_model.Trimmed, Trimmed): the second one's pass lists are what the gathers and the names take are given"""
    q = quals_model.trim(col, starts, **quals_opt)
    t = trim(stream, q.seg_first, q.seg_len, adapters, err, min_overlap, quals_opt.get("min_bases", 0), flags, seg_seq=q.seg_seq)
    return q, t
