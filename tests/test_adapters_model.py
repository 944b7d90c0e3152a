"""The model of dnagpu_dna_adapters (tests/adapters_model.py) pinned on vectors whose cuts are written out by hand, and the
host check of adapters_math.hpp (tests/host/adapters_math_check.cpp) built and run.  No GPU."""
import os
import shutil
import subprocess

import pytest

import adapters_model as am

AD = "AGATCGGAAGAGC"                     # 13 letters


def test_exact_full_adapter():
    #        0123456789
    read = "TTGCATGCAT" + AD + "CCC"
    assert am.first_hit(read, [AD]) == (10, 0, 0)
    assert am.first_hit(read, [AD], err=(1, 10), min_overlap=3) == (10, 0, 0)
    assert am.first_hit("TTGCATGCAT", [AD], min_overlap=3) is None


def test_one_mismatch_at_overlap_10_and_9():
    ten = AD[:10]                         # AGATCGGAAG
    bad = "AGATCTGAAG"                    # letter 5: G -> T
    assert sum(x != y for x, y in zip(ten, bad)) == 1
    # overlap 10 at the read's end: 1 * 10 <= 1 * 10
    assert am.first_hit("CCCCC" + bad, [AD], err=(1, 10), min_overlap=9) == (5, 1, 0)
    # overlap 9: 1 * 10 > 1 * 9; the overlaps behind it (8 .. 1 letters of "GATCTGAA..") match nothing of the adapter's head
    # until the 1-letter overlap, which min_overlap 9 excludes
    assert am.first_hit("CCCCC" + bad[:9], [AD], err=(1, 10), min_overlap=9) is None
    # the same 9 letters without the mismatch are a hit
    assert am.first_hit("CCCCC" + ten[:9], [AD], err=(1, 10), min_overlap=9) == (5, 0, 0)


def test_partial_overlap_of_min_overlap_and_one_less():
    assert am.first_hit("CCCCCCC" + AD[:5], [AD], min_overlap=5) == (7, 0, 0)
    assert am.first_hit("CCCCCCC" + AD[:4], [AD], min_overlap=5) is None
    # an adapter shorter than min_overlap: its whole length is enough
    assert am.first_hit("CCCCAGAC", ["AGA"], min_overlap=5) == (4, 0, 0)
    assert am.first_hit("CCCCCCAG", ["AGA"], min_overlap=5) is None


def test_earlier_hit_with_a_mismatch_beats_a_later_perfect_one():
    ad = "ACGTACGTAC"                     # 10 letters, rate 1/10
    one = "ACGTTCGTAC"                    # letter 4: A -> T
    read = "GG" + one + "GG" + ad + "GG"
    assert am.first_hit(read, [ad], err=(1, 10), min_overlap=10) == (2, 1, 0)
    assert am.first_hit(read, [ad], err=(0, 1), min_overlap=10) == (14, 0, 0)


def test_two_adapters_at_one_position():
    read = "TT" + "ACGTACGTAC" + "TT"
    # fewer mismatches first: adapter 1 is exact, adapter 0 has one mismatch
    assert am.first_hit(read, ["ACGTTCGTAC", "ACGTACGTAC"], err=(1, 10), min_overlap=10) == (2, 0, 1)
    # equal mismatches: the lower index
    assert am.first_hit(read, ["ACGTACGTAC", "ACGTACGTAC"], err=(1, 10), min_overlap=10) == (2, 0, 0)
    assert am.first_hit(read, ["ACGTTCGTAC", "ACGTACGTTC"], err=(1, 10), min_overlap=10) == (2, 1, 0)


def test_iupac_letters():
    assert am.first_hit("TTTTACGT", ["NNNN"], min_overlap=4) == (0, 0, 0)          # N matches every base
    assert am.first_hit("TTTTACGT", ["RCGT"], min_overlap=4) == (4, 0, 0)          # R = A or G
    assert am.first_hit("TTTTGCGT", ["RCGT"], min_overlap=4) == (4, 0, 0)
    assert am.first_hit("TTTTCCGT", ["RCGT"], min_overlap=4) is None
    assert am.first_hit("TTTTCCGT", ["RCGT"], err=(1, 4), min_overlap=4) == (4, 1, 0)
    # U matches no base: always a mismatch, so "UCGT" needs the rate to pay for it
    assert am.first_hit("TTTTACGT", ["UCGT"], min_overlap=4) is None
    assert am.first_hit("TTTTTCGT", ["UCGT"], min_overlap=4) is None
    assert am.first_hit("TTTTACGT", ["UCGT"], err=(1, 4), min_overlap=4) == (4, 1, 0)


def test_trim_lists_and_report():
    stream = "CCCCAGAT" + "AGATCCCC" + "CCCCCCCC" + "AG"
    first, length = [0, 8, 16, 24], [8, 8, 8, 2]
    t = am.trim(stream, first, length, ["AGAT"], min_overlap=3, min_bases=3, seg_seq=[7, 5, 3, 1])
    assert t.out_len == [4, 0, 8, 2]
    assert t.out_adapter == [0, 0, am.NO_ADAPTER, am.NO_ADAPTER]
    assert t.out_mismatch == [0, 0, 0, 0]
    assert (t.pass_seq, t.pass_first, t.pass_len) == ([7, 3], [0, 16], [4, 8])
    r = t.report
    assert (r["segments"], r["passed"], r["trimmed"], r["failed_short"], r["failed_discarded"]) == (4, 2, 2, 2, 0)
    assert (r["bases_in"], r["bases_kept"], r["bases_cut"]) == (26, 14, 12)
    assert r["per_adapter"][:2] == [2, 0]
    t = am.trim(stream, first, length, ["AGAT"], min_overlap=3, flags=am.DISCARD_UNTRIMMED)
    assert t.pass_seq == [0] and t.report["failed_short"] == 1 and t.report["failed_discarded"] == 2
    t = am.trim(stream, first, length, ["AGAT"], min_overlap=3, flags=am.DISCARD_TRIMMED, cap=1)
    assert t.pass_seq == [2] and t.report["passed"] == 2 and t.report["failed_discarded"] == 1


SANITIZERS = ["-g", "-Xarch_host", "-fsanitize=address,undefined"]


@pytest.mark.parametrize("extra", [[], SANITIZERS], ids=["plain", "sanitizers"])
def test_adapters_math_header(tmp_path, extra):
    """adapters_math.hpp's window mismatch count, thr table and lane walk against per-base loops.  Host code of the header the
    kernels use, built with hipcc as a stand-alone program (the second build with AddressSanitizer and
    UndefinedBehaviorSanitizer on it): no device is touched."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapters_math_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", *extra, "-I",
                           os.path.join(root, "dna-sequences-pg-extension_amd", "csrc"),
                           os.path.join(root, "tests", "host", "adapters_math_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
