"""glue/row_batch.h, the batch every streaming object of the glue collects its rows in, checked on the host."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SANITIZERS = ["-g", "-fsanitize=address,undefined"]


@pytest.mark.parametrize("extra", [[], SANITIZERS], ids=["plain", "sanitizers"])
def test_row_batch_on_the_host(tmp_path, extra):
    """row_batch.h as a stand-alone program (the second build with AddressSanitizer and UndefinedBehaviorSanitizer on it)
    against a packer that moves one base at a time: rows of 0 .. 1000 bases at every offset in a word, every row cut back out
    of the stream, a batch of all-T rows cleared and refilled with all-A rows, the growth past the first allocation, and the
    two tests of the add policy around the limit"""
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    exe = str(tmp_path / "row_batch_check")
    subprocess.check_call([gcc, "-O1", "-std=c11", "-Wall", "-Wextra", "-Werror", *extra, "-I",
                           os.path.join(ROOT, "dna-sequences-pg-extension_amd", "glue"),
                           os.path.join(ROOT, "tests", "host", "row_batch_check.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
