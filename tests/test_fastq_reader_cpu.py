"""The host FASTQ reader and the threaded PAM writer (circminer_amd/csrc/host_fastq.cpp) without Python in between:
tests/diag/fastq_reader_san_main.cpp is linked straight against that file and compares every way through the reader with a
single-threaded re-parse of the bytes it wrote."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fastq_reader_against_a_reparse(tmp_path):
    """built plain here (the program's header gives the lines for the address / undefined-behaviour and the thread sanitizer): the
    plain path with 1 and 6 threads, the record path, ranks 0 - 2 of 3 on plain and gzip input, text blocks with the "nothing
    consumed" path, the malformed tails, the release hook over growing reads, cm_write_pam over 70 000 rows on 5 threads"""
    exe = str(tmp_path / "fastq_reader")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "circminer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "diag", "fastq_reader_san_main.cpp"), os.path.join(ROOT, "circminer_amd", "csrc", "host_fastq.cpp"),
                           "-lz", "-lpthread", "-o", exe])
    assert subprocess.check_output([exe], text=True).strip() == "0 mismatches"
