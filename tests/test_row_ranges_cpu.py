"""format_ranges (circminer_amd/csrc/cm_row_ranges.h), the one loop cm_mapping_run gets a batch's text out of the device formatters
with, without a device: tests/diag/row_ranges_san_main.cpp drives it over a formatter that only counts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_ranges_over_a_counting_formatter(tmp_path):
    """for one file and for two, under the address and undefined-behaviour sanitizers: a range of 2^32 bytes is halved down to one
    record, where the refusal is final; every record is formatted once and in order across halvings and growths; a growth asks for
    the expression cm_mapping_run's three loops held (written out in the program); another refusal passes through once; an empty
    set is one call; a refusal that says nothing is the tie group's only for the first range"""
    exe = str(tmp_path / "row_ranges")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "circminer_amd", "csrc"), os.path.join(ROOT, "tests", "diag", "row_ranges_san_main.cpp"), "-o", exe])
    assert subprocess.check_output([exe], text=True).strip() == "0 mismatches"
