"""What cm_mapping_run must leave behind, from the CPU oracle's final states through the Python restatements of the writers
(tests/test_fastq_io.py): the rows of the mapping file and the lines of a remain file."""
from test_fastq_io import py_pam_row, py_remain_header, py_sam_rows


def expected_mapping_rows(report, names, want, chrs, s1=None, q1=None, s2=None, q2=None):
    """the rows of <out>.mapping.pam (report 1) or, behind its header, of <out>.mapping.sam (report 2): one row, or two, per pair"""
    if report == 1:
        return [py_pam_row(names[i], want[i], chrs) for i in range(len(names))]
    exp = []
    for i in range(len(names)):
        exp += py_sam_rows(names[i], want[i], chrs, s1[i], q1[i], s2[i], q2[i])
    return exp


def expected_remain_lines(names, want, keep, chrs, seqs, quals):
    """the lines of <out>_<R>_remain_R?.fastq: four per pair still active after the last round (`keep`), carried header first"""
    lines = []
    for i in keep:
        lines += [py_remain_header(names[i], want[i], chrs), seqs[i], "+", quals[i]]
    return lines
