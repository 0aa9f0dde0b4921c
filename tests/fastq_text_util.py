"""Helpers of the device-tokeniser tests (test_fastq_text_cpu.py, test_gpu_fastq_text.py): FASTQ text with ragged reads and names
of different lengths in R1 and R2, the project's host parser (cm_fastq_next) as the checker, record boundaries by counting lines."""
import ctypes as C
import os

import numpy as np

from circminer_amd import lib as cl

BASES = np.frombuffer(b"ACGTNacgt", np.uint8)


def records(rng, n, lo=30, hi=150, zero_at=(), name_pad=0, mate=1):
    """n FASTQ records as a list of [header, seq, plus, qual] (bytes, no newlines); reads of lo..hi bases, a zero-length read at
    the indices of zero_at; R2 names are longer than R1 names by a varying amount, so equal byte cuts hold different record counts"""
    out = []
    for i in range(n):
        ln = 0 if i in zero_at else int(rng.integers(lo, hi + 1))
        seq = bytes(BASES[rng.integers(0, len(BASES), ln)])
        qual = bytes(rng.integers(33, 74, ln).astype(np.uint8))               # '!' .. 'I': '@' (64) and '+' occur, also in front
        extra = b"x" * (name_pad + (i % 7 if mate == 2 else 0))
        name = b"@r%d%s/%d" % (i, extra, mate)
        if i % 3 == 0:
            name += b" 1:N:0:ACGT" if mate == 1 else b"  2:N:0  extra"        # comments: more tokens, runs of spaces
        out.append([name, seq, b"+" if i % 5 else b"+" + name[1:], qual])
    return out


def text_of(recs, last_newline=True):
    t = b"".join(b"\n".join(r) + b"\n" for r in recs)
    return t if last_newline or not t else t[:-1]


def line_starts(text: bytes):
    """offsets of the starts of the lines of `text` (lines end at a line feed; bytes behind the last one are a line) and their number"""
    a = np.frombuffer(text, np.uint8)
    nl = np.flatnonzero(a == 10)
    starts = np.concatenate([[0], nl + 1]).astype(np.int64)
    n_lines = len(nl) + (1 if len(a) and a[-1] != 10 else 0)
    return starts, n_lines


def whole_records(text: bytes, eof: bool):
    """(record starts incl. the end of the last whole record, whole records, lines): what a block holds, as the host parser counts"""
    a = np.frombuffer(text, np.uint8)
    starts, n_lines = line_starts(text)
    if not eof:
        n_lines = int((a == 10).sum())
    n_rec = n_lines // 4
    ends = np.concatenate([starts, [len(a)]])                                 # a last line without a line feed ends at the end
    rec = np.minimum(ends[np.arange(n_rec + 1) * 4], len(a)) if n_rec else np.zeros(1, np.int64)
    return rec.astype(np.uint64), n_rec, n_lines


class HostParse:
    """cm_fastq_next on files holding the given bytes: rc, n and copies of seq / off of the first batch"""

    def __init__(self, tmpdir, r1: bytes, r2: bytes, max_pairs: int, tag="h"):
        L = cl.load()
        p1, p2 = os.path.join(str(tmpdir), f"{tag}_1.fq"), os.path.join(str(tmpdir), f"{tag}_2.fq")
        with open(p1, "wb") as f:
            f.write(r1)
        with open(p2, "wb") as f:
            f.write(r2)
        self.paths = (p1, p2)
        h = C.c_void_p()
        assert L.cm_fastq_open(p1.encode(), p2.encode(), None, 0, 4, C.byref(h)) == 0
        fb = cl.FastqBatch()
        self.rc = L.cm_fastq_next(h, max_pairs, C.byref(fb))
        self.n = 0
        self.prior = False
        if self.rc == 0:
            n = self.n = int(fb.reads.n_pairs)
            self.prior = bool(fb.prior)
            self.off1 = np.ctypeslib.as_array(fb.reads.off1, (n + 1,)).copy() if n else np.zeros(1, np.uint64)
            self.off2 = np.ctypeslib.as_array(fb.reads.off2, (n + 1,)).copy() if n else np.zeros(1, np.uint64)
            self.seq1 = np.ctypeslib.as_array(fb.reads.seq1, (int(self.off1[n]),)).copy() if int(self.off1[n]) else np.zeros(0, np.uint8)
            self.seq2 = np.ctypeslib.as_array(fb.reads.seq2, (int(self.off2[n]),)).copy() if int(self.off2[n]) else np.zeros(0, np.uint8)
        L.cm_fastq_close(h)

    def max_len(self):
        return int(max(np.diff(self.off1).max(initial=0), np.diff(self.off2).max(initial=0)))


def check_against_host(e, h, n, t1, t2, eof=True):
    """arrays of the emulated (or device) stage `e` == the first n pairs of the host parse `h`; rec / used == the record boundaries"""
    assert e.rc == 0 and e.n == n and h.rc == 0 and h.n >= n
    for eo, es, ho, hs in ((e.off1, e.seq1, h.off1, h.seq1), (e.off2, e.seq2, h.off2, h.seq2)):
        assert np.array_equal(eo[:n + 1], ho[:n + 1])
        assert np.array_equal(es[:int(ho[n])], hs[:int(ho[n])])
    for er, used, t in ((e.rec1, e.tb.used1, t1), (e.rec2, e.tb.used2, t2)):
        rec, n_rec, _ = whole_records(t, eof)
        assert n_rec >= n and np.array_equal(er[:n + 1], rec[:n + 1]) and used == rec[n]
    assert e.tb.max_len == max(int(np.diff(h.off1[:n + 1]).max(initial=0)), int(np.diff(h.off2[:n + 1]).max(initial=0)))


def malformed(recs, i, how):
    """a copy of the records with record i broken in the way `how` names"""
    r = [list(x) for x in recs]
    if how == "header_empty":
        r[i][0] = b""
    elif how == "header_no_at":
        r[i][0] = b"r" + r[i][0][1:]
    elif how == "plus_empty":
        r[i][2] = b""
    elif how == "plus_no_plus":
        r[i][2] = b"-"
    elif how == "qual_short":
        r[i][3] = r[i][3][:-1]
    elif how == "qual_long":
        r[i][3] = r[i][3] + b"I"
    else:
        raise ValueError(how)
    return r


def fast_text(rng, n, name_width, lo=30, hi=150, tag=b"f"):
    """FASTQ text of n records built without a Python loop (for files of tens of MB): fixed-width names of name_width bytes,
    reads of lo..hi bases, "+" lines; returns bytes"""
    ln = rng.integers(lo, hi + 1, n).astype(np.int64)
    H = name_width + 1                                                         # '@' + name
    size = H + 1 + ln + 1 + 2 + ln + 1
    start = np.concatenate([[0], np.cumsum(size)])[:-1]
    out = np.empty(int(size.sum()), np.uint8)
    hdr = np.full((n, H + 1), ord("x"), np.uint8)
    hdr[:, 0], hdr[:, 1], hdr[:, H] = ord("@"), tag[0], 10
    v = np.arange(n)
    for d in range(8):                                                         # the record number, 8 digits
        hdr[:, H - 1 - d] = ord("0") + (v // 10 ** d) % 10
    out[(start[:, None] + np.arange(H + 1)[None, :]).ravel()] = hdr.ravel()
    tot = int(ln.sum())
    within = np.arange(tot) - np.repeat(np.concatenate([[0], np.cumsum(ln)])[:-1], ln)
    out[np.repeat(start + H + 1, ln) + within] = BASES[rng.integers(0, 4, tot)]
    out[start + H + 1 + ln] = 10
    out[start + H + 2 + ln] = ord("+")
    out[start + H + 3 + ln] = 10
    out[np.repeat(start + H + 4 + ln, ln) + within] = rng.integers(33, 74, tot).astype(np.uint8)
    out[start + size - 1] = 10
    return out.tobytes()


MALFORMED = ("header_empty", "header_no_at", "plus_empty", "plus_no_plus", "qual_short", "qual_long")
CARRIED_HEADER = b"@c1 1100000123 0 chr1 124 273 150 1 150 + 0 chr1 300 449 150 1 150 - 0 326 0 1 0"     # 23 tokens
assert len(CARRIED_HEADER[1:].split()) == 23
