"""Helpers of the device-side PAM formatter's tests (test_pam_text_cpu.py, test_gpu_pam_text.py): states at every boundary of the
row's number formats, FASTQ records whose names cover the rules of the host parser, and the project's own host writer as the
checker -- cm_fastq_next on files holding the same bytes, then cm_write_pam with the same states."""
import ctypes as C
import os

import numpy as np

from circminer_amd import lib as cl
from fastq_text_util import records, text_of

INT_MIN, INT_MAX, INF_I = -2 ** 31, 2 ** 31 - 1, 1_000_000_000
U32_VALUES = (0, 9, 10, 99, 100, 999_999_999, 1_000_000_000, 4_294_967_295)
MLEN_VALUES = U32_VALUES + (2 ** 31,)                                  # printed through (int): negative
INT_VALUES = (0, -1, -9, -10, INT_MIN, INT_MAX, INF_I)
# every type 0 .. 13, -1 and 14, and the int boundaries in the type field: 23 values, a prime, so that over 23 * 9 rows every value of
# every other field (cycles of 2, 3, 4, 7, 8 and 9) meets every type -- the mapped ones, which print the field, among them
TYPE_VALUES = tuple(range(14)) + (-1, 14, -9, -10, INT_MIN, INT_MAX, INF_I, 100, 13)
MAPPED_TYPES = (0, 1, 2, 3, 4, 5, 7)
U32_FIELDS = ("spos_r1", "spos_r2", "epos_r1", "epos_r2", "qspos_r1", "qspos_r2", "qepos_r1", "qepos_r2")
# chromosome names of 1 and 40 bytes among ordinary ones: rows (name, contig id, start, length) as the writer takes them
CHRS = [("c", 1, 0, 1000), ("chr_of_forty_bytes_" + "x" * 21, 1, 1000, 500), ("chr2", 2, 0, 70000), ("7", 2, 70000, 10)]
assert len(CHRS[1][0]) == 40 and len(TYPE_VALUES) == 23


def directed_states(n, n_chr=len(CHRS)):
    """n states that cycle through the boundaries of every printed field (see the lists above); state i depends on i only"""
    st = np.zeros(n, cl.MAPPED_DTYPE)
    i = np.arange(n)
    st["type"] = np.array(TYPE_VALUES, np.int64)[i % 23].astype(np.int32)
    for j, f in enumerate(U32_FIELDS):
        st[f] = np.array(U32_VALUES, np.uint64)[(i + j) % 8].astype(np.uint32)
    for j, f in enumerate(("mlen_r1", "mlen_r2")):
        st[f] = np.array(MLEN_VALUES, np.uint64)[(i + 4 * j) % 9].astype(np.uint32)
    for j, f in enumerate(("ed_r1", "ed_r2", "tlen")):
        st[f] = np.array(INT_VALUES, np.int64)[(i + 2 * j) % 7].astype(np.int32)
    st["junc_num"] = np.where(i % 2, 65535, 0)
    st["gm_compatible"] = np.array([0, 1, 255], np.uint8)[i % 3]
    st["r1_forward"] = i & 1
    st["r2_forward"] = (i >> 1) & 1
    st["chr_id"] = np.array([-1, 0, n_chr - 1, n_chr], np.int32)[i % 4]
    st["contig_num"] = (i % 5) - 1
    st["pad"] = 0xEE                                                    # nobody prints the padding
    return st


# headers whose names the rules decide: no token at all, only spaces, a name that is all suffix, a suffix cut, one byte, a tab, a NUL
SPECIAL_HEADERS = (b"@", b"@   ", b"@/1", b"@a/1", b"@q", b"@ta\tb/1 c", b"@nu\x00l/1", b"@  lead  two", b"@x/", b"@a/b/2", b"@//", b"@\x00")


def name_records(rng, n, long_run=None, mate=1):
    """n FASTQ records (fastq_text_util.records: comments, runs of spaces, /1 suffixes) with the special headers spread over them
    and, for long_run = (start, stop), names of 300 - 400 bytes on those consecutive records"""
    recs = records(rng, n, mate=mate)
    if long_run:
        for i in range(*long_run):
            recs[i][0] = b"@" + bytes(rng.integers(ord("a"), ord("z") + 1, int(rng.integers(300, 401))).astype(np.uint8)) + b"/1 tail"
    for k, h in enumerate(SPECIAL_HEADERS):                             # (a few land inside the long run: it stays far above the window)
        if k < n:
            recs[(k * 11 + 3) % n][0] = h
    return recs


class HostRows:
    """the checker: cm_fastq_next on files with the bytes t1 / t2, then the host writer `write` ("write_pam": cm_write_pam;
    "write_sam": cm_write_sam without a header) / the parser's names and arrays"""

    def __init__(self, tmpdir, t1: bytes, t2: bytes, n, tag="pam", chrs=CHRS, write="write_pam"):
        self.dir, self.tag, self.chrs, self.write = str(tmpdir), tag, chrs, write
        p1, p2 = os.path.join(self.dir, f"{tag}_1.fq"), os.path.join(self.dir, f"{tag}_2.fq")
        open(p1, "wb").write(t1)
        open(p2, "wb").write(t2)
        self.paths = (p1, p2)
        self.rd = cl.FastqReader(p1, p2, chrs, 4)
        self.batch = self.rd.next_batch(n)
        assert self.batch is not None and self.batch.n == n
        self._k = 0

    def arrays(self):
        """(seq1, off1, seq2, off2, qual1, qual2) of the parsed batch, copies"""
        fb, n = self.batch.fb, self.batch.n
        off1 = np.ctypeslib.as_array(fb.reads.off1, (n + 1,)).copy()
        off2 = np.ctypeslib.as_array(fb.reads.off2, (n + 1,)).copy()

        def take(p, ln):
            return np.ctypeslib.as_array(p, (ln,)).copy() if ln else np.zeros(0, np.uint8)
        return (take(fb.reads.seq1, int(off1[n])), off1, take(fb.reads.seq2, int(off2[n])), off2, take(fb.qual1, int(off1[n])), take(fb.qual2, int(off2[n])))

    def names(self):
        """the names as the writer prints them: without their NULs"""
        fb, n = self.batch.fb, self.batch.n
        off = np.ctypeslib.as_array(fb.name_off1, (n + 1,))
        raw = C.string_at(fb.names1, int(off[n])) if int(off[n]) else b""
        return [raw[int(off[i]):int(off[i + 1])].split(b"\0")[0] for i in range(n)]

    def rows(self, states, first=0, count=None, chrs=None):
        n = self.batch.n
        count = n - first if count is None else count
        self._k += 1
        path = os.path.join(self.dir, f"{self.tag}_{self._k}.{self.write[-3:]}")
        w = cl.RecordWriter(path, None, self.chrs if chrs is None else chrs)
        if count:
            getattr(w, self.write)(self.batch, np.ascontiguousarray(states), np.arange(first, first + count, dtype=np.uint64))
        w.close()
        return open(path, "rb").read()

    def close(self):
        self.rd.close()


def pair_text(rng, n, long_run=None):
    """(text of R1, text of R2) for n pairs"""
    return text_of(name_records(rng, n, long_run, 1)), text_of(records(rng, n, mate=2))
