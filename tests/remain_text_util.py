"""Helpers of the device-side remain formatter's tests (test_remain_text_cpu.py, test_gpu_remain_text.py): the host emulation
(tests/hostemu_remain.cpp) built here, the directed states of pam_text_util with the boundaries of the sort key gspos added, FASTQ
records whose R2 names differ from the R1 names, the selections, a plain restatement of a record, the key `sort -k2,2n` sees, and
the project's own host writer as the checker -- cm_fastq_next on files holding the same bytes, then cm_write_remain_records with
(pair, state) records."""
import ctypes as C
import os
import subprocess

import numpy as np

from circminer_amd import lib as cl
from fastq_text_util import BASES, records, text_of
from pam_text_util import CHRS, INT_MAX, INT_MIN, MAPPED_TYPES, HostRows, directed_states, name_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN_RECS, WINDOW = 16, 8192                                            # cmrm::SPAN_RECS, cmrt::WINDOW
CONTIG_SIZE = 1_100_000_000                                             # CM_CONTIG_SIZE
CONTIG_VALUES = (-1, 0, 1, 15, INT_MIN, INT_MAX, 2)                     # a cycle of 7 against the types' 23: every type meets every one
CM_EINVAL, CM_EIO, CM_ESTATE, CM_ELIMIT = -1, -3, -5, -6
# R2 headers whose names the rules decide, as pam_text_util.SPECIAL_HEADERS does for R1 (other places, so that a pair rarely has two)
SPECIAL_HEADERS2 = (b"@", b"@  ", b"@/2", b"@b/2", b"@z", b"@tb\tc/2 d", b"@mu\x00m/2", b"@ two  lead", b"@y/", b"@a/b/1", b"@//", b"@\x00", b"@same/1")
STARS = " * * * * * * * * * * * * * * * * * * * *"


def emu_remain(built=None):
    """tests/hostemu_remain.cpp as a shared library, built when it is older than what it includes"""
    out_dir = os.path.join(ROOT, "tests", "_hostemu")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libcmemu_remain.so")
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", x) for x in ("hostemu_remain.cpp", "hostemu_pam.cpp", "hostemu_sam.cpp", "hostemu_rows.h")] + \
           [os.path.join(csrc, x) for x in ("cm_remain_text.h", "cm_pam_text.h", "cm_sam_text.h", "cm_rows_text.h", "cm_fastq_text.h")] + \
           [os.path.join(ROOT, "include", "circminer_hot.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-I", os.path.join(ROOT, "tests"),
                               srcs[0], "-o", so])
    E = C.CDLL(so)
    vp = C.c_void_p
    E.emu_names.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, vp, vp]
    E.emu_names.restype = C.c_int
    E.emu_quals.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp]
    E.emu_quals.restype = C.c_int
    E.emu_format_remain.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(cl.ChrInfo), C.c_uint32, C.c_uint64, C.c_uint64,
                                    vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64), vp, C.c_uint64, C.c_uint32, vp]
    E.emu_format_remain.restype = C.c_int
    return E


def remain_states(n, n_chr=len(CHRS)):
    """pam_text_util.directed_states with the boundaries of gspos = contig_num * CM_CONTIG_SIZE + (uint32)(spos_r1 + shift): contig_num
    cycles through CONTIG_VALUES, and chr_id changes every 8 states, so that every spos_r1 of the cycle of 8 (4294967295 among them:
    the sum wraps 2^32 under a shift) meets every chr_id of -1, 0, n_chr - 1, n_chr"""
    st = directed_states(n, n_chr)
    i = np.arange(n)
    st["contig_num"] = np.array(CONTIG_VALUES, np.int64)[i % 7].astype(np.int32)
    st["chr_id"] = np.array([-1, 0, n_chr - 1, n_chr], np.int32)[(i // 8) % 4]
    return st


def remain_pair_records(rng, n, long_run=None, hi=150):
    """(records of R1, records of R2): pam_text_util.name_records for R1; for R2 records with names of their own (longer, other
    suffixes), the special R2 headers, and the long run's names on R2 as well; reads of 0, 1, 150 and hi bases in both files"""
    r1, r2 = name_records(rng, n, long_run, 1), records(rng, n, mate=2)
    if long_run:
        for i in range(*long_run):
            r2[i][0] = b"@" + bytes(rng.integers(ord("A"), ord("Z") + 1, int(rng.integers(300, 401))).astype(np.uint8)) + b"/2"
    for k, h in enumerate(SPECIAL_HEADERS2):
        if k < n:
            r2[(k * 7 + 5) % n][0] = h
    for k, ln in enumerate((0, 1, 150, hi, 0, 150)):
        for mate, recs in enumerate((r1, r2)):
            i = (k * 13 + 2 + 6 * mate) % n                                 # (a batch of one pair keeps the last of them)
            recs[i][1] = bytes(BASES[rng.integers(0, len(BASES), ln)])
            recs[i][3] = bytes(rng.integers(33, 74, ln).astype(np.uint8))
    return r1, r2


def remain_pair_text(rng, n, long_run=None, hi=150):
    r1, r2 = remain_pair_records(rng, n, long_run, hi)
    return text_of(r1), text_of(r2)


def selections(rng, n):
    """the active sets the tests format: all pairs, none, every other pair, only the last pair, a random third"""
    third = np.sort(rng.choice(n, max(n // 3, 1 if n > 1 else 0), replace=False)) if n > 1 else np.zeros(0, np.int64)
    return {"all": np.arange(n), "none": np.zeros(0, np.int64), "every_other": np.arange(0, n, 2), "last": np.array([n - 1]), "third": third}


class HostRemain(HostRows):
    """the checker: cm_fastq_next on files with the bytes t1 / t2 (pam_text_util.HostRows), then cm_write_remain_records"""

    def __init__(self, tmpdir, t1, t2, n, tag="rem", chrs=CHRS):
        super().__init__(tmpdir, t1, t2, n, tag=tag, chrs=chrs)

    def names2(self):
        fb, n = self.batch.fb, self.batch.n
        off = np.ctypeslib.as_array(fb.name_off2, (n + 1,))
        raw = C.string_at(fb.names2, int(off[n])) if int(off[n]) else b""
        return [raw[int(off[i]):int(off[i + 1])].split(b"\0")[0] for i in range(n)]

    def files(self, states, sel, chrs=None):
        """(bytes of file 1, bytes of file 2) of cm_write_remain_records for the pairs `sel` with their states"""
        self._k += 1
        p = [os.path.join(self.dir, f"{self.tag}_{self._k}_R{m}.fastq") for m in (1, 2)]
        w = cl.RecordWriter(p[0], p[1], self.chrs if chrs is None else chrs)
        recs = np.zeros(len(sel), cl.RECORD_DTYPE)
        recs["pair"] = sel
        recs["state"] = np.ascontiguousarray(states, dtype=cl.MAPPED_DTYPE)[np.asarray(sel, np.int64)]
        rc = w.L.cm_write_remain_records(w.h, C.byref(self.batch.fb), recs.ctypes.data, len(recs))
        w.close()
        assert rc == 0
        return open(p[0], "rb").read(), open(p[1], "rb").read()


def gspos_of(m, chrs):
    shift = chrs[int(m["chr_id"])][2] if 0 <= int(m["chr_id"]) < len(chrs) else 0
    g = (int(m["contig_num"]) * CONTIG_SIZE + ((int(m["spos_r1"]) + shift) & 0xFFFFFFFF)) & (2 ** 64 - 1)
    return g - 2 ** 64 if g >= 2 ** 63 else g


def key_value(m, chrs):
    """what cm_format_remain's out_keys holds for state m"""
    return gspos_of(m, chrs) if int(m["type"]) in MAPPED_TYPES else 0


def plain_record(name: bytes, m, seq: bytes, qual: bytes, chrs):
    """a record the plain way: the format string of write_read_category"""
    if int(m["type"]) in MAPPED_TYPES:
        cn = chrs[int(m["chr_id"])][0] if 0 <= int(m["chr_id"]) < len(chrs) else "-"
        i32 = lambda v: int(np.uint32(v).astype(np.int32))
        h = " %d %d %s %u %u %d %u %u %s %d %s %u %u %d %u %u %s %d %d %d %d %d" % (
            gspos_of(m, chrs), m["type"], cn, m["spos_r1"], m["epos_r1"], i32(m["mlen_r1"]), m["qspos_r1"], m["qepos_r1"], "+" if m["r1_forward"] else "-", m["ed_r1"],
            cn, m["spos_r2"], m["epos_r2"], i32(m["mlen_r2"]), m["qspos_r2"], m["qepos_r2"], "+" if m["r2_forward"] else "-", m["ed_r2"], m["tlen"], m["junc_num"],
            int(m["gm_compatible"] != 0), m["contig_num"])
    else:
        h = " * %d%s" % (m["type"], STARS)
    return b"@" + name + h.encode() + b"\n" + seq + b"\n+\n" + qual + b"\n"


def parsed_key(header: bytes):
    """key_of of host_circ.cpp on a header line: field 2 (fields: runs of non-blanks) as a signed decimal, 0 without digits"""
    i, n = 0, len(header)
    blank = (0x20, 0x09)
    while i < n and header[i] in blank:
        i += 1
    while i < n and header[i] not in blank:
        i += 1
    while i < n and header[i] in blank:
        i += 1
    neg = i < n and header[i] == 0x2D
    i += neg
    d = i
    while d < n and 0x30 <= header[d] <= 0x39:
        d += 1
    v = int(header[i:d]) if d > i else 0
    return -v if neg else v


def split_records(data: bytes, lens):
    """the records of a file whose reads have the lengths `lens`: a list of (header line, bases, qualities); the bases and the
    qualities are cut by length (either may hold a line feed's neighbours: '@', '+', NUL)"""
    out, p = [], 0
    for ln in lens:
        e = data.index(b"\n", p)
        out.append((data[p:e], data[e + 1:e + 1 + ln], data[e + 1 + ln + 3:e + 1 + 2 * ln + 3]))
        assert data[e + 1 + ln:e + 4 + ln] == b"\n+\n" and data[e + 4 + 2 * ln:e + 5 + 2 * ln] == b"\n"
        p = e + 5 + 2 * ln
    assert p == len(data)
    return out


class Emu:
    """emu_format_remain over the host parser's arrays of a batch, or over names / qualities given (the tokeniser emulation's)"""

    def __init__(self, E, h: HostRemain, names=None, names2=None, quals=None):
        self.E, self.n = E, h.batch.n
        self.seq1, self.off1, self.seq2, self.off2, self.qual1, self.qual2 = h.arrays()
        if quals is not None:
            self.qual1, self.qual2 = quals
        self.nm = []
        for given, parsed in ((names, h.names), (names2, h.names2)):
            if given is None:
                nm = parsed()
                given = (np.frombuffer(b"".join(nm) + b"\xa5", np.uint8).copy(), np.concatenate([[0], np.cumsum([len(x) for x in nm])]).astype(np.uint32))
            self.nm.append(given)

    def format(self, states, sel, first=0, count=None, caps=None, seed=1, chrs=CHRS, window=0, keys=True):
        st = np.ascontiguousarray(states, dtype=cl.MAPPED_DTYPE)
        sel = np.ascontiguousarray(sel, dtype=np.uint32)
        cnt = (1 << 64) - 1 if count is None else count
        n_out = max(len(sel) - first, 0) if count is None else count
        table = cl.chr_array(list(chrs))
        got, n_rec, stats, writes = np.zeros(2, np.uint64), C.c_uint64(0), np.zeros(4, np.uint64), np.zeros(2, np.uint64)
        kk = np.full(n_out + 1, -7, np.int64)
        a = [x.ctypes.data for x in (self.nm[0][0], self.nm[0][1], self.nm[1][0], self.nm[1][1], self.seq1, self.off1, self.seq2, self.off2, self.qual1, self.qual2)]

        def call(b1, c1, b2, c2):
            return self.E.emu_format_remain(st.ctypes.data, self.n, sel.ctypes.data if len(sel) else None, len(sel), *a, table, len(chrs), first, cnt,
                                            b1, c1, b2, c2, got.ctypes.data, kk.ctypes.data if keys else None, C.byref(n_rec), stats.ctypes.data, seed, window,
                                            writes.ctypes.data)
        if caps is None:
            rc = call(None, 0, None, 0)
            assert rc == (CM_ELIMIT if got.any() else 0), rc
            caps = (int(got[0]), int(got[1]))
        bufs = [np.full(c + 64, 0xA5, np.uint8) for c in caps]
        rc = call(bufs[0].ctypes.data, caps[0], bufs[1].ctypes.data, caps[1])
        assert kk[-1] == -7
        return rc, [int(x) for x in got], bufs, kk[:-1], int(n_rec.value), [int(x) for x in stats], [int(x) for x in writes]
