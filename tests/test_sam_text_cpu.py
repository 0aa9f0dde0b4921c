"""The device-side SAM formatter without a device: the bodies of circminer_amd/csrc/cm_sam_text.h and the plan of cm_rows_text.h run
by a host emulation (tests/hostemu_sam.cpp, tests/hostemu_rows.h: shuffled items, spans and lanes, every write of every call caught in shadow buffers and counted) against the
project's own host writer -- cm_fastq_next on files holding the same bytes, then cm_write_sam with the same states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from circminer_amd import lib as cl
from pam_text_util import CHRS
from sam_text_util import SPAN_PAIRS, SPAN_RECS, WINDOW, HostSam, reversed_records, sam_mapped, sam_pair_text, sam_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CM_EINVAL, CM_ESTATE, CM_ELIMIT = -1, -5, -6
N_MANY = 40 * SPAN_PAIRS + 3                                            # about 40 spans


@pytest.fixture(scope="module")
def emu_sam(built):
    out_dir = os.path.join(ROOT, "tests", "_hostemu")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libcmemu_sam.so")
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "hostemu_sam.cpp"), os.path.join(ROOT, "tests", "hostemu_rows.h"), os.path.join(csrc, "cm_sam_text.h"),
            os.path.join(csrc, "cm_rows_text.h"), os.path.join(csrc, "cm_fastq_text.h"), os.path.join(ROOT, "include", "circminer_hot.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-I", os.path.join(ROOT, "tests"),
                               srcs[0], "-o", so])
    E = C.CDLL(so)
    vp = C.c_void_p
    E.emu_quals.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp]
    E.emu_quals.restype = C.c_int
    E.emu_format_sam.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(cl.ChrInfo), C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_uint64,
                                 C.POINTER(C.c_uint64), vp, C.c_uint64, C.c_uint32, vp, vp]
    E.emu_format_sam.restype = C.c_int
    return E


class Emu:
    """emu_format_sam over the host parser's arrays of a batch (names without their NULs, as the device keeps them)"""

    def __init__(self, E, h: HostSam, quals=None):
        self.E, self.n = E, h.batch.n
        self.seq1, self.off1, self.seq2, self.off2, self.qual1, self.qual2 = h.arrays()
        if quals is not None:
            self.qual1, self.qual2 = quals
        names = h.names()
        self.names = np.frombuffer(b"".join(names) + b"\xa5", np.uint8).copy()
        self.name_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint32)
        self.table = cl.chr_array(CHRS)

    def format(self, states, first=0, count=None, cap=None, seed=1, n_chr=len(CHRS), window=0):
        count = self.n - first if count is None else count
        st = np.ascontiguousarray(states, dtype=cl.MAPPED_DTYPE)
        got, stats = C.c_uint64(0), np.zeros(4, np.uint64)
        rec_off, writes = np.zeros(2 * count + 1, np.uint32), np.zeros(3, np.uint64)
        a = [x.ctypes.data for x in (st, self.names, self.name_off, self.seq1, self.off1, self.seq2, self.off2, self.qual1, self.qual2)]

        def call(buf, cap, stats_p):
            return self.E.emu_format_sam(a[0], self.n, *a[1:], self.table, n_chr, first, count, buf, cap, C.byref(got), stats_p, seed, window,
                                         rec_off.ctypes.data, writes.ctypes.data)
        if cap is None:
            rc = call(None, 0, None)
            assert rc == (CM_ELIMIT if got.value else 0)
            cap = got.value
        buf = np.full(cap + 64, 0xA5, np.uint8)
        rc = call(buf.ctypes.data, cap, stats.ctypes.data)
        return rc, got.value, buf, [int(x) for x in stats], rec_off, [int(x) for x in writes]


def _check(e, h, st, first=0, count=None, **kw):
    """the emulated records of a range == the host writer's; every byte written once; the length body == the bytes produced"""
    count = e.n - first if count is None else count
    rc, got, buf, stats, rec_off, writes = e.format(st, first, count, **kw)
    rows = h.rows(st, first, count, chrs=CHRS[:kw["n_chr"]] if "n_chr" in kw else None)
    assert rc == 0 and got == len(rows), (first, count, got, len(rows))
    assert buf[:got].tobytes() == rows and bool((buf[got:] == 0xA5).all()), (first, count)
    if count:
        assert writes == [1, 1, 0], writes
        lines = rows.split(b"\n")[:-1]
        assert len(lines) == 2 * count and np.array_equal(np.diff(rec_off.astype(np.int64)), [len(x) + 1 for x in lines])
    assert stats[0] == 2 * count and stats[1] == got and stats[2] + stats[3] == (2 * count + SPAN_RECS - 1) // SPAN_RECS
    return rows, stats


@pytest.mark.parametrize("n", [1, SPAN_PAIRS - 1, SPAN_PAIRS, SPAN_PAIRS + 1, N_MANY])
def test_emulated_records_equal_the_host_writer(emu_sam, tmp_path, n):
    rng = np.random.default_rng(n)
    st = sam_states(n)
    long_run = (n // 2, min(n, n // 2 + 40)) if n > SPAN_PAIRS else None      # names of 300 - 400 bytes: spans that cross the window
    t1, t2, placed = sam_pair_text(rng, n, st, long_run)
    h = HostSam(tmp_path, t1, t2, n)
    e = Emu(emu_sam, h)
    if n == N_MANY:                                                            # the reads that decide the rules are all there
        assert placed == {"short": 18, "odd_rev": 15, "odd_fwd": 15, "lower": 2}, placed
    # the kept qualities: k_ft_qual_copy's body over the text == the host parser's
    for text, off, want in ((t1, e.off1, e.qual1), (t2, e.off2, e.qual2)):
        q = np.full(int(off[n]) + 1, 0xA5, np.uint8)
        a = np.frombuffer(text, np.uint8)
        assert emu_sam.emu_quals(a.ctypes.data, len(text), n, off.ctypes.data, n, q.ctypes.data) == 0
        assert np.array_equal(q[:-1], want) and q[-1] == 0xA5
    # whole: the directed states and all-zero states, by the window's rule, all direct, and with a window that splits the paths
    for states in (np.zeros(n, cl.MAPPED_DTYPE), st):
        rows, stats = _check(e, h, states, seed=n + 1)
        if n == N_MANY:             # 16 records with names of 300 bytes or more and their reads are more than a window; 9 pairs hold 5 such
            assert stats[2] > 0 and stats[3] > 0                                # both paths of the row body
        _, stats = _check(e, h, states, seed=n + 2, window=1)
        assert stats[2] == 0
        _check(e, h, states, seed=n + 3, window=3000)
    if n == N_MANY:
        m = sam_mapped(st["type"])
        r1, r2 = reversed_records(st)
        assert m.any() and (~m).any() and r1.any() and r2.any() and (m & ~r1).any()
        assert b"\t2147483647\t" in rows and b"\t4294967295\t" in rows and b"JC:i:65535\tTC:i:1\n" in rows and b"AT:i:-2147483648\t" in rows
    # ranges that cut a span, an empty one, one at the end
    for first, count in ((0, 0), (n, 0), (n - 1, 1), (n // 3, n - n // 3), ((SPAN_PAIRS - 1) % n, min(2, n - (SPAN_PAIRS - 1) % n)), (0, min(n, SPAN_PAIRS + 1)),
                         (n // 2, min(n - n // 2, 70))):
        _check(e, h, st, first, count, seed=first + count)
    # a cap that is too small: the needed size, and nothing written
    rows = h.rows(st)
    for cap in (len(rows) - 1, len(rows) // 2, 0):
        rc, got, buf, stats, _, _ = e.format(st, cap=cap)
        assert rc == CM_ELIMIT and got == len(rows) and bool((buf == 0xA5).all()) and stats == [0, 0, 0, 0]
    assert e.format(st, cap=len(rows))[:2] == (0, len(rows))
    # refusals of the range
    assert e.format(st, n, 1, cap=10)[0] == CM_EINVAL and e.format(st, 0, n + 1, cap=10)[0] == CM_EINVAL and e.format(st, n + 1, 0, cap=10)[0] == CM_EINVAL
    h.close()


def test_every_combination_is_among_the_first_64_states():
    st = sam_states(64)                                                  # (asserts the 24 combinations itself)
    assert (st["tlen"] != -2 ** 31).all() and (sam_states(700)["tlen"] == -2 ** 31 + 1).any()
    # the SAM rule is not the PAM rule: negative types and 3 / 4 fall on different sides
    assert sam_mapped([-1, -2 ** 31, 0, 1, 2, 5, 7]).all() and not sam_mapped([3, 4, 6, 8, 13, 14, 2 ** 31 - 1]).any()


def test_emulated_records_without_a_chromosome_table(emu_sam, tmp_path):
    """n_chr = 0: every mapped record's RNAME is '-'"""
    n = 70
    st = sam_states(n)
    t1, t2, _ = sam_pair_text(np.random.default_rng(3), n, st)
    h = HostSam(tmp_path, t1, t2, n, chrs=[])
    e = Emu(emu_sam, h)
    rows, _ = _check(e, h, st, n_chr=0)
    assert b"\t-\t" in rows
    h.close()


def test_the_window_constants_are_the_headers():
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    assert f"SPAN_RECS = {SPAN_RECS};" in open(os.path.join(csrc, "cm_sam_text.h")).read()
    assert f"WINDOW = {WINDOW};" in open(os.path.join(csrc, "cm_rows_text.h")).read()
