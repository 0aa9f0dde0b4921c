"""The device-side PAM formatter without a device: the bodies of circminer_amd/csrc/cm_pam_text.h and the plan of cm_rows_text.h run
by a host emulation (tests/hostemu_pam.cpp, tests/hostemu_rows.h: shuffled rows, spans, lanes and copy order, every write of every
call caught in shadow buffers and counted) against the project's own host
writer -- cm_fastq_next on files holding the same bytes, then cm_write_pam with the same states; cm_write_bytes against a plain
file write."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from circminer_amd import lib as cl
from pam_text_util import CHRS, MAPPED_TYPES, HostRows, directed_states, pair_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CM_EINVAL, CM_ESTATE, CM_ELIMIT, CM_EIO = -1, -5, -6, -7


@pytest.fixture(scope="module")
def emu_pam(built):
    out_dir = os.path.join(ROOT, "tests", "_hostemu")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libcmemu_pam.so")
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "hostemu_pam.cpp"), os.path.join(ROOT, "tests", "hostemu_rows.h"), os.path.join(csrc, "cm_pam_text.h"),
            os.path.join(csrc, "cm_rows_text.h"), os.path.join(csrc, "cm_fastq_text.h"), os.path.join(ROOT, "include", "circminer_hot.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-I", os.path.join(ROOT, "tests"),
                               srcs[0], "-o", so])
    E = C.CDLL(so)
    vp = C.c_void_p
    E.emu_names.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, vp, vp]
    E.emu_names.restype = C.c_int
    E.emu_format_pam.argtypes = [vp, C.c_uint64, vp, vp, C.POINTER(cl.ChrInfo), C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), vp,
                                 C.c_uint64, C.c_uint32, vp, vp]
    E.emu_format_pam.restype = C.c_int
    return E


class Emu:
    """names of the first n records of t1 through the emulation, then emu_format_pam over them"""

    def __init__(self, E, t1: bytes, n, seed=1):
        self.E, self.n = E, n
        a = np.frombuffer(t1, np.uint8)
        self.names = np.full(len(t1) + 1, 0xA5, np.uint8)
        self.off = np.zeros(n + 1, np.uint32)
        assert E.emu_names(a.ctypes.data, len(t1), n, seed, self.names.ctypes.data, self.off.ctypes.data) == 0
        self.table = cl.chr_array(CHRS)

    def format(self, states, first=0, count=None, cap=None, seed=1, n_chr=len(CHRS), window=0):
        """(rc, bytes, buffer, stats, writes); an emulation that found a byte written outside its span or a byte of a window
        not written exactly once fails here"""
        count = self.n - first if count is None else count
        st = np.ascontiguousarray(states, dtype=cl.MAPPED_DTYPE)
        got, stats, writes = C.c_uint64(0), np.zeros(4, np.uint64), np.zeros(3, np.uint64)

        def call(buf, cap, stats_p):
            rc = self.E.emu_format_pam(st.ctypes.data, self.n, self.names.ctypes.data, self.off.ctypes.data, self.table, n_chr, first, count, buf, cap,
                                       C.byref(got), stats_p, seed, window, None, writes.ctypes.data)
            assert rc not in (-100, -101), rc
            return rc
        if cap is None:
            rc = call(None, 0, None)
            assert rc == (CM_ELIMIT if got.value else 0)
            cap = got.value
        buf = np.full(cap + 64, 0xA5, np.uint8)
        rc = call(buf.ctypes.data, cap, stats.ctypes.data)
        return rc, got.value, buf, [int(x) for x in stats], [int(x) for x in writes]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_emulated_names_and_rows_equal_the_host_writer(emu_pam, tmp_path, n):
    rng = np.random.default_rng(n)
    long_run = (n // 2, min(n, n // 2 + 90)) if n >= 64 else None             # names of 300 - 400 bytes: spans that cross the window
    t1, t2 = pair_text(rng, n, long_run)
    h = HostRows(tmp_path, t1, t2, n)
    e = Emu(emu_pam, t1, n, seed=n)
    # names + offsets against the host parser
    want = h.names()
    assert [bytes(e.names[int(e.off[i]):int(e.off[i + 1])]) for i in range(n)] == want
    assert int(e.off[0]) == 0 and int(e.off[n]) == sum(len(x) for x in want) and bool((e.names[int(e.off[n]):] == 0xA5).all())
    assert n < 12 or {b"", b"a", b"q", b"ta\tb", b"nu"} <= set(want)
    # rows against cm_write_pam: the directed states, and all-zero states (the shortest mapped rows)
    st = directed_states(n)
    # ... by the window's rule, all direct, and with a window that splits the paths otherwise; every byte written exactly once
    for states in (np.zeros(n, cl.MAPPED_DTYPE), st):
        rows = h.rows(states)
        for window, seed in ((0, n + 1), (1, n + 2), (3000, n + 3)):
            rc, got, buf, stats, writes = e.format(states, seed=seed, window=window)
            assert rc == 0 and got == len(rows) and buf[:got].tobytes() == rows and bool((buf[got:] == 0xA5).all()), window
            assert writes == [1, 1, 0], (window, writes)
            assert stats[0] == n and stats[1] == got and stats[2] + stats[3] == (n + 63) // 64
            if window == 0 and long_run and n >= 65:                              # (64 rows are one span)
                assert stats[2] > 0 and stats[3] > 0                              # both paths of the row kernel
            if window == 1:
                assert stats[2] == 0
    if n >= 700:
        types = set(int(t) for t in st["type"])
        assert types >= set(range(14)) | {-1, 14} and b"\t-2147483648\t" in rows and b"\t4294967295\t" in rows and b"\t65535\t1\t" in rows
    # ranges that cut a 64-row group, an empty one, one at the end
    for first, count in ((0, 0), (n, 0), (n - 1, 1), (n // 3, n - n // 3), (63 % n, min(2, n - 63 % n)), (0, min(n, 65)), (n // 2, min(n - n // 2, 70))):
        rc, got, buf, stats, writes = e.format(st, first, count, seed=first + count)
        rows = h.rows(st, first, count)
        assert rc == 0 and got == len(rows) and buf[:got].tobytes() == rows and bool((buf[got:] == 0xA5).all()), (first, count)
        assert count == 0 or writes == [1, 1, 0], (first, count, writes)
        assert stats[0] == count and stats[2] + stats[3] == (count + 63) // 64
    # a cap that is too small: the needed size, and nothing written
    rows = h.rows(st)
    for cap in (len(rows) - 1, len(rows) // 2, 0):
        rc, got, buf, stats, _ = e.format(st, cap=cap)
        assert rc == CM_ELIMIT and got == len(rows) and bool((buf == 0xA5).all()) and stats == [0, 0, 0, 0]
    rc, got, buf, _, _ = e.format(st, cap=len(rows))
    assert rc == 0 and got == len(rows)
    # refusals of the range
    assert e.format(st, n, 1, cap=10)[0] == CM_EINVAL and e.format(st, 0, n + 1, cap=10)[0] == CM_EINVAL and e.format(st, n + 1, 0, cap=10)[0] == CM_EINVAL
    h.close()


def test_every_boundary_meets_a_mapped_type():
    """the directed states really print what they are meant to: over 700 rows every value of every field occurs in a row of a
    mapped type, and both forms of a row occur"""
    from pam_text_util import INT_VALUES, MLEN_VALUES, U32_FIELDS, U32_VALUES
    st = directed_states(700)
    mapped = np.isin(st["type"], MAPPED_TYPES)
    assert mapped.any() and (~mapped).any()
    for f in U32_FIELDS:
        assert set(int(v) for v in st[f][mapped]) == set(U32_VALUES)
    for f in ("mlen_r1", "mlen_r2"):
        assert set(int(v) for v in st[f][mapped]) == set(MLEN_VALUES)
    for f in ("ed_r1", "ed_r2", "tlen"):
        assert set(int(v) for v in st[f][mapped]) == set(INT_VALUES)
    assert set(int(v) for v in st["chr_id"][mapped]) == {-1, 0, len(CHRS) - 1, len(CHRS)}
    assert set(int(v) for v in st["gm_compatible"][mapped]) == {0, 1, 255} and set(int(v) for v in st["junc_num"][mapped]) == {0, 65535}
    assert set(zip(st["r1_forward"][mapped].tolist(), st["r2_forward"][mapped].tolist())) == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_emulated_rows_without_a_chromosome_table(emu_pam, tmp_path):
    """n_chr = 0: every chr_id prints '-'"""
    n = 130
    t1, t2 = pair_text(np.random.default_rng(3), n)
    h = HostRows(tmp_path, t1, t2, n, chrs=[])
    e = Emu(emu_pam, t1, n)
    st = directed_states(n)
    rc, got, buf, _, writes = e.format(st, n_chr=0)
    assert rc == 0 and buf[:got].tobytes() == h.rows(st) and writes == [1, 1, 0]
    h.close()


def test_write_bytes_equals_a_plain_write(built, tmp_path):
    """cm_write_bytes: pieces smaller and larger than the writer's buffer, between rows of cm_write_pam; /dev/full is CM_EIO"""
    rng = np.random.default_rng(8)
    n = 300
    t1, t2 = pair_text(rng, n)
    h = HostRows(tmp_path, t1, t2, n, tag="wb")
    st = directed_states(n)
    pieces = [b"", b"x", bytes(rng.integers(0, 256, 70_000).astype(np.uint8)), bytes(rng.integers(0, 256, (5 << 20) + 3).astype(np.uint8)), b"tail\n"]
    path = str(tmp_path / "bytes.out")
    w = cl.RecordWriter(path, None, CHRS)
    want = b""
    for p in pieces:
        w.write_bytes(p)
        w.write_pam(h.batch, st, np.arange(5, dtype=np.uint64))
        want += p + h.rows(st, 0, 5)
    w.close()
    assert open(path, "rb").read() == want
    L = cl.load()
    assert L.cm_write_bytes(None, None, 0) == CM_EINVAL
    if os.path.exists("/dev/full"):
        w = cl.RecordWriter("/dev/full", None, CHRS)
        w.write_bytes(b"abc")                                                      # buffered: may not notice yet
        with pytest.raises(RuntimeError):
            w.close()
        w = cl.RecordWriter("/dev/full", None, CHRS)
        with pytest.raises(RuntimeError, match=r"\(-7\)"):
            w.write_bytes(pieces[3])                                               # larger than the buffer: written through, noticed at once
        with pytest.raises(RuntimeError):
            w.close()
    h.close()
