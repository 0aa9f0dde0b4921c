"""The device-side FASTQ tokeniser without a device: the bodies of circminer_amd/csrc/cm_fastq_text.h run by a host emulation
(tests/hostemu_fastq.cpp, shuffled chunk / record / lane order) against the project's host parser cm_fastq_next on files holding
the same bytes; the raw-block mode of the reader; cm_write_remain_text against cm_write_remain_records."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from circminer_amd import lib as cl
from fastq_text_util import (CARRIED_HEADER, MALFORMED, HostParse, check_against_host, malformed, records, text_of, whole_records)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_BAD1, RES_BAD2, RES_PAIRS = 0, 1, 5


@pytest.fixture(scope="module")
def emu_ft(built):
    out_dir = os.path.join(ROOT, "tests", "_hostemu")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libcmemu_fastq.so")
    srcs = [os.path.join(ROOT, "tests", "hostemu_fastq.cpp"), os.path.join(ROOT, "circminer_amd", "csrc", "cm_fastq_text.h"),
            os.path.join(ROOT, "include", "circminer_hot.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "circminer_amd", "csrc"), srcs[0], "-o", so])
    E = C.CDLL(so)
    vp = C.c_void_p
    E.emu_stage_text.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp, vp, vp, vp,
                                 C.POINTER(cl.TextBatch), vp]
    E.emu_stage_text.restype = C.c_int
    return E


class Emu:
    def __init__(self, E, t1: bytes, t2: bytes, max_pairs, flags=3, max_read_len=300, kmer=20, seed=1):
        a1, a2 = np.frombuffer(t1, np.uint8), np.frombuffer(t2, np.uint8)
        cap = min(max_pairs, min(len(t1), len(t2)) // 4) + 1
        self.seq1, self.seq2 = np.zeros(len(t1) + 1, np.uint8), np.zeros(len(t2) + 1, np.uint8)
        self.off1, self.off2, self.rec1, self.rec2 = (np.zeros(cap, np.uint64) for _ in range(4))
        self.tb = cl.TextBatch()
        self.res = np.zeros(16, np.uint64)
        self.rc = E.emu_stage_text(a1.ctypes.data if len(t1) else None, len(t1), a2.ctypes.data if len(t2) else None, len(t2), max_pairs, flags,
                                   max_read_len, kmer, seed, self.seq1.ctypes.data, self.off1.ctypes.data, self.rec1.ctypes.data, self.seq2.ctypes.data,
                                   self.off2.ctypes.data, self.rec2.ctypes.data, C.byref(self.tb), self.res.ctypes.data)
        self.n = int(self.tb.n_pairs)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_emulated_tokeniser_equals_host_parser(emu_ft, tmp_path, n):
    """whole files (both end-of-input flags), with and without a final line feed, a zero-length read, max_pairs below the file"""
    rng = np.random.default_rng(n)
    r1 = records(rng, n, zero_at=(0, n // 2) if n > 1 else (), mate=1)      # (not the last one: without the final line feed
    r2 = records(rng, n, zero_at=(n - 2,) if n > 1 else (), mate=2)         #  its empty quality line would not be a line)
    for last_nl in (True, False):
        t1, t2 = text_of(r1, last_nl), text_of(r2, last_nl)
        for mp in sorted({n, n + 5, max(1, n // 2)}):
            h = HostParse(tmp_path, t1, t2, mp, tag=f"w{n}")
            e = Emu(emu_ft, t1, t2, mp, seed=n + mp)
            check_against_host(e, h, min(n, mp), t1, t2)
            assert h.n == e.n


def test_emulated_tokeniser_on_cut_blocks(emu_ft, tmp_path):
    """flags 0: blocks cut inside a header, a sequence line, right behind a line feed and at a record boundary -- the tail is
    not consumed, used* is the host's record boundary, the pairs are those the host parses first"""
    rng = np.random.default_rng(5)
    n = 300
    r1, r2 = records(rng, n, mate=1), records(rng, n, mate=2, zero_at=(7,))
    t1, t2 = text_of(r1), text_of(r2)
    h = HostParse(tmp_path, t1, t2, n, tag="cut")
    rec1, _, _ = whole_records(t1, True)
    rec2, _, _ = whole_records(t2, True)
    cuts = [int(rec1[200]) + 3, int(rec1[200]) + len(r1[200][0]) + 10, int(rec1[201]), int(rec1[201]) - 1, 20_000, 1, 0]
    for cut in cuts:
        b1, b2 = t1[:cut], t2[:cut]
        want = min(whole_records(b1, False)[1], whole_records(b2, False)[1])
        assert whole_records(b1, False)[1] != whole_records(b2, False)[1] or cut < 400      # names differ in length: a_1 != a_2
        e = Emu(emu_ft, b1, b2, n, flags=0, seed=cut)
        check_against_host(e, h, want, b1, b2, eof=False)
        e = Emu(emu_ft, b1, b2, 50, flags=0, seed=cut)                                      # max_pairs below what the block holds
        check_against_host(e, h, min(want, 50), b1, b2, eof=False)


def test_emulated_verdicts_equal_host_parser(emu_ft, tmp_path):
    """every malformed case on either file in the first, a middle and the last record (CM_EINVAL where the host parser says so);
    trailing lines, an R2 that ends early, a legal '@' quality, the carried header, the read-length verdicts"""
    rng = np.random.default_rng(11)
    n = 40                                       # ~ 9 KB per file: records straddle the 1-KB newline chunks
    r1, r2 = records(rng, n, mate=1), records(rng, n, mate=2)
    for f in (0, 1):
        for i in (0, n // 2, n - 1):
            for how in MALFORMED:
                b = [r1, r2]
                b[f] = malformed(b[f], i, how)
                t1, t2 = text_of(b[0]), text_of(b[1])
                h = HostParse(tmp_path, t1, t2, n, tag="bad")
                e = Emu(emu_ft, t1, t2, n, seed=i)
                assert h.rc == -1 and e.rc == -1, (f, i, how)
                assert int(e.res[RES_BAD1 + f]) >> 3 == i and int(e.res[RES_BAD2 - f]) == 2 ** 64 - 1      # the first malformed record, of that file
                e = Emu(emu_ft, t1, t2, i, seed=i) if i else None                # the batch ends in front of it: fine
                assert e is None or (e.rc == 0 and e.n == i)
    # two malformed records: the first one is reported
    t1 = text_of(malformed(malformed(r1, 30, "qual_long"), 12, "plus_empty"))
    e = Emu(emu_ft, t1, text_of(r2), n)
    assert e.rc == -1 and int(e.res[RES_BAD1]) >> 3 == 12
    # a quality line that starts with '@', a sequence line that starts with '+': legal, records are counted by line
    q = [list(x) for x in r1]
    q[3][3] = b"@" + q[3][3][1:]
    q[4][1] = b"+" + q[4][1][1:]
    t1, t2 = text_of(q), text_of(r2)
    check_against_host(Emu(emu_ft, t1, t2, n), HostParse(tmp_path, t1, t2, n, tag="at"), n, t1, t2)
    # lines behind the last whole record at the end of the input
    for tail in (b"\n", b"@x\nACGT\n", b"@x\nACGT\n+", b"\n\n\n"):
        for f in (0, 1):
            t = [text_of(r1), text_of(r2)]
            t[f] += tail
            h, e = HostParse(tmp_path, t[0], t[1], n + 1, tag="tail"), Emu(emu_ft, t[0], t[1], n + 1)
            assert h.rc == e.rc == -1, (tail, f)
            h, e = HostParse(tmp_path, t[0], t[1], n, tag="tail"), Emu(emu_ft, t[0], t[1], n)     # the batch is full without them
            assert h.rc == e.rc == 0 and e.n == h.n == n
            assert Emu(emu_ft, t[0], t[1], n + 1, flags=3 ^ (1 << f)).rc == 0                    # not the end of the input: a cut block
    # R2 ends before R1 / R1 before R2 (surplus R2 records are ignored)
    t1, t2 = text_of(r1), text_of(r2[:n - 3])
    assert HostParse(tmp_path, t1, t2, n, tag="short").rc == Emu(emu_ft, t1, t2, n).rc == -1
    assert HostParse(tmp_path, t1, t2, n - 3, tag="short").rc == Emu(emu_ft, t1, t2, n - 3).rc == 0
    assert Emu(emu_ft, t1, t2, n, flags=1).rc == 0 and Emu(emu_ft, t1, t2, n, flags=1).n == n - 3
    t1, t2 = text_of(r1[:n - 3]), text_of(r2)
    h, e = HostParse(tmp_path, t1, t2, n, tag="short"), Emu(emu_ft, t1, t2, n)
    check_against_host(e, h, n - 3, t1, t2)
    # the carried header: the device path refuses it in R1 (the host parser reads the state), R2's tokens are nobody's business
    c = [list(x) for x in r1]
    c[n // 2][0] = CARRIED_HEADER
    h = HostParse(tmp_path, text_of(c), text_of(r2), n, tag="car")
    e = Emu(emu_ft, text_of(c), text_of(r2), n)
    assert h.rc == 0 and h.prior and e.rc == -1 and int(e.res[RES_BAD1]) == (n // 2) << 3 | 4
    c2 = [list(x) for x in r2]
    c2[n // 2][0] = CARRIED_HEADER
    t1, t2 = text_of(r1), text_of(c2)
    h, e = HostParse(tmp_path, t1, t2, n, tag="car"), Emu(emu_ft, t1, t2, n)
    assert not h.prior
    check_against_host(e, h, n, t1, t2)
    # read length: check_reads' verdicts
    lg = [list(x) for x in r2]
    lg[5][1], lg[5][3] = b"A" * 301, b"I" * 301
    assert Emu(emu_ft, text_of(r1), text_of(lg), n, max_read_len=300).rc == -1
    assert Emu(emu_ft, text_of(r1), text_of(lg), n, max_read_len=301, kmer=14).rc == 0           # 21 seeds
    assert Emu(emu_ft, text_of(r1), text_of(lg), n, max_read_len=400, kmer=12).rc == -6          # 25 seeds: CM_ELIMIT
    # empty input
    e = Emu(emu_ft, b"", b"", 10)
    assert e.rc == 0 and e.n == 0


def test_emulated_tokeniser_random_files(emu_ft, tmp_path):
    """a few hundred random small files: every verdict and, where the host parser accepts the input, every array"""
    rng = np.random.default_rng(2024)
    agree = ok = 0
    for it in range(300):
        n1 = int(rng.integers(0, 12))
        n2 = n1 if rng.random() < 0.7 else int(rng.integers(0, 12))
        lo, hi = (0, 5) if it % 3 == 0 else (1, 90)
        r1, r2 = records(rng, n1, lo, hi, mate=1), records(rng, n2, lo, hi, mate=2)
        if rng.random() < 0.25 and n1:
            r1 = malformed(r1, int(rng.integers(0, n1)), MALFORMED[int(rng.integers(0, len(MALFORMED)))])
        if rng.random() < 0.25 and n2 and n2 <= n1:          # (surplus R2 records are validated by the host parser only: header says so)
            r2 = malformed(r2, int(rng.integers(0, n2)), MALFORMED[int(rng.integers(0, len(MALFORMED)))])
        t1, t2 = text_of(r1, rng.random() < 0.5), text_of(r2, rng.random() < 0.5)
        if rng.random() < 0.15:
            t1 += [b"\n", b"@", b"\r\n", b"@q\nAC\n+\n"][int(rng.integers(0, 4))]
        mp = int(rng.integers(1, 14))
        h, e = HostParse(tmp_path, t1, t2, mp, tag="rnd"), Emu(emu_ft, t1, t2, mp, seed=it)
        # the host parser validates min(a_2, max_pairs) records of R2, the device path the n it stages
        a1, a2 = whole_records(t1, True)[1], whole_records(t2, True)[1]
        r2_surplus = min(a2, mp) > min(a1, mp)
        if not (r2_surplus and h.rc == -1 and e.rc == 0):
            assert h.rc == e.rc, (it, h.rc, e.rc)
            agree += 1
        if h.rc == 0:
            check_against_host(e, h, h.n, t1, t2)
            ok += 1
    assert agree > 280 and ok > 100


def test_reader_text_blocks_carry_their_tails(tmp_path):
    """cm_fastq_next_text / cm_fastq_text_consumed: the blocks are the files' bytes in order, what was not consumed is the front
    of the next block, a block nothing was consumed of comes back larger, four generations stay valid; gzip is CM_EINVAL"""
    import gzip
    rng = np.random.default_rng(3)
    r1, r2 = records(rng, 900, mate=1), records(rng, 900, mate=2)
    t1, t2 = text_of(r1), text_of(r2, last_newline=False)
    h = HostParse(tmp_path, t1, t2, 1, tag="blk")
    rd = cl.FastqReader(*h.paths)
    pos = [0, 0]
    kept = []
    want = 16 << 10
    for it in range(1000):
        b1, e1, b2, e2 = rd.next_text(want)
        for x, (b, e, t) in enumerate(((b1, e1, t1), (b2, e2, t2))):
            assert bytes(b) == t[pos[x]:pos[x] + len(b)]
            assert e == (pos[x] + len(b) == len(t))
        kept.append((b1, pos[0]))
        for old, at in kept[-4:]:                                        # the three blocks before this one are still what they were
            assert bytes(old) == t1[at:at + len(old)]
        if it == 3:                                                     # nothing consumed: the same bytes again, and more
            rd.consumed(0, 0)
            n1, _, n2, _ = rd.next_text(want)
            assert len(n1) > len(b1) and bytes(n1[:len(b1)]) == bytes(b1) and bytes(n1) == t1[pos[0]:pos[0] + len(n1)]
            b1, b2 = n1, n2
            kept[-1] = (b1, pos[0])
        if e1 and e2 and len(b1) == 0:
            break
        used = [int(whole_records(bytes(b1), e1)[0][-1]), int(whole_records(bytes(b2), e2)[0][-1])]
        if it % 5 == 0:
            used[0] = int(whole_records(bytes(b1), e1)[0][0 if len(b1) < 4000 else 1])          # R1 lags behind: a longer tail
        rd.consumed(*used)
        pos[0] += used[0]
        pos[1] += used[1]
    assert pos == [len(t1), len(t2)]
    rd.close()
    # a shard's byte range is respected
    whole = []
    for rank in range(3):
        rd = cl.FastqReader(*h.paths, rank=rank, world=3, n_threads=2)
        got = b""
        while True:
            b1, e1, b2, e2 = rd.next_text(32 << 10)
            got += bytes(b1)
            rd.consumed(len(b1), len(b2))
            if e1:
                break
        rd.close()
        assert got.count(b"\n") == 4 * rd.n_pairs
        whole.append(got)
    assert b"".join(whole) == t1
    # gzip input stays on cm_fastq_next
    g1, g2 = os.path.join(str(tmp_path), "a_1.fq.gz"), os.path.join(str(tmp_path), "a_2.fq.gz")
    for p, t in ((g1, t1), (g2, t2)):
        with gzip.open(p, "wb") as f:
            f.write(t)
    rd = cl.FastqReader(g1, g2)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        rd.next_text(1 << 16)
    assert rd.next_batch(10).n == 10
    rd.close()


def test_write_remain_text_equals_write_remain_records(tmp_path):
    """the rows sliced from the text at the record starts == the rows written from the parsed batch, byte for byte"""
    rng = np.random.default_rng(8)
    n = 500
    r1, r2 = records(rng, n, mate=1, zero_at=(3,)), records(rng, n, mate=2, zero_at=(9,))
    r1[10][0] = b"@"                                        # no name at all
    r1[11][0] = b"@  lead/1  x"                             # spaces in front of the first token
    r2[12][0] = b"@a"                                       # shorter than the "/x" rule looks at
    r2[13][0] = b"@/2"
    chr_table = [("chr1", 1, 0, 5000), ("chr2", 1, 5050, 7000)]
    for last_nl in (True, False):
        t1, t2 = text_of(r1, last_nl), text_of(r2, last_nl)
        h = HostParse(tmp_path, t1, t2, n, tag="wr")
        rd = cl.FastqReader(*h.paths)
        batch = rd.next_batch(n)
        recs = np.zeros(0, cl.RECORD_DTYPE)
        sel = np.concatenate([[0, 3, 9, 10, 11, 12, 13, n - 1], rng.integers(0, n, 60)]).astype(np.uint64)
        recs = np.zeros(len(sel), cl.RECORD_DTYPE)
        recs["pair"] = sel
        st = recs["state"]
        st["type"] = rng.integers(0, 14, len(sel))
        for fld in ("spos_r1", "spos_r2", "epos_r1", "epos_r2", "mlen_r1", "mlen_r2", "qspos_r1", "qepos_r2"):
            st[fld] = rng.integers(0, 5000, len(sel))
        st["chr_id"] = rng.integers(-1, 2, len(sel))
        st["tlen"], st["ed_r1"], st["r1_forward"] = rng.integers(-500, 500, len(sel)), rng.integers(0, 5, len(sel)), rng.integers(0, 2, len(sel))
        recs["state"] = st
        out = {}
        for kind in ("records", "text"):
            p1, p2 = os.path.join(str(tmp_path), f"{kind}_1.fq"), os.path.join(str(tmp_path), f"{kind}_2.fq")
            w = cl.RecordWriter(p1, p2, chr_table)
            if kind == "records":
                assert w.L.cm_write_remain_records(w.h, C.byref(batch.fb), recs.ctypes.data, len(recs)) == 0
            else:
                w.write_remain_text(np.frombuffer(t1, np.uint8), whole_records(t1, True)[0], np.frombuffer(t2, np.uint8), whole_records(t2, True)[0], recs)
            w.close()
            out[kind] = (open(p1, "rb").read(), open(p2, "rb").read())
        rd.close()
        assert out["text"] == out["records"] and len(out["text"][0]) > 5000


def test_new_names_of_the_abi():
    L = cl.load()
    for name in ("cm_reads_stage_text", "cm_reads_peek", "cm_fastq_next_text", "cm_fastq_text_consumed", "cm_write_remain_text"):
        assert hasattr(L, name) and name in cl.EXPORTED_SYMBOLS
    assert C.sizeof(cl.TextBatch) == 32
    assert cl.MappingStats.device_parsed_batches.offset == cl.MappingStats.rounds.offset + 4 and C.sizeof(cl.MappingStats) == 176
    assert L.cm_reads_stage_text(None, None, 0, None, 0, 1, 3, None, None, C.byref(cl.TextBatch())) == -1      # without a context
