"""cm_format_remain on the device: the remain-FASTQ records of the resident batch's active set formatted by k_remain_len /
k_remain_rows from the states in HBM, the R1 names (flag bit 2), the qualities (bit 3) and the R2 names (bit 4) cm_reads_stage_text
keeps and the bases in the read buffers, against the project's own host writer -- cm_fastq_next on files holding the same bytes, then
cm_write_remain_records with the records cm_collect_records delivers -- byte for byte, both files; cm_mapping_run with
CM_REMAIN_DEVICE=1.

The span kernel takes 16 records per wave and an 8-KB window: 65 pairs are five spans, 4100 are 257; a run of 300 - 400-byte names in
both files and the 300-bp reads of the 24-seed build cross the window, the ranges cut a span.  A fresh batch has every pair active;
the subsets are the ones mapping leaves (the tiny two-contig data set), with the directed states poked over them.

The runs of cm_mapping_run share the process, as test_gpu_sam_text.py's do: the variables are read by every call."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from circminer_amd import lib as cl
from fastq_text_util import HostParse, check_against_host, whole_records
from pam_text_util import CHRS
from remain_text_util import CM_EINVAL, CM_ELIMIT, CM_ESTATE, SPAN_RECS, HostRemain, key_value, remain_pair_text, remain_states, split_records

pytestmark = pytest.mark.gpu
N_MANY = 4100
BITS = dict(keep_names=True, keep_quals=True, keep_names2=True)


class Dev:
    """stage_text -> swap -> peek_reads, in the shape check_against_host compares"""

    def __init__(self, hp, t1: bytes, t2: bytes, max_pairs, **bits):
        self.rc = 0
        self.tb, self.rec1, self.rec2 = hp.stage_text(t1, t2, max_pairs, **bits)
        self.n = int(self.tb.n_pairs)
        hp.swap()
        self.seq1, self.off1, self.seq2, self.off2 = hp.peek_reads()


def _rc(call, *a, **kw):
    """(error code, message) of a call that is refused"""
    with pytest.raises(RuntimeError) as e:
        call(*a, **kw)
    return int(str(e.value).split("(")[1].split(")")[0]), str(e.value)


@pytest.fixture(scope="module")
def hp_plain(built):
    hp = cl.HotPath(cl.default_params())
    yield hp
    hp.close()


@pytest.fixture(scope="module")
def hp_wide(built):
    hp = cl.HotPath(cl.default_params(kmer=14))                  # 300 / 14 = 21 seeds per read: the library's 24-seed build
    yield hp
    hp.close()


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    """per (n, longest read): the directed states, the two texts (special names in both files, a run of long names from 65 pairs
    on) and the host parser's view of them, made once"""
    tmp = tmp_path_factory.mktemp("remain_texts")
    out = {}

    def get(n, hi=150):
        if (n, hi) not in out:
            t1, t2 = remain_pair_text(np.random.default_rng(n + hi), n, (n // 2, min(n, n // 2 + 40)) if n >= 65 else None, hi)
            out[n, hi] = (t1, t2, HostParse(tmp, t1, t2, n, tag=f"p{n}_{hi}"), HostRemain(tmp, t1, t2, n, tag=f"r{n}_{hi}"), remain_states(n))
        return out[n, hi]
    yield get
    for v in out.values():
        v[3].close()


def _whole(hp, hrem, st, sel, chrs=CHRS):
    """format_remain of the whole active set == the host writer's files for `sel`; the keys; the counts"""
    f1, f2, keys, n_rec, stats = hp.format_remain(chrs, keys=True)
    want = hrem.files(st, sel, chrs=chrs)
    assert n_rec == len(sel) and (f1, f2) == want
    assert keys.tolist() == [key_value(st[int(p)], chrs) for p in sel]
    assert stats[:2] == [2 * len(sel), len(f1) + len(f2)] and stats[2] + stats[3] == 2 * ((len(sel) + SPAN_RECS - 1) // SPAN_RECS)
    return want, stats


@pytest.mark.parametrize("n", [1, 63, 64, 65, N_MANY])
def test_staging_with_and_without_bit_4(hp_plain, texts, n):
    """the staged arrays and verdicts are the host parser's with and without bit 4, alone and beside bits 2 and 3; format_remain
    needs all three and names the missing ones, the sibling formatters are served as before; the R2 names, read back through the
    second file of the fresh batch (every pair active), are the host parser's"""
    hp = hp_plain
    t1, t2, hparse, hrem, _ = texts(n)
    for names, quals, names2 in ((False, False, False), (False, False, True), (True, True, False), (True, False, True), (True, True, True)):
        e = Dev(hp, t1, t2, n, keep_names=names, keep_quals=quals, keep_names2=names2)
        check_against_host(e, hparse, n, t1, t2)
        if names:
            assert hp.format_pam(CHRS)[0].count(b"\n") == n
        if names and quals:
            assert hp.format_sam(CHRS)[0].count(b"\n") == 2 * n
        if not (names and quals and names2):
            rc, msg = _rc(hp.format_remain, CHRS)
            assert rc == CM_ESTATE and ("no R1 names" in msg) == (not names) and ("no qualities" in msg) == (not quals) and ("no R2 names" in msg) == (not names2), msg
    st = hp.download()[0]
    want, stats = _whole(hp, hrem, st, np.arange(n))
    recs2 = split_records(want[1], np.diff(hparse.off2.astype(np.int64)))
    assert all(hdr.startswith(b"@" + name + b" ") for (hdr, _, _), name in zip(recs2, hrem.names2()))
    if n >= 65:
        assert stats[2] > 0 and stats[3] > 0


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [65, N_MANY])
def test_directed_states(hp_plain, hp_wide, texts, n, wide):
    """stage with bits 2 | 3 | 4 -> swap -> poke_states(remain_states) -> format_remain: whole sets and ranges in pieces that cut a
    span of 16 records, the keys, another chromosome table and the first one again, in both kernel builds (reads of 300 bp in the
    24-seed one); both paths of the span kernel are taken"""
    hp = hp_wide if wide else hp_plain
    t1, t2, hparse, hrem, st = texts(n, 300 if wide else 150)
    e = Dev(hp, t1, t2, n, **BITS)
    check_against_host(e, hparse, n, t1, t2)
    hp.poke_states(st)
    assert hp.download()[0].tobytes() == st.tobytes()
    sel = np.arange(n)
    want, stats = _whole(hp, hrem, st, sel)
    assert stats[2] > 0 and stats[3] > 0
    for first, count in ((SPAN_RECS - 1, 2), (n // 3, 0), (n // 2 - 7, n - n // 2 + 7), (n - 1, 1), (n, 0), (5, None)):
        f1, f2, keys, n_rec, stats = hp.format_remain(CHRS, first=first, count=count, keys=True)
        c = n - first if count is None else count
        assert (f1, f2) == hrem.files(st, sel[first:first + c]) and n_rec == n, (first, count)
        assert keys.tolist() == [key_value(st[i], CHRS) for i in range(first, first + c)]
        assert stats[0] == 2 * c and stats[2] + stats[3] == 2 * ((c + SPAN_RECS - 1) // SPAN_RECS)
    pieces, at = [b"", b""], 0                                    # the set in pieces of 21 records: the files are their concatenation
    while at < min(n, 200):
        f1, f2, _, _, _ = hp.format_remain(CHRS, first=at, count=min(21, n - at))
        pieces = [pieces[0] + f1, pieces[1] + f2]
        at += 21
    full = hrem.files(st, sel[:min(at, n)])
    assert tuple(pieces) == full
    _whole(hp, hrem, st, sel, chrs=[])                            # another chromosome table (none): "-" and no shift in the key
    assert hp.format_remain(CHRS)[:2] == want                     # ... and the first table again
    assert hp.format_pam(CHRS)[0].count(b"\n") == n and hp.format_remain(CHRS)[:2] == want      # the siblings share the buffers


def test_refusals_leave_the_batch_intact(built, texts):
    hp = cl.HotPath(cl.default_params())
    L = cl.load()
    try:
        n = 65
        t1, t2, hparse, hrem, st = texts(n)
        table = cl.chr_array(CHRS)
        got, n_rec = (C.c_uint64 * 2)(), C.c_uint64(99)

        def raw(first, count, b1, c1, b2, c2, keys=None):
            return L.cm_format_remain(hp.h, table, len(CHRS), first, count, b1, c1, b2, c2, got, keys, C.byref(n_rec), None)
        assert raw(0, 0, None, 0, None, 0) == CM_ESTATE and n_rec.value == 0           # before any batch
        b = cl.ReadBatch(np.full((n, 40), ord("A"), np.uint8), np.full((n, 40), ord("C"), np.uint8))
        hp.upload(b)                                              # a batch from upload has neither names nor qualities
        fresh = hp.download()[0]
        n_rec.value = 99
        assert raw(0, 0, None, 0, None, 0) == CM_ESTATE and n_rec.value == n and hp.download()[0].tobytes() == fresh.tobytes()
        assert hp.stage_text(t1, t2, n, **BITS)[0].n_pairs == n
        hp.swap()
        hp.poke_states(st)
        want = hrem.files(st, np.arange(n))
        sizes = [len(want[0]), len(want[1])]
        bufs = [np.full(s + 8, 0xA5, np.uint8) for s in sizes]
        keys = np.full(n, -7, np.int64)

        def good():
            for x in bufs:
                x[:] = 0xA5
            assert raw(0, n, bufs[0].ctypes.data, sizes[0], bufs[1].ctypes.data, sizes[1], keys.ctypes.data) == 0 and list(got) == sizes
            for m in (0, 1):
                assert bufs[m][:sizes[m]].tobytes() == want[m] and bool((bufs[m][sizes[m]:] == 0xA5).all())
            assert keys.tolist() == [key_value(st[i], CHRS) for i in range(n)]
            keys[:] = -7
            for x in bufs:
                x[:] = 0xA5
        good()
        for first, count in ((n, 1), (0, n + 1), (n + 1, 0), (n + 1, 2 ** 64 - 1)):
            n_rec.value = 99
            assert raw(first, count, bufs[0].ctypes.data, sizes[0], bufs[1].ctypes.data, sizes[1]) == CM_EINVAL and n_rec.value == n and list(got) == [0, 0]
            good()
        assert raw(0, n, None, 5, bufs[1].ctypes.data, sizes[1]) == CM_EINVAL and raw(0, n, bufs[0].ctypes.data, sizes[0], None, 5) == CM_EINVAL
        good()
        for c1, c2 in ((sizes[0] - 1, sizes[1]), (sizes[0], sizes[1] - 1), (0, 0)):
            n_rec.value = 99
            assert raw(0, n, bufs[0].ctypes.data, c1, bufs[1].ctypes.data, c2, keys.ctypes.data) == CM_ELIMIT
            assert list(got) == sizes and n_rec.value == n and all(bool((x == 0xA5).all()) for x in bufs) and bool((keys == -7).all())      # the needed sizes, nothing written
            good()
        assert raw(0, 0, bufs[0].ctypes.data, 0, bufs[1].ctypes.data, 0) == 0 and list(got) == [0, 0] and n_rec.value == n
        assert raw(n, 2 ** 64 - 1, None, 0, None, 0) == 0 and list(got) == [0, 0]      # "to the end" from the end
        assert hp.download()[0].tobytes() == st.tobytes()
        s1, o1, _, _ = hp.peek_reads()
        assert np.array_equal(o1, hparse.off1) and np.array_equal(s1, hparse.seq1)
        rec = hp.collect_records()                               # the set is cm_collect_records'
        assert np.array_equal(rec["pair"], np.arange(n))
    finally:
        hp.close()


def test_names_and_qualities_follow_their_batch(ds_tiny2r, tmp_path):
    """stage A -> swap -> a stage without the bits (dropped) -> stage B -> map_rounds (B's first round is prefetched out of the
    tokeniser's buffers, B's text has overwritten A's): format_remain gives the records of the pairs mapping left active, with A's
    names of both files, bases and qualities; then the directed states over the same active set; after the swap B's"""
    ds = ds_tiny2r
    hp = cl.HotPath(cl.default_params(kmer=ds.kmer))
    try:
        for ci in range(ds.hi.n_contigs):
            hp.load_contig(ci, ds.hi.views[ci], ds.hi.annots[ci])
        slots = list(range(ds.hi.n_contigs))
        n = ds.batch.n
        h = n // 2
        rng = np.random.default_rng(5)
        paths = []
        for mate, arr in ((1, ds.d.seq1), (2, ds.d.seq2)):        # (names that differ between the files, qualities from record to record)
            paths.append(str(tmp_path / f"in_{mate}.fq"))
            with open(paths[-1], "wb") as f:
                for i in range(n):
                    s = arr[i].tobytes()
                    f.write(b"@pair%d%s/%d\n%s\n+\n%s\n" % (i, (b"n" if mate == 1 else b"mm") * (i % 9), mate, s, bytes(rng.integers(33, 74, len(s)).astype(np.uint8))))
        t1, t2 = open(paths[0], "rb").read(), open(paths[1], "rb").read()
        r1, r2 = whole_records(t1, True)[0], whole_records(t2, True)[0]
        a = (t1[:int(r1[h])], t2[:int(r2[h])])
        b = (t1[int(r1[h]):], t2[int(r2[h]):])
        chrs = list(ds.d.chr_table)
        ha, hb = HostRemain(tmp_path, *a, h, tag="A", chrs=chrs), HostRemain(tmp_path, *b, n - h, tag="B", chrs=chrs)
        hp.prof(True)
        hp.prof_reset()
        assert hp.stage_text(*a, h, **BITS)[0].n_pairs == h
        hp.swap()
        assert hp.stage_text(*b, n)[0].n_pairs == n - h           # without the bits: takes the staged set, never becomes resident
        assert hp.stage_text(*b, n, **BITS)[0].n_pairs == n - h
        hp.map_rounds(slots)
        for hx, m in ((ha, h), (hb, n - h)):
            rec = hp.collect_records().copy()
            sel = rec["pair"].astype(np.int64)
            assert 0 < len(sel) < m                               # mapping chose a proper subset
            st = hp.download()[0]
            assert np.array_equal(st[sel], rec["state"])
            want, _ = _whole(hp, hx, st, sel, chrs=chrs)
            assert b"mm/" not in want[1] and b"mm " in want[1] and b"mm " not in want[0]
            f1, f2, keys, n_rec, _ = hp.format_remain(chrs, first=1, count=len(sel) - 1, keys=True)      # a range of the set
            assert (f1, f2) == hx.files(st, sel[1:], chrs=chrs) and n_rec == len(sel)
            ds_st = remain_states(m, len(chrs))                   # the directed states over the active set mapping chose
            hp.poke_states(ds_st)
            _whole(hp, hx, ds_st, sel, chrs=chrs)
            if hx is ha:
                hp.swap()
                hp.map_rounds(slots)                              # takes B's first round over from the prefetch
        assert hp.prof_get()[1][7] == 1 and hp.prof_get()[0][7] > 0      # one prefetch; the formatter's kernels were timed
        hp.prof(False)
        ha.close()
        hb.close()
    finally:
        hp.close()


@pytest.fixture(scope="module")
def run_files(tmp_path_factory, built):
    from circminer_amd import synth
    from stage2_util import write_fastq_pair
    tmp = tmp_path_factory.mktemp("remain_run")
    n = 2400
    d = synth.generate("tiny2r", n_pairs=n, seed=45, mix=(0.5, 0.2, 0.3))
    fa = str(tmp / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    packed, info = cl.pack_genome(fa, 150_000)
    idx = cl.write_index(packed, kmer=20, n_threads=4)
    gtf = str(tmp / "ref.gtf")
    open(gtf, "w").write(d.gtf_text)
    fq1, fq2 = write_fastq_pair(tmp, d, n, name=lambda i: f"pair{i}" + "y" * (i % 5))
    return tmp, n, idx, gtf, fq1, fq2


def _run(run_files, out, remain, monkeypatch, world=1, fq=None, report=0):
    tmp, n, idx, gtf, fq1, fq2 = run_files
    if fq:
        fq1, fq2 = fq
    for var, val in (("CM_FASTQ_DEVICE", "1"), ("CM_FASTQ_DEVICE_BLOCK", "65536")):
        monkeypatch.setenv(var, val)
    for var, on in (("CM_REMAIN_DEVICE", remain), ("CM_PAM_DEVICE", report == 1)):
        if on:
            monkeypatch.setenv(var, "1")
        else:
            monkeypatch.delenv(var, raising=False)
    monkeypatch.delenv("CM_SAM_DEVICE", raising=False)
    out = str(tmp / out)
    sts = [cl.run_mapping(idx, gtf, fq1, fq2, out, cl.default_params(kmer=0), report=report, n_threads=4, batch_pairs=512, rank=r, world=world)
           for r in range(world)]
    cl.merge_parts(out, 2, world, report)
    files = tuple(open(f"{out}_2_remain_R{m}.fastq", "rb").read() for m in (1, 2)) + ((open(out + ".mapping.pam", "rb").read(),) if report == 1 else ())
    return (sum(s.pairs for s in sts), sum(s.bsj_pairs for s in sts), [sum(s.by_type[t] for s in sts) for t in range(14)],
            [s.device_parsed_batches for s in sts], files, out)


def test_files_to_files_with_device_records(run_files, monkeypatch):
    """cm_mapping_run, CM_FASTQ_DEVICE=1 with and without CM_REMAIN_DEVICE=1 and 64-KB blocks (several blocks per batch of 512
    pairs, five batches): both remain files and the counts, for one process and for two ranks on one card, and with report 1 and
    CM_PAM_DEVICE=1 beside it (bits 2 | 3 | 4 coexist); gzip input falls back to the host parser with the same files"""
    n = run_files[1]
    base = _run(run_files, "base", False, monkeypatch)
    dev = _run(run_files, "dev", True, monkeypatch)
    assert base[0] == dev[0] == n and base[1] == dev[1] > 50 and base[2] == dev[2]
    assert dev[3][0] >= 3 and base[3] == dev[3]
    assert dev[4] == base[4] and len(base[4][0]) > 10_000 and base[4][0].count(b"\n") == 4 * base[1]
    dev2 = _run(run_files, "dev2", True, monkeypatch, world=2)
    assert dev2[:3] == base[:3] and min(dev2[3]) >= 3 and dev2[4] == base[4]
    assert not [f for f in os.listdir(str(run_files[0])) if ".part" in f]
    pam0 = _run(run_files, "pam0", False, monkeypatch, report=1)
    pam1 = _run(run_files, "pam1", True, monkeypatch, report=1)
    assert pam1[:5] == pam0[:5] and pam1[4][:2] == base[4] and pam1[3][0] >= 3 and pam1[4][2].count(b"\n") == n
    gz = []
    for p in run_files[4:6]:
        gz.append(p + ".gz")
        with gzip.open(gz[-1], "wb", compresslevel=1) as f:
            f.write(open(p, "rb").read())
    dz = _run(run_files, "dz", True, monkeypatch, fq=gz)
    assert dz[3] == [0] and dz[0] == n and dz[4] == base[4]
