"""cm_format_sam on the device: the SAM records of the resident batch formatted by k_sam_len / k_sam_rows from the states in HBM, the
names (flag bit 2) and qualities (flag bit 3) cm_reads_stage_text keeps and the bases in the read buffers, against the project's own
host writer -- cm_fastq_next on files holding the same bytes, then cm_write_sam with the same states -- byte for byte;
cm_quals_peek; cm_mapping_run with CM_SAM_DEVICE=1.

The row kernel takes 16 records (8 pairs) per wave and an 8-KB window: 65 and 323 pairs are many spans (323: about 40), a run of
300 - 400-byte names and the 250 - 300-bp reads of the 24-seed build cross the window, the ranges cut a span.  The texts hold the
reads that decide the rules (sam_text_util): every short length, bytes without a complement -- a NUL among them, which
check_against_host shows both parsers stage alike -- on reversed and unreversed records.

The runs of cm_mapping_run share the process, as test_gpu_pam_text.py's do: the variables are read by every call."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from circminer_amd import lib as cl
from fastq_text_util import HostParse, check_against_host, whole_records
from pam_text_util import CHRS, HostRows
from sam_text_util import SPAN_PAIRS, SPAN_RECS, HostSam, sam_mapped, sam_pair_text, sam_states

pytestmark = pytest.mark.gpu
CM_EINVAL, CM_ESTATE, CM_ELIMIT = -1, -5, -6
N_MANY = 40 * SPAN_PAIRS + 3


class Dev:
    """stage_text -> swap -> peek_reads, in the shape check_against_host compares"""

    def __init__(self, hp, t1: bytes, t2: bytes, max_pairs, keep_names, keep_quals):
        self.rc = 0
        self.tb, self.rec1, self.rec2 = hp.stage_text(t1, t2, max_pairs, keep_names=keep_names, keep_quals=keep_quals)
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
    """per (n, longest read): the directed states, the two texts (special names and reads, a run of long names from 65 pairs on) and
    the host parser's view of them, made once"""
    tmp = tmp_path_factory.mktemp("sam_texts")
    out = {}

    def get(n, hi=150):
        if (n, hi) not in out:
            st = sam_states(n)
            t1, t2, _ = sam_pair_text(np.random.default_rng(n + hi), n, st, (n // 2, min(n, n // 2 + 40)) if n >= 65 else None, hi)
            out[n, hi] = (t1, t2, HostParse(tmp, t1, t2, n, tag=f"p{n}_{hi}"), HostSam(tmp, t1, t2, n, tag=f"r{n}_{hi}"), st)
        return out[n, hi]
    yield get
    for v in out.values():
        v[3].close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, N_MANY])
def test_staging_with_and_without_the_bits(hp_plain, texts, n):
    """the staged arrays are the host parser's for every combination of bits 2 and 3; the kept qualities are the host parser's;
    format_sam needs both bits and says which is missing, format_pam needs the names only; the records of the fresh batch are
    cm_write_sam's on its first-round states"""
    hp = hp_plain
    t1, t2, hparse, hsam, _ = texts(n)
    _, _, _, _, q1, q2 = hsam.arrays()
    for names, quals in ((False, False), (True, False), (False, True), (True, True)):
        e = Dev(hp, t1, t2, n, names, quals)
        check_against_host(e, hparse, n, t1, t2)
        if quals:
            d1, d2 = hp.peek_quals()
            assert np.array_equal(d1, q1) and np.array_equal(d2, q2)
        else:
            assert _rc(hp.peek_quals)[0] == CM_ESTATE
        if names:
            assert hp.format_pam(CHRS)[0].count(b"\n") == n          # names alone are enough for PAM rows
        if not (names and quals):
            rc, msg = _rc(hp.format_sam, CHRS)
            assert rc == CM_ESTATE and ("no names" in msg) == (not names) and ("no qualities" in msg) == (not quals)      # names which
    st = hp.download()[0]
    rows, stats = hp.format_sam(CHRS)
    assert rows == hsam.rows(st) and rows.count(b"\n") == 2 * n
    assert stats[:2] == [2 * n, len(rows)] and stats[2] + stats[3] == (2 * n + SPAN_RECS - 1) // SPAN_RECS
    if n >= 65:
        assert stats[2] > 0 and stats[3] > 0


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [65, N_MANY])
def test_directed_states(hp_plain, hp_wide, texts, n, wide):
    """stage with names and qualities -> swap -> poke_states(sam_states) -> format_sam: whole batches and ranges that cut a span of
    8 pairs, in both kernel builds (reads of up to 300 bp in the 24-seed one); both paths of the row kernel are taken"""
    hp = hp_wide if wide else hp_plain
    t1, t2, hparse, hsam, st = texts(n, 300 if wide else 150)
    e = Dev(hp, t1, t2, n, True, True)
    check_against_host(e, hparse, n, t1, t2)
    hp.poke_states(st)
    assert hp.download()[0].tobytes() == st.tobytes()
    rows, stats = hp.format_sam(CHRS)
    want = hsam.rows(st)
    assert rows == want
    assert stats[:2] == [2 * n, len(rows)] and stats[2] > 0 and stats[3] > 0 and stats[2] + stats[3] == (2 * n + SPAN_RECS - 1) // SPAN_RECS
    m = sam_mapped(st["type"])
    assert (m & (st["r1_forward"] == 0)).any() and (m & (st["r2_forward"] == 0)).any()
    for first, count in ((SPAN_PAIRS - 1, 2), (n // 3, 0), (n // 2 - 7, n - n // 2 + 7), (n - 1, 1)):
        rows, stats = hp.format_sam(CHRS, first=first, count=count)
        assert rows == hsam.rows(st, first, count), (first, count)
        assert stats[0] == 2 * count and stats[2] + stats[3] == (2 * count + SPAN_RECS - 1) // SPAN_RECS
    rows, _ = hp.format_sam([])                                   # another chromosome table (none): every mapped RNAME is "-"
    assert rows == hsam.rows(st, chrs=[])
    assert hp.format_sam(CHRS)[0] == want                         # ... and the first table again


@pytest.mark.parametrize("wide", [False, True])
def test_the_two_formatters_alternate_on_one_context(hp_plain, hp_wide, texts, wide):
    """cm_format_pam and cm_format_sam share the driver, the device buffers and the cached chromosome table: PAM, SAM with another
    table (none), PAM, a SAM range that cuts a span, on one context; 65 pairs are one full PAM span + 1 row and eight full SAM
    spans + 2 records"""
    hp = hp_wide if wide else hp_plain
    n = 65
    t1, t2, _, hsam, st = texts(n)
    hpam = HostRows(hsam.dir, t1, t2, n, tag=f"alt{int(wide)}")
    try:
        assert Dev(hp, t1, t2, n, True, True).n == n
        hp.poke_states(st)
        pam = hpam.rows(st)
        assert hp.format_pam(CHRS)[0] == pam
        assert hp.format_sam(())[0] == hsam.rows(st, chrs=[])
        assert hp.format_pam(CHRS)[0] == pam
        assert hp.format_sam(CHRS, first=3, count=9)[0] == hsam.rows(st, 3, 9)
    finally:
        hpam.close()


def test_refusals_leave_the_batch_intact(built, texts):
    hp = cl.HotPath(cl.default_params())
    L = cl.load()
    try:
        n = 65
        t1, t2, hparse, hsam, st = texts(n)
        table = cl.chr_array(CHRS)
        assert _rc(hp.format_sam, CHRS)[0] == CM_ESTATE           # before any batch
        assert L.cm_quals_peek(hp.h, None, 0, None, 0) == CM_ESTATE
        b = cl.ReadBatch(np.full((n, 40), ord("A"), np.uint8), np.full((n, 40), ord("C"), np.uint8))
        hp.upload(b)                                              # a batch from upload has neither names nor qualities
        fresh = hp.download()[0]
        assert _rc(hp.format_sam, CHRS)[0] == CM_ESTATE and hp.download()[0].tobytes() == fresh.tobytes()
        assert hp.stage_text(t1, t2, n, keep_names=True, keep_quals=True)[0].n_pairs == n
        hp.swap()
        hp.poke_states(st)
        want = hsam.rows(st)
        for kw in (dict(first=n, count=1), dict(first=0, count=n + 1), dict(first=n + 1, count=0)):
            assert _rc(hp.format_sam, CHRS, **kw)[0] == CM_EINVAL
        got = C.c_uint64(0)
        buf = np.full(len(want) + 8, 0xA5, np.uint8)
        assert L.cm_format_sam(hp.h, table, len(CHRS), 0, n, None, 5, C.byref(got), None) == CM_EINVAL
        assert L.cm_format_sam(hp.h, table, len(CHRS), 0, n, buf.ctypes.data, len(want) - 1, C.byref(got), None) == CM_ELIMIT
        assert got.value == len(want) and bool((buf == 0xA5).all())                 # the needed size, nothing written
        assert L.cm_format_sam(hp.h, table, len(CHRS), 0, 0, buf.ctypes.data, 0, C.byref(got), None) == 0 and got.value == 0
        assert L.cm_format_sam(hp.h, table, len(CHRS), 0, n, buf.ctypes.data, len(want), C.byref(got), None) == 0
        assert got.value == len(want) and buf[:len(want)].tobytes() == want and bool((buf[len(want):] == 0xA5).all())
        assert hp.format_sam(CHRS)[0] == want and hp.download()[0].tobytes() == st.tobytes()
        s1, o1, _, _ = hp.peek_reads()
        assert np.array_equal(o1, hparse.off1) and np.array_equal(s1, hparse.seq1)
    finally:
        hp.close()


def test_names_and_qualities_follow_their_batch(ds_tiny2r, tmp_path):
    """stage A -> swap -> a stage without the bits (dropped) -> stage B -> map_rounds (B's first round is prefetched out of the
    tokeniser's buffers, B's text has overwritten A's): format_sam gives A's names, bases and qualities with A's mapped states;
    after the swap B's"""
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
        for mate, arr in ((1, ds.d.seq1), (2, ds.d.seq2)):        # (qualities that differ from record to record)
            paths.append(str(tmp_path / f"in_{mate}.fq"))
            with open(paths[-1], "wb") as f:
                for i in range(n):
                    s = arr[i].tobytes()
                    f.write(b"@pair%d%s/%d\n%s\n+\n%s\n" % (i, b"n" * (i % 9), mate, s, bytes(rng.integers(33, 74, len(s)).astype(np.uint8))))
        t1, t2 = open(paths[0], "rb").read(), open(paths[1], "rb").read()
        r1, r2 = whole_records(t1, True)[0], whole_records(t2, True)[0]
        a = (t1[:int(r1[h])], t2[:int(r2[h])])
        b = (t1[int(r1[h]):], t2[int(r2[h]):])
        chrs = list(ds.d.chr_table)
        ha, hb = HostSam(tmp_path, *a, h, tag="A", chrs=chrs), HostSam(tmp_path, *b, n - h, tag="B", chrs=chrs)
        hp.prof(True)
        hp.prof_reset()
        assert hp.stage_text(*a, h, keep_names=True, keep_quals=True)[0].n_pairs == h
        hp.swap()
        assert hp.stage_text(*b, n)[0].n_pairs == n - h           # without the bits: takes the staged set, never becomes resident
        assert hp.stage_text(*b, n, keep_names=True, keep_quals=True)[0].n_pairs == n - h
        hp.map_rounds(slots)
        rows, stats = hp.format_sam(chrs)
        st = hp.download()[0]
        assert rows == ha.rows(st) and (sam_mapped(st["type"]) & (st["r1_forward"] != st["r2_forward"])).any()
        hp.swap()
        hp.map_rounds(slots)                                      # takes B's first round over from the prefetch
        rows, _ = hp.format_sam(chrs)
        st = hp.download()[0]
        assert rows == hb.rows(st) and sam_mapped(st["type"]).any() and hp.prof_get()[1][7] == 1
        assert hp.prof_get()[0][7] > 0                            # the formatter's kernels were timed
        hp.prof(False)
        ha.close()
        hb.close()
    finally:
        hp.close()


def test_a_stage_without_the_bits_keeps_nothing(built, texts):
    """Launch neutrality.  The launch counters of cm_prof_get (test_gpu_launch_counts.py) count the mapping kernels, not the
    staging stream's, so this asserts the state instead: on a fresh context a stage without bits 2 / 3 leaves a batch for which
    neither names nor qualities exist (both readers refuse with CM_ESTATE, no error on the way), and bit 2 alone leaves no
    qualities; the staged arrays are the host parser's either way (test_staging_with_and_without_the_bits)."""
    hp = cl.HotPath(cl.default_params())
    try:
        n = 65
        t1, t2, hparse, _, _ = texts(n)
        e = Dev(hp, t1, t2, n, False, False)
        check_against_host(e, hparse, n, t1, t2)
        assert _rc(hp.peek_quals)[0] == CM_ESTATE and _rc(hp.format_pam, CHRS)[0] == CM_ESTATE and _rc(hp.format_sam, CHRS)[0] == CM_ESTATE
        e = Dev(hp, t1, t2, n, True, False)
        assert _rc(hp.peek_quals)[0] == CM_ESTATE and hp.format_pam(CHRS)[0].count(b"\n") == n
    finally:
        hp.close()


@pytest.fixture(scope="module")
def run_files(tmp_path_factory, built):
    from circminer_amd import synth
    from stage2_util import write_fastq_pair
    tmp = tmp_path_factory.mktemp("sam_run")
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


def _run(run_files, out, device, monkeypatch, world=1, fq=None):
    tmp, n, idx, gtf, fq1, fq2 = run_files
    if fq:
        fq1, fq2 = fq
    for var, val in (("CM_FASTQ_DEVICE", "1"), ("CM_SAM_DEVICE", "1"), ("CM_FASTQ_DEVICE_BLOCK", "65536")):
        if device:
            monkeypatch.setenv(var, val)
        else:
            monkeypatch.delenv(var, raising=False)
    out = str(tmp / out)
    sts = [cl.run_mapping(idx, gtf, fq1, fq2, out, cl.default_params(kmer=0), report=2, n_threads=4, batch_pairs=512, rank=r, world=world)
           for r in range(world)]
    cl.merge_parts(out, 2, world, 2)
    files = tuple(open(f"{out}_2_remain_R{m}.fastq", "rb").read() for m in (1, 2)) + (open(out + ".mapping.sam", "rb").read(),)
    return (sum(s.pairs for s in sts), sum(s.bsj_pairs for s in sts), [sum(s.by_type[t] for s in sts) for t in range(14)],
            [s.device_parsed_batches for s in sts], files, out)


def test_files_to_files_with_device_records(run_files, monkeypatch):
    """cm_mapping_run, report 2, CM_FASTQ_DEVICE=1 CM_SAM_DEVICE=1 and 64-KB blocks (several blocks per batch of 512 pairs, five
    batches): .mapping.sam, the remain files and the counts of the run without the variables, for one process and for two ranks on
    one card; gzip input falls back to the host parser with the same files"""
    n = run_files[1]
    host = _run(run_files, "host", False, monkeypatch)
    dev = _run(run_files, "dev", True, monkeypatch)
    assert host[0] == dev[0] == n and host[1] == dev[1] > 50 and host[2] == dev[2]
    assert dev[3][0] >= 3 and host[3] == [0]
    sam = host[4][2]
    assert dev[4] == host[4] and sam.startswith(b"@HD") and len(host[4][0]) > 10_000
    assert sum(1 for x in sam.split(b"\n") if x and not x.startswith(b"@")) == 2 * n
    dev2 = _run(run_files, "dev2", True, monkeypatch, world=2)
    assert dev2[:3] == host[:3] and min(dev2[3]) >= 3 and dev2[4] == host[4]
    assert not [f for f in os.listdir(str(run_files[0])) if ".part" in f]
    gz = []
    for p in run_files[4:6]:
        gz.append(p + ".gz")
        with gzip.open(gz[-1], "wb", compresslevel=1) as f:
            f.write(open(p, "rb").read())
    dz = _run(run_files, "dz", True, monkeypatch, fq=gz)
    assert dz[3] == [0] and dz[0] == n and dz[4] == host[4]
