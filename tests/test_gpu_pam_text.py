"""cm_format_pam on the device: the PAM rows of the resident batch formatted by k_pam_len / k_pam_rows from the states in HBM and the
names cm_reads_stage_text keeps (flag bit 2), against the project's own host writer -- cm_fastq_next on files holding the same
bytes, then cm_write_pam with the same states -- byte for byte; cm_state_poke; cm_mapping_run with CM_PAM_DEVICE=1.

The row kernel takes 64 rows per wave and an 8-KB window: 65 and 4100 rows are more than one span, a run of 300 - 400-byte names
crosses the window, the ranges cut a span."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from circminer_amd import lib as cl
from fastq_text_util import HostParse, check_against_host, whole_records
from pam_text_util import CHRS, MAPPED_TYPES, HostRows, directed_states, pair_text

pytestmark = pytest.mark.gpu
CM_EINVAL, CM_ESTATE, CM_ELIMIT = -1, -5, -6


class Dev:
    """stage_text -> swap -> peek_reads, in the shape check_against_host compares"""

    def __init__(self, hp, t1: bytes, t2: bytes, max_pairs, keep_names):
        self.rc = 0
        self.tb, self.rec1, self.rec2 = hp.stage_text(t1, t2, max_pairs, keep_names=keep_names)
        self.n = int(self.tb.n_pairs)
        hp.swap()
        self.seq1, self.off1, self.seq2, self.off2 = hp.peek_reads()


def _rc(hp, **kw):
    """the error code of a format_pam that is refused"""
    with pytest.raises(RuntimeError) as e:
        hp.format_pam(CHRS, **kw)
    return int(str(e.value).split("(")[1].split(")")[0])


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
    """per n: the two texts (special names, a run of long names from 65 pairs on) and the host parser's view of them, made once"""
    tmp = tmp_path_factory.mktemp("pam_texts")
    out = {}

    def get(n):
        if n not in out:
            t1, t2 = pair_text(np.random.default_rng(n), n, (n // 2, min(n, n // 2 + 90)) if n >= 65 else None)
            out[n] = (t1, t2, HostParse(tmp, t1, t2, n, tag=f"p{n}"), HostRows(tmp, t1, t2, n, tag=f"r{n}"))
        return out[n]
    yield get
    for v in out.values():
        v[3].close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4100])
def test_staging_with_and_without_names(hp_plain, texts, n):
    """the staged arrays are the host parser's with and without bit 2; with it the rows of the fresh batch are cm_write_pam's on
    its first-round states (all unmapped rows), without it there is nothing to format"""
    hp = hp_plain
    t1, t2, hparse, hrows = texts(n)
    e = Dev(hp, t1, t2, n, keep_names=False)
    check_against_host(e, hparse, n, t1, t2)
    assert _rc(hp) == CM_ESTATE
    e = Dev(hp, t1, t2, n, keep_names=True)
    check_against_host(e, hparse, n, t1, t2)
    st = hp.download()[0]
    assert not np.isin(st["type"], MAPPED_TYPES).any()
    rows, stats = hp.format_pam(CHRS)
    assert rows == hrows.rows(st) and rows.count(b"\n") == n
    assert stats[:2] == [n, len(rows)] and stats[2] + stats[3] == (n + 63) // 64
    if n >= 65:
        assert stats[2] > 0 and stats[3] > 0


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [65, 4100])
def test_directed_states(hp_plain, hp_wide, texts, n, wide):
    """stage with names -> swap -> poke_states(directed_states) -> format_pam: whole batches and ranges that cut a span of 64 rows,
    in both kernel builds; both paths of the row kernel are taken"""
    hp = hp_wide if wide else hp_plain
    t1, t2, _, hrows = texts(n)
    assert hp.stage_text(t1, t2, n, keep_names=True)[0].n_pairs == n
    hp.swap()
    st = directed_states(n)
    hp.poke_states(st)
    assert hp.download()[0].tobytes() == st.tobytes()
    rows, stats = hp.format_pam(CHRS)
    assert rows == hrows.rows(st)
    assert stats[:2] == [n, len(rows)] and stats[2] > 0 and stats[3] > 0 and stats[2] + stats[3] == (n + 63) // 64
    for first, count in ((63, 2), (n // 3, 0), (n // 2 - 7, n - n // 2 + 7), (n - 1, 1)):
        rows, stats = hp.format_pam(CHRS, first=first, count=count)
        assert rows == hrows.rows(st, first, count), (first, count)
        assert stats[0] == count and stats[2] + stats[3] == (count + 63) // 64
    rows, _ = hp.format_pam([])                                   # another chromosome table (none): every chr_id prints "-"
    w = HostRows(hrows.dir, t1, t2, n, tag=f"nochr{n}{int(wide)}", chrs=[])
    assert rows == w.rows(st)
    w.close()
    assert hp.format_pam(CHRS)[0] == hrows.rows(st)               # ... and the first table again


def test_refusals_leave_the_batch_intact(built, texts):
    hp = cl.HotPath(cl.default_params())
    L = cl.load()
    try:
        n = 65
        t1, t2, hparse, hrows = texts(n)
        table = cl.chr_array(CHRS)
        assert _rc(hp) == CM_ESTATE                               # before any batch
        assert L.cm_state_poke(hp.h, directed_states(n).ctypes.data) == CM_ESTATE
        b = cl.ReadBatch(np.full((n, 40), ord("A"), np.uint8), np.full((n, 40), ord("C"), np.uint8))
        hp.upload(b)                                              # a batch from upload has no names
        fresh = hp.download()[0]
        assert _rc(hp) == CM_ESTATE and hp.download()[0].tobytes() == fresh.tobytes()
        assert hp.stage_text(t1, t2, n)[0].n_pairs == n           # staged without bit 2
        hp.swap()
        assert _rc(hp) == CM_ESTATE
        s1, o1, _, _ = hp.peek_reads()
        assert np.array_equal(o1, hparse.off1) and np.array_equal(s1, hparse.seq1)
        assert hp.stage_text(t1, t2, n, keep_names=True)[0].n_pairs == n
        hp.swap()
        st = directed_states(n)
        hp.poke_states(st)
        want = hrows.rows(st)
        for kw in (dict(first=n, count=1), dict(first=0, count=n + 1), dict(first=n + 1, count=0)):
            assert _rc(hp, **kw) == CM_EINVAL
        got = C.c_uint64(0)
        buf = np.full(len(want) + 8, 0xA5, np.uint8)
        assert L.cm_format_pam(hp.h, table, len(CHRS), 0, n, None, 5, C.byref(got), None) == CM_EINVAL
        assert L.cm_format_pam(hp.h, table, len(CHRS), 0, n, buf.ctypes.data, len(want) - 1, C.byref(got), None) == CM_ELIMIT
        assert got.value == len(want) and bool((buf == 0xA5).all())                 # the needed size, nothing written
        assert L.cm_format_pam(hp.h, table, len(CHRS), 0, n, buf.ctypes.data, len(want), C.byref(got), None) == 0
        assert got.value == len(want) and buf[:len(want)].tobytes() == want and bool((buf[len(want):] == 0xA5).all())
        assert hp.format_pam(CHRS)[0] == want and hp.download()[0].tobytes() == st.tobytes()
    finally:
        hp.close()


def test_names_follow_their_batch(ds_tiny2r, tmp_path):
    """stage A -> swap -> stage B -> map_rounds (B's first round is prefetched out of the tokeniser's buffers, B's text has
    overwritten A's): format_pam gives A's names with A's mapped states; after the swap B's"""
    from stage2_util import write_fastq_pair
    ds = ds_tiny2r
    hp = cl.HotPath(cl.default_params(kmer=ds.kmer))
    try:
        for ci in range(ds.hi.n_contigs):
            hp.load_contig(ci, ds.hi.views[ci], ds.hi.annots[ci])
        slots = list(range(ds.hi.n_contigs))
        n = ds.batch.n
        h = n // 2
        p1, p2 = write_fastq_pair(tmp_path, ds.d, n, name=lambda i: f"pair{i}" + "n" * (i % 9))
        t1, t2 = open(p1, "rb").read(), open(p2, "rb").read()
        r1, r2 = whole_records(t1, True)[0], whole_records(t2, True)[0]
        a = (t1[:int(r1[h])], t2[:int(r2[h])])
        b = (t1[int(r1[h]):], t2[int(r2[h]):])
        chrs = list(ds.d.chr_table)
        ha, hb = HostRows(tmp_path, *a, h, tag="A", chrs=chrs), HostRows(tmp_path, *b, n - h, tag="B", chrs=chrs)
        hp.prof(True)
        hp.prof_reset()
        assert hp.stage_text(*a, h, keep_names=True)[0].n_pairs == h
        hp.swap()
        assert hp.stage_text(*b, n, keep_names=True)[0].n_pairs == n - h
        hp.map_rounds(slots)
        rows, stats = hp.format_pam(chrs)
        st = hp.download()[0]
        assert rows == ha.rows(st) and np.isin(st["type"], MAPPED_TYPES).any() and hp.prof_get()[1][7] == 0
        hp.swap()
        hp.map_rounds(slots)                                      # takes B's first round over from the prefetch
        rows, _ = hp.format_pam(chrs)
        st = hp.download()[0]
        assert rows == hb.rows(st) and np.isin(st["type"], MAPPED_TYPES).any() and hp.prof_get()[1][7] == 1
        assert hp.prof_get()[0][7] > 0                            # the formatter's kernels were timed
        hp.prof(False)
        ha.close()
        hb.close()
    finally:
        hp.close()


@pytest.fixture(scope="module")
def run_files(tmp_path_factory, built):
    from circminer_amd import synth
    from stage2_util import write_fastq_pair
    tmp = tmp_path_factory.mktemp("pam_run")
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


def _run(run_files, out, device, monkeypatch, report=1, world=1, fq=None):
    tmp, n, idx, gtf, fq1, fq2 = run_files
    if fq:
        fq1, fq2 = fq
    for var, val in (("CM_FASTQ_DEVICE", "1"), ("CM_PAM_DEVICE", "1"), ("CM_FASTQ_DEVICE_BLOCK", "65536")):
        if device:
            monkeypatch.setenv(var, val)
        else:
            monkeypatch.delenv(var, raising=False)
    out = str(tmp / out)
    sts = [cl.run_mapping(idx, gtf, fq1, fq2, out, cl.default_params(kmer=0), report=report, n_threads=4, batch_pairs=512, rank=r, world=world)
           for r in range(world)]
    cl.merge_parts(out, 2, world, report)
    files = tuple(open(f"{out}_2_remain_R{m}.fastq", "rb").read() for m in (1, 2))
    files += (open(out + (".mapping.sam" if report == 2 else ".mapping.pam"), "rb").read(),)
    return (sum(s.pairs for s in sts), sum(s.bsj_pairs for s in sts), [sum(s.by_type[t] for s in sts) for t in range(14)],
            [s.device_parsed_batches for s in sts], files, out)


def test_files_to_files_with_device_rows(run_files, monkeypatch):
    """cm_mapping_run, report 1, CM_FASTQ_DEVICE=1 CM_PAM_DEVICE=1 and 64-KB blocks: .mapping.pam, the remain files and the counts
    of the host parser's run, for one process and for two ranks on one card"""
    n = run_files[1]
    host = _run(run_files, "host", False, monkeypatch)
    dev = _run(run_files, "dev", True, monkeypatch)
    assert host[0] == dev[0] == n and host[1] == dev[1] > 50 and host[2] == dev[2]
    assert dev[3][0] >= 3 and host[3] == [0]
    assert dev[4] == host[4] and host[4][2].count(b"\n") == n and len(host[4][0]) > 10_000
    dev2 = _run(run_files, "dev2", True, monkeypatch, world=2)
    assert dev2[:3] == host[:3] and min(dev2[3]) >= 3 and dev2[4] == host[4]
    assert not [f for f in os.listdir(str(run_files[0])) if ".part" in f]


def test_the_host_parser_keeps_what_it_must(run_files, monkeypatch):
    """with both variables set, report = 2 (SAM rows need bases and qualities), gzip input and carried 23-token headers stay on
    cm_fastq_next: no batch is parsed on the device, the files are those of the run without the variables"""
    n = run_files[1]
    host = _run(run_files, "h1", False, monkeypatch)
    hs = _run(run_files, "hs", False, monkeypatch, report=2)
    ds = _run(run_files, "dsam", True, monkeypatch, report=2)
    assert ds[3] == [0] and ds[:3] == hs[:3] and ds[4] == hs[4] and hs[4][2].startswith(b"@HD")
    gz = []
    for p in run_files[4:6]:
        gz.append(p + ".gz")
        with gzip.open(gz[-1], "wb", compresslevel=1) as f:
            f.write(open(p, "rb").read())
    dz = _run(run_files, "dz", True, monkeypatch, fq=gz)
    assert dz[3] == [0] and dz[0] == n and dz[4] == host[4]
    rem = (host[5] + "_2_remain_R1.fastq", host[5] + "_2_remain_R2.fastq")      # carried headers: the remain files are such input
    h2 = _run(run_files, "hc", False, monkeypatch, fq=rem)
    d2 = _run(run_files, "dc", True, monkeypatch, fq=rem)
    assert d2[3] == [0] and d2[:3] == h2[:3] and d2[4] == h2[4] and d2[0] == host[1]
