"""cm_detect_run on the device: both stages in one call against cm_mapping_run + cm_circ_run with every path variable unset, file by
file and byte for byte, on both hand-overs; cm_circ_call_resident against cm_circ_call; the chain workspace owned by the context.

The data set is the one of test_gpu_remain_sorted.run_files, made here again: tiny2r, 800 pairs, each three times -- 400 as triples
side by side, 400 three blocks apart -- so that sort keys tie inside a batch and across batches; two contigs, 512 pairs a batch."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

from circminer_amd import lib as cl, synth
from oracle import oracle_py as op
import circ_chain_util as u
from stage2_util import write_fastq_pair

pytestmark = pytest.mark.gpu
N_BASE = 800
PATH_VARS = ("CM_FASTQ_DEVICE", "CM_PAM_DEVICE", "CM_SAM_DEVICE", "CM_REMAIN_DEVICE", "CM_REMAIN_SORTED", "CM_CIRC_PRESORTED", "CM_CIRC_DEVICE")
KNOBS = ("CM_REMAIN_TIE_CAP", "CM_CIRC_LOG_CAP", "CM_CIRC_TABLE_BYTES", "CM_CIRC_THREADS", "CM_REMAIN_TRACE", "CM_CIRC_TRACE")
WIDE = dict(kmer=14, max_read_len=300)


def _reference_files(tmp, d):
    fa = str(tmp / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    packed, info = cl.pack_genome(fa, 150_000)
    idx = cl.write_index(packed, kmer=20, n_threads=4)
    gtf = str(tmp / "ref.gtf")
    open(gtf, "w").write(d.gtf_text)
    return packed, info, idx, gtf


class Data:
    def __init__(self, tmp):
        self.tmp = tmp
        self.d = d = synth.generate("tiny2r", n_pairs=N_BASE, seed=45, mix=(0.3, 0.1, 0.6))
        self.packed, self.info, self.idx, self.gtf = _reference_files(tmp, d)
        h = N_BASE // 2
        order = np.concatenate([np.repeat(np.arange(h), 3), np.tile(np.arange(h, N_BASE), 3)])

        class _Sub:
            seq1, seq2 = d.seq1[order], d.seq2[order]
        self.fq1, self.fq2 = write_fastq_pair(tmp, _Sub, len(order), name=lambda i: f"r{i:05d}")
        self.n = len(order)
        self._base = {}

    def out(self, tag):
        p = self.tmp / tag
        p.mkdir()
        return str(p / "o")

    def base(self, report, monkeypatch):
        """cm_mapping_run + cm_circ_run with every path variable unset -> (counts, files), once per report mode"""
        if report not in self._base:
            _clean_env(monkeypatch)
            out = self.out(f"base{report}")
            st = cl.run_mapping(self.idx, self.gtf, self.fq1, self.fq2, out, cl.default_params(kmer=0), report=report, n_threads=4, batch_pairs=512)
            assert st.device_parsed_batches == 0
            cl.run_circ(self.idx, self.gtf, out, 2, cl.default_params(kmer=0))
            self._base[report] = (_counts(st), _files(out, report), out)
        return self._base[report]


@pytest.fixture(scope="module")
def data(tmp_path_factory, built):
    return Data(tmp_path_factory.mktemp("detect"))


def _clean_env(monkeypatch):
    for var in PATH_VARS + KNOBS:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("CM_FASTQ_DEVICE_BLOCK", "65536")


def _counts(st):
    return st.pairs, st.bsj_pairs, list(st.by_type), st.rounds


def _files(out, report, rounds=2):
    names = [f"{out}_{rounds}_remain_R1.fastq", f"{out}_{rounds}_remain_R2.fastq", out + ".candidates.pam", out + ".circ_report"]
    if report:
        names.append(out + (".mapping.sam" if report == 2 else ".mapping.pam"))
    return {os.path.basename(p): open(p, "rb").read() for p in names}


def _srt(out, rounds=2):
    return tuple(open(p, "rb").read() if os.path.exists(p) else None for p in (f"{out}_{rounds}_remain_R{m}.fastq.srt" for m in (1, 2)))


def _detect(data, tag, report=0, fq=None, **kw):
    out = data.out(tag)
    fq1, fq2 = fq or (data.fq1, data.fq2)
    st = cl.run_detect(kw.pop("index", data.idx), data.gtf, fq1, fq2, out, kw.pop("params", cl.default_params(kmer=0)), report=report, n_threads=4, batch_pairs=512,
                       **kw)
    return st, out


@pytest.mark.parametrize("report", [0, 1, 2])
def test_memory_hand_over(data, monkeypatch, report):
    counts, want, base_out = data.base(report, monkeypatch)
    assert counts[0] == data.n and counts[1] > 50
    # the path variables are not read: set against the rule, they change nothing
    for var in PATH_VARS:
        monkeypatch.setenv(var, "0")
    st, out = _detect(data, f"mem{report}", report)
    for var in PATH_VARS:
        monkeypatch.delenv(var)
    got = _files(out, report)
    for name in want:
        assert got[name] == want[name], name
    rows = want["o.candidates.pam"].decode().strip().split("\n")
    assert {r.split("\t")[1] for r in rows} == {"chr1", "chr2"} and want["o.circ_report"]
    print("detect stats: problems", st.problems, "refused", st.refused, "recomputed", st.recomputed, "batches", st.map.device_parsed_batches,
          "hand-over s", st.seconds_handover, "total s", st.seconds_total)
    assert st.handover_used == 0 and _counts(st.map) == counts and st.map.device_parsed_batches >= 3
    assert st.problems > 1000 and st.refused == 0 and st.recomputed == 0
    assert (st.circ.pairs, st.circ.candidate_rows) == (counts[1], len(rows)) and st.circ.calls > 0
    assert _srt(out) == (None, None) and sorted(os.listdir(os.path.dirname(out))) == sorted(want)      # nothing else is left
    # flags bit 0: the two .srt files too, the bytes cm_sort_remain makes of the remain files
    st2, out2 = _detect(data, f"mem{report}srt", report, srt_files=True)
    want_srt = tuple(open(cl.sort_remain(f"{base_out}_2_remain_R{m}.fastq", str(data.tmp / f"want{report}_R{m}.srt")), "rb").read() for m in (1, 2))
    assert _srt(out2) == want_srt and len(want_srt[0]) > 0
    assert _files(out2, report) == want and st2.handover_used == 0 and st2.problems == st.problems


def test_files_hand_over(data, monkeypatch):
    counts, want, base_out = data.base(0, monkeypatch)
    st, out = _detect(data, "files", handover=1)
    assert _files(out, 0) == want and st.handover_used == 1 and _counts(st.map) == counts and st.map.device_parsed_batches == 0
    assert st.problems > 1000 and st.refused == 0 and st.recomputed == 0
    assert _srt(out) == _srt(base_out) and _srt(out)[0]                          # as cm_circ_run leaves them
    gz = []
    for p in (data.fq1, data.fq2):
        gz.append(p + ".gz")
        with open(p, "rb") as src, gzip.open(gz[-1], "wb", compresslevel=1) as dst:
            dst.write(src.read())
    st, out = _detect(data, "gzip", fq=gz, handover=0)
    assert _files(out, 0) == want and st.handover_used == 1 and _counts(st.map) == counts and st.problems > 1000


def test_tie_cap_orders_batches_on_the_host(data, monkeypatch, capfd):
    counts, want, _ = data.base(0, monkeypatch)
    monkeypatch.setenv("CM_REMAIN_TIE_CAP", "2")
    monkeypatch.setenv("CM_REMAIN_TRACE", "1")
    capfd.readouterr()
    st, out = _detect(data, "cap2")
    trace = [ln for ln in capfd.readouterr().err.split("\n") if ln.startswith("[remain] sorted runs:")]
    assert len(trace) == 1 and int(trace[0].split(" batches, ")[1].split(" ")[0]) >= 1, trace
    assert f"{st.map.device_parsed_batches} batches" in trace[0] and f"{counts[1]} records" in trace[0]
    assert _files(out, 0) == want and st.handover_used == 0 and _counts(st.map) == counts


def test_log_cap_refuses_and_recomputes(data, monkeypatch, capfd):
    counts, want, _ = data.base(0, monkeypatch)
    monkeypatch.setenv("CM_CIRC_LOG_CAP", "20")
    monkeypatch.setenv("CM_CIRC_TRACE", "1")
    capfd.readouterr()
    st, out = _detect(data, "log20")
    err = capfd.readouterr().err
    print("refused", st.refused, "of", st.problems, "recomputed", st.recomputed)
    assert 0 < st.refused < st.problems and st.recomputed > 0
    assert _files(out, 0) == want
    assert "chains ahead (device, resident contigs)" in err and re.search(r"workspace: \d+ allocations, \d+ held", err)


def test_no_candidate(data, monkeypatch):
    """pairs cut out of the genome as they stand (concordant, no error): no pair reaches stage 2, both of its files are empty"""
    _clean_env(monkeypatch)
    d = data.d
    name, con, start, ln = d.chr_table[0]
    chrom = d.contigs[con - 1][start:start + ln]
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGTN")] = list(b"TGCAN")
    rng = np.random.default_rng(2)
    at = rng.integers(1000, ln - 1000, 300)

    class _Sub:
        seq1 = np.stack([chrom[p:p + 150] for p in at])
        seq2 = np.stack([comp[chrom[p + 200:p + 350]][::-1] for p in at])
    # pairs are mapped one by one: the few of these the two-call flow itself re-queues (a pair over a repeat or an exon border) are
    # found with it and left out, and the flow is run again on the rest
    fq = write_fastq_pair(data.tmp, _Sub, 300, prefix="plainpairs_all")
    out = data.out("none_first")
    cl.run_mapping(data.idx, data.gtf, fq[0], fq[1], out, cl.default_params(kmer=0), report=0, n_threads=4, batch_pairs=512)
    requeued = {int(ln.split(b" ")[0].split(b"/")[0][5:]) for ln in open(out + "_2_remain_R1.fastq", "rb").read().split(b"\n")[0::4] if ln}
    keep = np.array([i for i in range(300) if i not in requeued])
    assert len(keep) >= 250

    class _Kept:
        seq1, seq2 = _Sub.seq1[keep], _Sub.seq2[keep]
    fq = write_fastq_pair(data.tmp, _Kept, len(keep), prefix="plainpairs")
    out = data.out("none_base")
    st0 = cl.run_mapping(data.idx, data.gtf, fq[0], fq[1], out, cl.default_params(kmer=0), report=0, n_threads=4, batch_pairs=512)
    cl.run_circ(data.idx, data.gtf, out, 2, cl.default_params(kmer=0))
    want = _files(out, 0)
    assert st0.bsj_pairs == 0 and want["o.candidates.pam"] == b"" and want["o.circ_report"] == b"" and want["o_2_remain_R1.fastq"] == b""
    st, out = _detect(data, "none", fq=fq)
    assert _files(out, 0) == want and st.handover_used == 0 and _counts(st.map) == _counts(st0) and st.problems == 0 and st.circ.pairs == 0
    st, out = _detect(data, "none_files", fq=fq, handover=1)
    assert _files(out, 0) == want and st.handover_used == 1


def test_packed_fasta_source(data, monkeypatch):
    """no index file: the tables are built on the device, the host sequence is kept from the packed FASTA's records"""
    counts, want, _ = data.base(0, monkeypatch)
    st, out = _detect(data, "fasta", index=data.packed, params=cl.default_params(kmer=20), index_info=data.info)
    assert _files(out, 0) == want and st.handover_used == 0 and _counts(st.map) == counts and st.problems > 1000 and st.refused == 0


def test_compact_index_source(data, monkeypatch):
    """the third contig source: a compact index, decoded on the host; its sequence stays, its tables go back"""
    counts, want, _ = data.base(0, monkeypatch)
    compact = str(data.tmp / "compact.packed.fa")
    open(compact, "wb").write(open(data.packed, "rb").read())
    idx = cl.load().cm_host_write_index(compact.encode(), (compact + ".index").encode(), 20, 1, 4)
    assert idx == 0
    st, out = _detect(data, "compact", index=compact + ".index", index_info=data.info)
    assert _files(out, 0) == want and st.handover_used == 0 and _counts(st.map) == counts and st.problems > 1000


def test_call_resident_directly(built, monkeypatch, tmp_path):
    _clean_env(monkeypatch)
    s = u.remain_set("tiny2r")
    hp = cl.HotPath(s.P)
    lacking = cl.HotPath(s.P)
    try:
        for c in range(s.hi.n_contigs):
            hp.load_contig(c, s.hi.views[c], s.hi.annots[c])
        cl.circ_call(s.P, s.hi, s.d.chr_table, s.b, str(tmp_path / "host.c"), str(tmp_path / "host.r"))
        want = open(tmp_path / "host.c", "rb").read(), open(tmp_path / "host.r", "rb").read()
        assert want[0].count(b"\n") > 100 and want[1]
        for threads in ("1", "13"):
            monkeypatch.setenv("CM_CIRC_THREADS", threads)
            rc, st = cl.circ_call_resident(hp, s.P, s.hi, s.d.chr_table, s.b, str(tmp_path / "res.c"), str(tmp_path / "res.r"))
            assert rc == 0 and (open(tmp_path / "res.c", "rb").read(), open(tmp_path / "res.r", "rb").read()) == want, threads
            assert st.candidate_rows == want[0].count(b"\n")
        # slot 1 holds its contig and no annotation: CM_ESTATE, nothing written
        lacking.load_contig(0, s.hi.views[0], s.hi.annots[0])
        lacking.load_contig(1, s.hi.views[1])
        rc, _ = cl.circ_call_resident(lacking, s.P, s.hi, s.d.chr_table, s.b, str(tmp_path / "no.c"), str(tmp_path / "no.r"))
        assert rc == -5 and not os.path.exists(tmp_path / "no.c") and not os.path.exists(tmp_path / "no.r")
        # ... and slot 1 with its annotation and no contig: the same code, by the other way
        bare = cl.HotPath(s.P)
        try:
            bare.load_contig(0, s.hi.views[0], s.hi.annots[0])
            bare.load_annotation(1, s.hi.annots[1])
            rc, _ = cl.circ_call_resident(bare, s.P, s.hi, s.d.chr_table, s.b, str(tmp_path / "no.c"), str(tmp_path / "no.r"))
            assert rc == -5 and not os.path.exists(tmp_path / "no.c")
        finally:
            bare.close()
        # ... and an annotation without its contig
        lacking.load_annotation(2, s.hi.annots[0])
        assert cl.load().cm_circ_chain_batch(lacking.h, 2, 0, None, 0, None, 0, None, 0, None, None, None, None, 0, None, None, 0, None, None, None) == -1
        # the context is intact: a freshly staged batch maps as the oracle says
        batch = cl.ReadBatch(s.d.seq1[:600], s.d.seq2[:600])
        want_st, _, _ = op.map_all_rounds(s.P, s.ohi, batch)
        hp.stage(batch)
        hp.swap()
        hp.map_rounds(list(range(s.hi.n_contigs)))
        assert hp.download()[0].tobytes() == want_st.tobytes()
    finally:
        hp.close()
        lacking.close()


@pytest.mark.parametrize("wide", [False, True])
def test_workspace_is_the_contexts(built, monkeypatch, capfd, wide):
    """one context, four calls: all requests, a prefix of 50, all again, all under CM_CIRC_LOG_CAP=20 -- allocations on the first,
    none on the second and third, a re-size on the fourth; every answer is the serial statement's"""
    _clean_env(monkeypatch)
    s = u.remain_set("variety")
    con = int(np.argmax([len(p[0]) for p in s.problems]))
    req, _, seqs = s.problems[con]
    want = s.host(con)
    assert len(req) > 200
    monkeypatch.setenv("CM_CIRC_TRACE", "1")
    hp = cl.HotPath(cl.default_params(**dict(u.SETS["variety"][3], **(WIDE if wide else {}))))
    try:
        if wide:
            hp.load_annotation(0, s.hi.annots[con])
            genome = s.hi.contigs[con]
        else:
            hp.load_contig(0, s.hi.views[con], s.hi.annots[con])
            genome = None                                                        # the contig resident in the slot

        def call(r):
            capfd.readouterr()
            got = hp.circ_chain_batch(0, genome, seqs, r)
            m = re.findall(r"workspace: (\d+) allocations, (\d+) held", capfd.readouterr().err)
            assert len(m) == 1, m
            return got, int(m[0][0]), int(m[0][1])
        first, a1, h1 = call(req)
        assert first.bytes() == want.bytes() and first.stats[5] == 0 and a1 >= 15 and h1 > 0
        part, a2, h2 = call(req[:50])
        assert [part.chains(i) for i in range(50)] == [want.chains(i) for i in range(50)] and (a2, h2) == (0, h1)
        again, a3, h3 = call(req)
        assert again.bytes() == want.bytes() and (a3, h3) == (0, h1)
        monkeypatch.setenv("CM_CIRC_LOG_CAP", "20")
        capped, a4, h4 = call(req)
        refused = capped.res["flags"] & 1
        print("wide", wide, "allocations", (a1, a2, a3, a4), "held", (h1, h4), "refused", int(refused.sum()), "of", len(req))
        assert 0 < a4 <= 4 and h4 < h1 and 0 < refused.sum() < len(req)
        for i in np.nonzero(refused == 0)[0]:
            assert capped.chains(i) == want.chains(i) and capped.res[i]["n_chains"] == want.res[i]["n_chains"]
        monkeypatch.delenv("CM_CIRC_LOG_CAP")
        back, a5, h5 = call(req)
        assert back.bytes() == want.bytes() and 0 < a5 <= 4 and h5 == h1
    finally:
        hp.close()


def test_example_program(data, monkeypatch, tmp_path):
    """examples/cm_detect.cpp, compiled against the header and the library: the same files from a process without Python"""
    import subprocess
    counts, want, _ = data.base(1, monkeypatch)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cm_detect")
    lib_dir = os.path.join(root, "circminer_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "cm_detect.cpp"), "-L", lib_dir, "-lcmhot",
                           f"-Wl,-rpath,{lib_dir}", "-o", exe])
    out = data.out("example")
    r = subprocess.run([exe, data.idx, data.gtf, data.fq1, data.fq2, out, "pam"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "hand-over through memory" in r.stdout and f"{counts[0]} pairs" in r.stdout, r.stdout
    assert _files(out, 1) == want
