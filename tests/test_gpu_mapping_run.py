"""cm_mapping_run from files to files against the CPU oracle's bytes, one run per source of the contigs, per report and per feed.

The expectation never comes from the library: the oracle maps the pairs on its own index (op.map_all_rounds) and the Python
restatements of the writers (tests/test_fastq_io.py, through mapping_files_util) turn its final states into the mapping file and
the two remain files.  2 400 pairs of `tiny2r` in batches of 512 are five batches -- every one of the parser's four generations is
used again, the last batch is short -- and contigs of 150 000 are two packed contigs, so the contig loop's read-ahead thread runs
once with a contig to read and once into the end.  The last case cuts R2 short, so that the run fails with its threads in flight."""
import os
import re
import shutil

import numpy as np
import pytest

from circminer_amd import lib as cl
from oracle import oracle_py as op
from mapping_files_util import expected_mapping_rows, expected_remain_lines

pytestmark = pytest.mark.gpu
N, BATCH = 2400, 512
TEXT = {"CM_FASTQ_DEVICE": "1", "CM_FASTQ_DEVICE_BLOCK": "65536"}
# the parent's return code and message prefix for an R2 that ends after its 1 500th record, recorded by running this module's body
# against the parent's library: the host parser refuses batch 2 on the parser thread while batch 0 is on the device; the device
# tokeniser refuses the block that holds R2's end when the calling thread stages it, with a writer in flight
CUT = {"host": (-1, "cm_fastq_next failed (-1)"), "text": (-1, "cm_reads_stage_text failed (-1): FASTQ file 2 ends before file 1")}


class Files:
    pass


@pytest.fixture(scope="module")
def run_files(tmp_path_factory, built):
    from circminer_amd import synth
    from stage2_util import write_fastq_pair
    F = Files()
    tmp = F.tmp = tmp_path_factory.mktemp("mapping_run")
    d = synth.generate("tiny2r", n_pairs=N, seed=45, mix=(0.5, 0.2, 0.3))
    fa = str(tmp / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    F.packed, F.info = cl.pack_genome(fa, 150_000)
    F.full = cl.write_index(F.packed, kmer=20, n_threads=4)
    os.makedirs(str(tmp / "compact"))
    packed_c = shutil.copy(F.packed, str(tmp / "compact"))
    shutil.copy(F.info, str(tmp / "compact"))
    F.compact = cl.write_index(packed_c, kmer=20, compact=True, n_threads=4)
    F.gtf = str(tmp / "ref.gtf")
    open(F.gtf, "w").write(d.gtf_text)
    names = [f"pair{i}" + "y" * (i % 5) for i in range(N)]
    F.fq1, F.fq2 = write_fastq_pair(tmp, d, N, name=lambda i: names[i])
    F.cut2 = str(tmp / "cut_2.fq")
    with open(F.cut2, "w") as f:
        f.writelines(open(F.fq2).readlines()[:4 * 1500])
    # the expectation: the oracle on its own builders' index of the same genome
    hi = op.OracleIndex(d.contigs, d.chr_table, F.gtf, kmer=20)
    want, act, _ = op.map_all_rounds(cl.default_params(), hi, cl.ReadBatch(d.seq1, d.seq2))
    assert hi.n_contigs == 2
    keep = np.nonzero(act)[0]
    F.bsj, F.by_type, F.chrs = len(keep), [int((want["type"] == t).sum()) for t in range(14)], d.chr_table
    assert F.bsj > 50 and set(want["type"][keep]) <= {3, 4}
    seqs = [[a[i].tobytes().decode() for i in range(N)] for a in (d.seq1, d.seq2)]
    quals = [["I" * len(s) for s in mate] for mate in seqs]
    F.remain = tuple("".join(ln + "\n" for ln in expected_remain_lines(names, want, keep, F.chrs, seqs[m], quals[m])).encode() for m in (0, 1))
    F.pam = "".join(r + "\n" for r in expected_mapping_rows(1, names, want, F.chrs)).encode()
    F.sam = expected_mapping_rows(2, names, want, F.chrs, seqs[0], quals[0], seqs[1], quals[1])
    return F


def _run(F, monkeypatch, out, index, report, env=None, kmer=0, index_info=None, fq2=None):
    for var in ("CM_FASTQ_DEVICE", "CM_PAM_DEVICE", "CM_FASTQ_DEVICE_BLOCK"):
        monkeypatch.delenv(var, raising=False)
    for var, val in (env or {}).items():
        monkeypatch.setenv(var, val)
    out = str(F.tmp / out)
    st = cl.run_mapping(index, F.gtf, F.fq1, fq2 or F.fq2, out, cl.default_params(kmer=kmer), report=report, n_threads=4, batch_pairs=BATCH,
                        index_info=index_info)
    return st, out


def _check(F, st, out, report):
    assert (st.pairs, st.bsj_pairs, st.rounds) == (N, F.bsj, 2) and list(st.by_type) == F.by_type
    for m in (0, 1):
        assert open(f"{out}_2_remain_R{m + 1}.fastq", "rb").read() == F.remain[m], m
    if report == 1:
        assert open(out + ".mapping.pam", "rb").read() == F.pam
    elif report == 2:
        rows = open(out + ".mapping.sam").read().split("\n")
        hdr = 1 + len(F.chrs)
        assert rows[0].startswith("@HD") and [r.split("\t")[1] for r in rows[1:hdr]] == [f"SN:{c[0]}" for c in F.chrs]
        assert rows[-1] == "" and rows[hdr:-1] == F.sam
    else:
        assert not os.path.exists(out + ".mapping.pam") and not os.path.exists(out + ".mapping.sam")


@pytest.mark.parametrize("report", [0, 1, 2])
def test_full_index(run_files, monkeypatch, report):
    """the table crosses PCIe as it is in the file (cm_load_contig_raw); records + histogram, PAM rows, SAM rows"""
    st, out = _run(run_files, monkeypatch, f"full{report}", run_files.full, report)
    _check(run_files, st, out, report)
    assert st.device_parsed_batches == 0


def test_compact_index(run_files, monkeypatch):
    """the host decodes the table (cm_host_next_contig + cm_load_contig), the contig's host copy goes back after each upload"""
    st, out = _run(run_files, monkeypatch, "compact", run_files.compact, 1)
    _check(run_files, st, out, 1)


def test_packed_fasta(run_files, monkeypatch):
    """no index file: the device builds the tables (cm_build_contig), k comes from the parameters"""
    st, out = _run(run_files, monkeypatch, "fasta", run_files.packed, 1, kmer=20, index_info=run_files.info)
    _check(run_files, st, out, 1)


@pytest.mark.parametrize("report,env", [(0, TEXT), (1, dict(TEXT, CM_PAM_DEVICE="1"))], ids=["records", "pam_rows"])
def test_device_tokeniser(run_files, monkeypatch, report, env):
    """CM_FASTQ_DEVICE=1 with 64-KB blocks: the text registrations are widened block by block; with CM_PAM_DEVICE=1 the rows too
    are the device's"""
    st, out = _run(run_files, monkeypatch, f"text{report}", run_files.full, report, env=env)
    _check(run_files, st, out, report)
    assert st.device_parsed_batches >= 3


@pytest.mark.parametrize("feed", ["host", "text"])
def test_r2_ends_early_with_the_threads_in_flight(run_files, monkeypatch, feed):
    """R2 ends after its 1 500th record: a malformed input file.  The call returns the parent's code and message -- it does not hang
    or crash, whatever thread meets the end -- and the next run in the process writes the expected bytes"""
    env = TEXT if feed == "text" else None
    with pytest.raises(RuntimeError) as e:
        _run(run_files, monkeypatch, "cut_" + feed, run_files.full, 0, env=env, fq2=run_files.cut2)
    m = re.match(r"cm_mapping_run failed \((-?\d+)\): (.*)", str(e.value), re.S)
    print("cut R2,", feed, "feed:", str(e.value))
    assert m and (int(m.group(1)), m.group(2)[:len(CUT[feed][1])]) == CUT[feed], str(e.value)
    st, out = _run(run_files, monkeypatch, "after_cut_" + feed, run_files.full, 0, env=env)
    _check(run_files, st, out, 0)
    assert (st.device_parsed_batches >= 3) == (feed == "text")
