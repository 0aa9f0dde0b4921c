"""cm_circ_chain_batch (circminer_amd/csrc/cm_circ_chain.hip) against cm_circ_chain_host, the serial statement, over the whole
result arrays; cm_circ_call_device / cm_circ_run with CM_CIRC_DEVICE=1 against cm_circ_call and the oracle, byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from circminer_amd import lib as cl
import circ_chain_util as u
from stage2_util import gnu_sort, oracle_stage2

pytestmark = pytest.mark.gpu

WIDE = dict(kmer=14, max_read_len=300)          # the context of the 24-seed kernel build (cm_dispatch.cpp)


@pytest.fixture(scope="module")
def hot(built):
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = cl.HotPath(cl.default_params(**kw))
        return made[key]

    yield get
    for hp in made.values():
        hp.close()


def _load_annot(hp, slot, av):
    hp._chk(hp.L.cm_load_annotation(hp.h, slot, C.byref(av)), "cm_load_annotation")


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", ["tiny", "tiny2r", "variety", "long300"])
def test_batch_equals_the_serial_statement(hot, name, wide):
    s = u.remain_set(name)
    hp = hot(**dict(u.SETS[name][3], **(WIDE if wide else {})))
    for con in range(s.hi.n_contigs):
        req, _, seqs = s.problems[con]
        want = s.host(con)
        if wide:
            _load_annot(hp, 0, s.hi.annots[con])
        else:
            hp.load_contig(0, s.hi.views[con], s.hi.annots[con])
        got = hp.circ_chain_batch(0, s.hi.contigs[con], seqs, req)
        print(name, con, len(req), "problems; stats", got.stats)
        assert got.stats[5] == 0 and 0 < got.stats[0] < len(req)          # nothing refused (a refused problem is the host's); tables are shared
        assert got.stats[3] == want.stats[3] and got.stats[4] == want.stats[4]
        assert got.bytes() == want.bytes()
        if not wide:                                                         # the contig resident in the slot instead of host bytes
            again = hp.circ_chain_batch(0, None, seqs, req)
            assert again.bytes() == want.bytes() and again.stats[5] == 0


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("ws", [8, 6])
def test_directed_problems(hot, ws, wide):
    s, D = u.remain_set("tiny"), u.directed(ws)
    hp = hot(**(WIDE if wide else {}))
    _load_annot(hp, 0, s.hi.annots[0])
    want = cl.circ_chain_host(hp.params, s.hi.annots[0], D.contig, D.seqs, D.req, ws)
    got = hp.circ_chain_batch(0, D.contig, D.seqs, D.req, ws)
    print("stats", got.stats)
    assert got.stats[5] == 0
    for g, ix in D.groups.items():
        for i in ix:
            assert got.chains(i) == want.chains(i) and got.res[i] == want.res[i], (g, i)
    assert got.bytes() == want.bytes()


@pytest.mark.parametrize("wide", [False, True])
def test_max_intron_binds(hot, wide):
    s = u.remain_set("tiny")
    req, seqs = u.junction_problems(s)
    hp = hot(max_intron=1000, **(WIDE if wide else {}))
    _load_annot(hp, 0, s.hi.annots[0])
    want = cl.circ_chain_host(hp.params, s.hi.annots[0], s.hi.contigs[0], seqs, req)
    loose = cl.circ_chain_host(cl.default_params(), s.hi.annots[0], s.hi.contigs[0], seqs, req)
    assert any(want.chains(i) != loose.chains(i) for i in range(len(req)))          # (else the case tests nothing)
    got = hp.circ_chain_batch(0, s.hi.contigs[0], seqs, req)
    assert got.bytes() == want.bytes() and got.stats[5] == 0


def test_table_budget_makes_gene_groups(hot, monkeypatch):
    s = u.remain_set("tiny")
    req, _, seqs = s.problems[0]
    hp = hot()
    _load_annot(hp, 0, s.hi.annots[0])
    monkeypatch.setenv("CM_CIRC_TABLE_BYTES", str(3 * 600_000))          # a table at ws = 8: 524 292 bytes + 4 per window
    got = hp.circ_chain_batch(0, s.hi.contigs[0], seqs, req)
    print("stats", got.stats)
    assert got.stats[2] >= 3 and got.stats[5] == 0 and got.stats[1] <= 3 * 600_000
    assert got.bytes() == s.host(0).bytes()
    monkeypatch.setenv("CM_CIRC_TABLE_BYTES", "1000")                     # no gene fits: every problem is refused, none is cut short
    none = hp.circ_chain_batch(0, s.hi.contigs[0], seqs, req)
    assert none.stats[5] == len(req) and (none.res["flags"] == 1).all() and len(none.score) == 0 and not none.res["n_chains"].any()


def test_log_cap_refuses_what_the_emulation_predicts(hot, monkeypatch):
    s = u.remain_set("tiny")
    req, _, seqs = s.problems[0]
    want = s.host(0)
    _, log_len = u.emu_chains(s.P, s.hi.annots[0], s.hi.contigs[0], seqs, req)
    cap = int(log_len.max()) - 1
    predicted = np.nonzero(log_len > cap)[0]
    assert 0 < len(predicted) < len(req)
    hp = hot()
    _load_annot(hp, 0, s.hi.annots[0])
    monkeypatch.setenv("CM_CIRC_LOG_CAP", str(cap))
    got = hp.circ_chain_batch(0, s.hi.contigs[0], seqs, req)
    assert np.array_equal(np.nonzero(got.res["flags"] & 1)[0], predicted) and got.stats[5] == len(predicted)
    for i in range(len(req)):
        if i in predicted:
            assert got.res[i]["n_chains"] == got.res[i]["n_stored"] == got.res[i]["listed"] == 0
        else:
            assert got.chains(i) == want.chains(i) and got.res[i]["n_chains"] == want.res[i]["n_chains"] and got.res[i]["listed"] == want.res[i]["listed"]


def test_edges(hot):
    s = u.remain_set("tiny")
    req, _, seqs = s.problems[0]
    want = s.host(0)
    hp = hot()
    _load_annot(hp, 0, s.hi.annots[0])
    g = s.hi.contigs[0]
    empty = hp.circ_chain_batch(0, g, seqs, req[:0])
    assert len(empty.res) == 0 and len(empty.score) == 0
    one = hp.circ_chain_batch(0, g, seqs, req[5:6])
    assert one.chains(0) == want.chains(5) and one.stats[0] == 1
    same_gene = np.nonzero((req["gene_start"] == req["gene_start"][0]) & (req["gene_end"] == req["gene_end"][0]))[0]
    sub = hp.circ_chain_batch(0, g, seqs, req[same_gene])
    assert sub.stats[0] == 1 and [sub.chains(k) for k in range(len(same_gene))] == [want.chains(i) for i in same_gene]
    # capacities one short: CM_ELIMIT, and the context goes on working
    for caps in (dict(cap_chains=len(want.score) - 1), dict(cap_frags=len(want.rpos) - 1)):
        with pytest.raises(RuntimeError, match=r"\(-6\).*room for"):
            hp.circ_chain_batch(0, g, seqs, req, **caps)
    exact = hp.circ_chain_batch(0, g, seqs, req, cap_chains=len(want.score), cap_frags=len(want.rpos))
    assert exact.bytes() == want.bytes()
    for ws in (5, 11):
        with pytest.raises(RuntimeError, match=r"\(-6\).*window size"):
            hp.circ_chain_batch(0, g, seqs, req[:4], ws)
    with pytest.raises(RuntimeError, match="slot 99 out of range"):
        hp.circ_chain_batch(99, g, seqs, req[:4])
    with pytest.raises(RuntimeError, match=r"\(-5\).*annotation of slot 3 not loaded"):
        hp.circ_chain_batch(3, g, seqs, req[:4])
    _load_annot(hp, 1, s.hi.annots[0])                                                  # an annotation and no contig in slot 1
    with pytest.raises(RuntimeError, match=r"\(-1\).*no contig is resident"):
        hp.circ_chain_batch(1, None, seqs, req[:4])
    assert hp.circ_chain_batch(0, g, seqs, req[:50]).chains(7) == want.chains(7)


def _files(prefix, tag):
    return open(f"{prefix}.{tag}.c", "rb").read(), open(f"{prefix}.{tag}.r", "rb").read()


def _trace(text):
    """the CM_CIRC_TRACE lines of the device path, summed over the contigs' calls: (problems, refused, answers taken, recomputed)"""
    ahead = re.findall(r"chains ahead \(device\): (\d+) problems, .*? (\d+) refused", text)
    fed = re.findall(r"(\d+) answers taken, (\d+) problems recomputed", text)
    assert ahead and fed, text
    return sum(int(a[0]) for a in ahead), sum(int(a[1]) for a in ahead), sum(int(f[0]) for f in fed), sum(int(f[1]) for f in fed)


@pytest.mark.parametrize("name", ["tiny", "tiny2r", "variety"])
def test_call_device_writes_the_same_files(hot, name, monkeypatch, capfd):
    s = u.remain_set(name)
    hp = hot(**u.SETS[name][3])
    cl.circ_call(s.P, s.hi, s.d.chr_table, s.b, s.prefix + ".host.c", s.prefix + ".host.r")
    want = _files(s.prefix, "host")
    assert want == oracle_stage2(s.tmp, s.ohi, s.d, s.P, gnu_sort(s.r1), gnu_sort(s.r2), tag="oracle_" + name) and want[0].count(b"\n") > 100
    monkeypatch.setenv("CM_CIRC_TRACE", "1")
    n_problems = sum(len(p[0]) for p in s.problems)
    for threads, log_cap in (("1", None), ("13", None), ("13", "20")):
        monkeypatch.setenv("CM_CIRC_THREADS", threads)
        if log_cap:
            monkeypatch.setenv("CM_CIRC_LOG_CAP", log_cap)          # some problems are refused and recomputed on the host
        capfd.readouterr()
        cl.circ_call_device(hp, s.P, s.hi, s.d.chr_table, s.b, s.prefix + ".dev.c", s.prefix + ".dev.r")
        assert _files(s.prefix, "dev") == want, (threads, log_cap)
        problems, refused, taken, recomputed = _trace(capfd.readouterr().err)
        assert problems == n_problems and taken > n_problems // 2          # the chains came from the device's answers ...
        if log_cap:
            assert 0 < refused < n_problems and recomputed > 0      # ... but for the refused ones a pair asked for (some of them twice)
        else:
            assert refused == 0 and recomputed == 0


def test_circ_run_on_the_device(built, tmp_path, monkeypatch, capfd):
    """the two-contig files of test_stage2_from_files_to_files"""
    from test_circ_call import _case
    d, gtf, (hi, ohi), P, prefix, r1, r2 = _case(tmp_path, "tiny2r", 2500, 23)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    packed, info = cl.pack_genome(fa, 150_000)
    idx = cl.write_index(packed, kmer=20, n_threads=4)
    cl.run_circ(idx, gtf, prefix, hi.n_contigs, cl.default_params(kmer=0))
    want = open(prefix + ".candidates.pam", "rb").read(), open(prefix + ".circ_report", "rb").read()
    os.remove(prefix + ".candidates.pam")
    os.remove(prefix + ".circ_report")
    monkeypatch.setenv("CM_CIRC_DEVICE", "1")
    monkeypatch.setenv("CM_CIRC_TRACE", "1")
    capfd.readouterr()
    st = cl.run_circ(idx, gtf, prefix, hi.n_contigs, cl.default_params(kmer=0))
    assert (open(prefix + ".candidates.pam", "rb").read(), open(prefix + ".circ_report", "rb").read()) == want
    problems, refused, taken, recomputed = _trace(capfd.readouterr().err)          # the variable was honoured and the context used
    assert problems > 1000 and refused == 0 and taken > problems // 2 and recomputed == 0
    assert st.calls > 0 and {r.split("\t")[1] for r in want[0].decode().strip().split("\n")} == {"chr1", "chr2"}
