"""Stage 2's seeds and chains computed ahead, without a device: the bodies of circminer_amd/csrc/cm_circ_chain.h in the kernels'
shapes (tests/hostemu_circ_chain.cpp: lanes, cells and problems in shuffled order) against the serial statement
(cm_regional_table_build, Caller::chains_of behind cm_circ_chain_host), the listing against one written from its rule, and the
provider path of cm_circ_call_device against cm_circ_call and the oracle."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

from circminer_amd import lib as cl
import circ_chain_util as u
from stage2_util import gnu_sort, oracle_stage2

needs_coreutils = pytest.mark.skipif(not all(shutil.which(x) for x in ("paste", "sort", "tr")), reason="GNU coreutils not on PATH")


# ---- tables ---------------------------------------------------------------------------------------------------------------
def _same_table(gene: bytes, ws: int, seed=3):
    (eo, el), (ho, hl) = u.emu_table(gene, ws, seed), u.host_table(gene, ws)
    assert np.array_equal(eo, ho) and np.array_equal(el, hl), (len(gene), ws)
    return ho, hl


@pytest.mark.parametrize("ws", [8, 6])
def test_tables_of_real_genes(built, ws):
    for name in ("tiny", "variety"):
        s = u.remain_set(name)
        for con in range(s.hi.n_contigs):
            av, g = s.hi.annots[con], s.hi.contigs[con]
            gs, ge = np.ctypeslib.as_array(av.gene_start, (av.n_gene,)), np.ctypeslib.as_array(av.gene_end, (av.n_gene,))
            for k in range(av.n_gene):
                off, loc = _same_table(bytes(g[gs[k] - 1:ge[k]]), ws)
                assert off[-1] == len(loc) > 0


@pytest.mark.parametrize("ws", [8, 6])
def test_tables_of_fabricated_genes(built, ws):
    rng = np.random.default_rng(5)
    # a tandem repeat of period 10: its 10 windows have 1001, 1001, ..., 1000, 1000 hits -- a bucket of exactly 1000 stays, 1001 is emptied
    unit = b"ACGTTGCAGA" if ws == 8 else b"ACGTTGCAGA"
    n_win = 10005
    gene = (unit * 1002)[:n_win + ws - 1]
    off, loc = _same_table(gene, ws)
    sizes = np.diff(off)
    assert sorted(sizes[sizes > 0].tolist()) == [1000] * 5 and off[-1] == 5000          # the five windows with 1001 hits are gone
    for h in np.nonzero(sizes)[0]:
        assert (np.diff(loc[off[h]:off[h + 1]]) == 10).all()                            # ascending offsets inside the gene
    _same_table(u._rand(rng, ws - 1), ws)                                               # a gene shorter than a window: no hit
    assert _same_table(b"", ws)[0][-1] == 0
    assert _same_table(u._rand(rng, ws), ws)[0][-1] == 1
    mixed = bytearray(u._rand(rng, 3000))
    mixed[100:160] = b"N" * 60
    mixed[700:1200] = bytes(mixed[700:1200]).lower()
    mixed[2000] = 0
    mixed[2500:2503] = b"xyz"
    off, loc = _same_table(bytes(mixed), ws)
    assert not ((loc > 100 - ws) & (loc < 160)).any() and ((loc >= 700) & (loc < 1190)).sum() == 490
    for seed in (1, 2):                                                                 # the order positions are placed in does not show
        assert np.array_equal(u.emu_table(bytes(mixed), ws, seed)[1], loc)


def test_tables_at_the_contigs_ends(built):
    """a gene at position 1, one that ends beyond ref_len (genome_at refuses it: all NUL, no hit), seen through the chains"""
    s, D = u.remain_set("tiny"), u.directed()
    h = cl.circ_chain_host(s.P, s.hi.annots[0], D.contig, D.seqs, D.req)
    first, (beyond, zero) = D.groups["first_gene"][0], D.groups["refused_genes"]
    assert h.res[first]["n_chains"] == 1 and h.chains(first)[0][1][0] == (11, 0)         # contig[10:] found at contig position 11
    for i in (beyond, zero):
        assert h.res[i]["n_chains"] == 0 and h.res[i]["listed"] > 20


# ---- chains ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny2r", "variety", "long300"])
def test_chains_of_real_remain_pairs(built, name):
    s = u.remain_set(name)
    total = 0
    for con in range(s.hi.n_contigs):
        req, pair_of, seqs = s.problems[con]
        want = s.host(con)
        got, log_len = u.emu_chains(s.P, s.hi.annots[con], s.hi.contigs[con], seqs, req, seed=11 + con)
        assert got.bytes() == want.bytes()
        assert got.stats[3] == want.stats[3] and got.stats[4] == want.stats[4] == int(log_len.sum()) and got.stats[5] == 0
        assert got.stats[0] == want.stats[0] < len(req)
        total += len(req)
    assert total > 1000
    if name == "long300":
        assert max(int(s.host(c).res["listed"].max()) for c in range(s.hi.n_contigs)) > 64      # more lists than a wave has lanes


@pytest.mark.parametrize("ws", [8, 6])
def test_directed_problems(built, ws):
    s, D = u.remain_set("tiny"), u.directed(ws)
    av = s.hi.annots[0]
    want = cl.circ_chain_host(s.P, av, D.contig, D.seqs, D.req, ws)
    got, log_len = u.emu_chains(s.P, av, D.contig, D.seqs, D.req, ws, seed=5)
    for g, ix in D.groups.items():
        for i in ix:
            assert got.chains(i) == want.chains(i) and got.res[i] == want.res[i], (g, i)
    assert got.bytes() == want.bytes()
    # the cases are what they claim to be
    res = want.res
    sp = D.groups["spans"]
    assert [int(res[i]["listed"]) for i in sp[:4]] == [0, 1, 1, 2] and res[sp[0]]["n_chains"] == 0 and res[sp[4]]["n_chains"] == 1
    assert all(res[i]["listed"] == 0 and res[i]["n_chains"] == 0 for i in D.groups["invalid"])
    tr = D.groups["trailing"][0]
    assert b"T" not in bytes(D.contig[D.genes["no_t"][0] - 1:D.genes["no_t"][1]])           # the poly-T tail's seeds have no hit in the gene ...
    assert res[tr]["listed"] > len(want.chains(tr)[0][1]) + 20                            # ... so far more seeds are listed than chained
    fam = D.groups["family"]
    assert max(int(res[i]["n_chains"]) for i in fam) == s.P.max_chain_len > 10 and max(int(log_len[i]) for i in fam) > s.P.max_chain_len
    assert all(res[i]["n_stored"] == min(int(res[i]["n_chains"]), 10) for i in range(len(res)))
    for i in fam:                                                                          # many entries of one score
        scores = [c[0] for c in want.chains(i)]
        assert len(scores) < 10 or len(set(scores[:10])) < 10
    lim500, lim501 = D.groups["seed_lim"]
    assert log_len[lim500] > 4 * log_len[lim501]          # 501 hits > seed_lim: those lists are listed with n = 0
    assert res[lim500]["listed"] == res[lim501]["listed"]
    for i in D.groups["no_improvement"]:
        assert log_len[i] == 0 and res[i]["n_chains"] >= 1 and all(len(c[1]) == 1 for c in want.chains(i))
    two = want.chains(D.groups["no_improvement"][0])
    assert two[0][1][0][1] > two[1][1][0][1]                                               # single seeds, last list first
    assert res[D.groups["short_gene"][0]]["n_chains"] == 0


def test_hit_counts_around_a_wave(built):
    """lists of 63 / 64 / 65 hits (the family genes), seen in the tables the problems use"""
    D = u.directed()
    for copies in (63, 64, 65):
        gs, ge = D.genes[f"rep{copies}"]
        off, _ = u.host_table(bytes(D.contig[gs - 1:ge]), 8)
        assert copies in np.diff(off)


def test_max_intron_binds(built):
    s = u.remain_set("tiny")
    req, seqs = u.junction_problems(s)
    av, g = s.hi.annots[0], s.hi.contigs[0]
    tight = cl.default_params(max_intron=1000)
    want, loose = cl.circ_chain_host(tight, av, g, seqs, req), cl.circ_chain_host(cl.default_params(), av, g, seqs, req)
    changed = [i for i in range(len(req)) if want.chains(i) != loose.chains(i)]
    assert len(req) >= 5 and changed                          # (if no problem changes, the case tests nothing)
    assert any(len(loose.chains(i)[0][1]) > len(want.chains(i)[0][1]) for i in changed)     # the chain over the intron is gone
    for P, ref in ((tight, want), (cl.default_params(), loose)):
        assert u.emu_chains(P, av, g, seqs, req, seed=9)[0].bytes() == ref.bytes()


def test_refusal_by_log_capacity(built):
    s = u.remain_set("tiny")
    req, _, seqs = s.problems[0]
    av, g = s.hi.annots[0], s.hi.contigs[0]
    want = s.host(0)
    _, log_len = u.emu_chains(s.P, av, g, seqs, req)
    top = int(log_len.max())
    at_cap, _ = u.emu_chains(s.P, av, g, seqs, req, log_cap=top)
    assert at_cap.stats[5] == 0 and at_cap.bytes() == want.bytes()
    below, _ = u.emu_chains(s.P, av, g, seqs, req, log_cap=top - 1)
    hit = np.nonzero(log_len == top)[0]
    assert np.array_equal(np.nonzero(below.res["flags"] & cl.CIRC_CHAIN_REFUSED)[0], hit) and below.stats[5] == len(hit) > 0
    for i in range(len(req)):
        if i in hit:
            assert tuple(below.res[i])[:4] == (0, 0, 0, 1) and below.chains(i) == []          # refused, never truncated
        else:
            assert below.chains(i) == want.chains(i) and tuple(below.res[i])[:4] == tuple(want.res[i])[:4]
    cells = u.emu_chains(s.P, av, g, seqs, req, cell_cap=8)[0]                               # and by cell capacity
    assert 0 < cells.stats[5] < len(req)


def test_bad_requests_are_refused_by_both(built):
    s = u.remain_set("tiny")
    req, _, seqs = s.problems[0]
    av, g = s.hi.annots[0], s.hi.contigs[0]
    for field, value in (("qs", 0), ("qe", 10_000), ("seq_off", len(seqs)), ("gene_end", 0)):
        bad = req[:3].copy()
        bad[field][1] = value
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            cl.circ_chain_host(s.P, av, g, seqs, bad)
    for ws in (5, 11):
        with pytest.raises(RuntimeError, match=r"\(-6\)"):
            cl.circ_chain_host(s.P, av, g, seqs, req[:3], ws)
    with pytest.raises(RuntimeError, match=r"\(-6\).*needs \d+ chains"):
        cl.circ_chain_host(s.P, av, g, seqs, req, cap_chains=len(s.host(0).score) - 1)
    assert len(cl.circ_chain_host(s.P, av, g, seqs, req[:0]).res) == 0


# ---- listing and the provider path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny2r", "variety"])
def test_listing_equals_the_rule(built, name):
    s = u.remain_set(name)
    kinds = set()
    for con in range(s.hi.n_contigs):
        req, pair_of, seqs = s.problems[con]
        want_req, want_pair, want_seqs = u.py_list_requests(s.hi.annots[con], s.d.chr_table, s.b, con)
        assert req.tobytes() == want_req.tobytes() and np.array_equal(pair_of, want_pair) and seqs.tobytes() == want_seqs.tobytes()
        kinds |= set(s.b.prior["type"][pair_of.astype(np.int64)].tolist())
    assert kinds == {u.CM_CHIBSJ, u.CM_CHI2BSJ}


@needs_coreutils
@pytest.mark.parametrize("name", ["tiny", "tiny2r", "variety"])
def test_provider_path_writes_the_same_files(built, name, monkeypatch, capfd):
    """cm_circ_call_device without a context: the answers of cm_circ_chain_host fed back through the Caller's provider path"""
    s = u.remain_set(name)
    cl.circ_call(s.P, s.hi, s.d.chr_table, s.b, s.prefix + ".host.c", s.prefix + ".host.r")
    want = open(s.prefix + ".host.c", "rb").read(), open(s.prefix + ".host.r", "rb").read()
    assert want == oracle_stage2(s.tmp, s.ohi, s.d, s.P, gnu_sort(s.r1), gnu_sort(s.r2), tag="oracle_cpu_" + name)
    assert want[0].count(b"\n") > 100 and want[1].count(b"\n") > 20
    monkeypatch.setenv("CM_CIRC_TRACE", "1")
    for threads in ("1", "13"):
        monkeypatch.setenv("CM_CIRC_THREADS", threads)
        st = cl.circ_call_device(None, s.P, s.hi, s.d.chr_table, s.b, s.prefix + ".prov.c", s.prefix + ".prov.r")
        assert (open(s.prefix + ".prov.c", "rb").read(), open(s.prefix + ".prov.r", "rb").read()) == want
        assert st.candidate_rows == want[0].count(b"\n")
        trace = capfd.readouterr().err
        n_problems = sum(len(p[0]) for p in s.problems)
        assert f"chains ahead (host): {n_problems} problems" in trace
        m = re.search(r"(\d+) answers taken, (\d+) problems recomputed", trace)
        assert int(m.group(1)) > n_problems // 2 and int(m.group(2)) == 0      # every chain came from the answers (a pair that is finished early does not ask for its later genes)


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="a device is present")
def test_device_path_without_a_device_is_an_error(built, tmp_path, monkeypatch):
    from test_circ_call import _case
    d, gtf, (hi, ohi), P, prefix, r1, r2 = _case(tmp_path, "tiny", 300, 3)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    packed, info = cl.pack_genome(fa, 1_100_000_000)
    idx = cl.write_index(packed, kmer=20, n_threads=4)
    monkeypatch.setenv("CM_CIRC_DEVICE", "1")
    with pytest.raises(RuntimeError, match=r"\(-2\).*CM_CIRC_DEVICE=1 and no HIP device \(CM_ENODEV\)"):
        cl.run_circ(idx, gtf, prefix, hi.n_contigs, cl.default_params(kmer=0))
    assert not os.path.exists(prefix + ".candidates.pam")          # no silent host fall-back
    monkeypatch.delenv("CM_CIRC_DEVICE")
    cl.run_circ(idx, gtf, prefix, hi.n_contigs, cl.default_params(kmer=0))
    assert os.path.exists(prefix + ".candidates.pam")


def test_abi_of_the_new_structs(built):
    L = cl.load()
    two = (C.c_uint32 * 2)()
    assert L.cm_circ_chain_abi_sizes(two, 2) == 2 and list(two) == [C.sizeof(cl.CircChainReq), C.sizeof(cl.CircChainRes)] == [32, 24]
    assert L.cm_circ_chain_abi_sizes(two, 1) == -1 and L.cm_circ_chain_abi_sizes(None, 2) == -1
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(u.ROOT, "include", "circminer_hot.h")).read(), flags=re.S)
    for name in ("cm_circ_chain_batch", "cm_circ_chain_host", "cm_circ_chain_list", "cm_circ_call_device", "cm_circ_chain_abi_sizes"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(L, name) and name in cl.EXPORTED_SYMBOLS
    assert L.cm_circ_chain_batch(None, 0, 0, None, 0, None, 0, None, 0, None, None, None, None, 0, None, None, 0, None, None, None) == -1
