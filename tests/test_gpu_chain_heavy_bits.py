"""k_chain_heavy's two bit sets against the oracle: the near-border bits by index entry (Slot::entry_near, made from the index AND
the annotation of a slot: it must follow every (un)load of either) and the improved bits (only improved DP cells reach HBM; every
reader takes the initial score / back pointer of the others from the bit).  Data: a 0.8-Mbp genome whose repeat families have 240
copies, so that reads from a copy give chaining problems over the heavy line (more than 96 hits or more than 256 hit pairs), plus
one-seed reads cut from them (nothing to chain: the singleton path on a heavy problem)."""
import ctypes as C
import os

import numpy as np
import pytest

from circminer_amd import lib as cl, synth
from oracle import oracle_py as op
from conftest import DataSet, first_diff

CHR_LENS = [500_000, 300_000]
FAM_COPIES = 240
SEED = 51
N_PAIRS = 3000
N_CUT = 300            # pairs appended again, cut to 39 bp: one seed per read
LIGHT_W, LIGHT_CELLS = 256, 96          # cm_hot.hip chain_light_w() / chain_light_cells()


class _Data:
    """DataSet-like: the genome, index and annotation of a DataSet under another read batch"""

    def __init__(self, ds, batch):
        self.d, self.hi, self.ohi, self.kmer, self.gtf, self.batch = ds.d, ds.hi, ds.ohi, ds.kmer, ds.gtf, batch


@pytest.fixture(scope="module")
def ds_heavy(tmp_path_factory, built):
    ds = DataSet(tmp_path_factory.mktemp("heavy"), "tiny", N_PAIRS, SEED, chr_lens=CHR_LENS, fam_copies=FAM_COPIES)
    d = ds.d
    L = d.seq1.shape[1]
    s1 = np.concatenate([d.seq1.reshape(-1), d.seq1[:N_CUT, :39].reshape(-1)])
    s2 = np.concatenate([d.seq2.reshape(-1), d.seq2[:N_CUT, :39].reshape(-1)])
    ln = np.concatenate([np.full(N_PAIRS, L), np.full(N_CUT, 39)])
    return _Data(ds, cl.ReadBatch(s1, s2, ln, ln))


@pytest.fixture(scope="module")
def want(ds_heavy):
    """the oracle's chains and its states after the (one) round, computed once"""
    ds = ds_heavy
    P = cl.default_params(kmer=ds.kmer)
    ch = op.chains(P, ds.ohi.views[0], ds.ohi.annots[0], ds.batch)
    st, act = op.default_state(P, ds.batch.n)
    cat = op.map_round(P, ds.ohi.views[0], ds.ohi.annots[0], ds.batch, True, st, act)
    return dict(chains=ch, st=st, act=act, cat=cat)


def _chains_equal(got, ref):
    (c1, n1, h1), (c0, n0, h0) = got, ref
    assert (n0 == n1).all(), np.nonzero(n0 != n1)[0][:10]
    assert (h0 == h1).all()
    a, b = c0.reshape(-1, cl.CM_BESTCHAINLIM), c1.reshape(-1, cl.CM_BESTCHAINLIM)
    for r in np.nonzero(n0)[0]:
        for k in range(n0[r]):
            x, y = a[r, k], b[r, k]
            L = int(x["chain_len"])
            assert L == int(y["chain_len"]), (r, k)
            assert x["score"] == y["score"], (r, k, x["score"], y["score"])      # fp32 of the fp64 sum, exact
            assert (x["rpos"][:L] == y["rpos"][:L]).all() and (x["qpos"][:L] == y["qpos"][:L]).all(), (r, k)


def _preconditions(ds, start, cnt, S, ref_chains):
    """The data reaches what the tests are about (so that they cannot pass vacuously), from the seed ranges (first entry, count per
    problem and seed), the index's positions, the annotation's bitset and the oracle's chains."""
    start, cnt = start.reshape(-1, S).astype(np.int64), cnt.reshape(-1, S).astype(np.int64)
    cells = cnt.sum(1)
    later = np.cumsum(cnt[:, ::-1], 1)[:, ::-1] - cnt
    w = (cnt * later).sum(1)                             # (hit, later hit) pairs: k_chain_cls
    heavy = np.nonzero((cells > 0) & ((w > LIGHT_W) | (cells > LIGHT_CELLS)))[0]
    assert len(heavy) >= 100, len(heavy)
    iv, av = ds.hi.views[0], ds.hi.annots[0]
    pos = np.ctypeslib.as_array(iv.pos, (int(iv.n_entries),))
    bits = np.ctypeslib.as_array(av.near_border_bits, (int(av.n_bits) // 64,))
    p = np.concatenate([pos[start[r, s]:start[r, s] + cnt[r, s]] for r in heavy for s in range(S) if cnt[r, s]]).astype(np.int64)
    near = np.zeros(len(p), bool)
    ok = p < int(av.n_bits)
    near[ok] = ((bits[p[ok] >> 6] >> (p[ok] & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    assert 0.01 <= near.mean() <= 0.99, near.mean()
    # A problem's chains come either out of its improvement log (every logged cell has a back pointer: two fragments or more; the
    # walk ends in an unimproved cell) or, when nothing was improved, from the singleton path (all of length 1): no problem has
    # both, so the two are asked of the heavy problems as a set.
    ch, n, _ = ref_chains
    ch = ch.reshape(-1, cl.CM_BESTCHAINLIM)
    longest = np.array([ch[r, :n[r]]["chain_len"].max() if n[r] else 0 for r in heavy])
    shortest = np.array([ch[r, :n[r]]["chain_len"].min() if n[r] else 0 for r in heavy])
    assert (longest >= 3).sum() >= 1 and (shortest == 1).sum() >= 1, ((longest >= 3).sum(), (shortest == 1).sum())
    return heavy


def _loaded(ds, P):
    hp = cl.HotPath(P)
    hp.load_contig(0, ds.hi.views[0], ds.hi.annots[0])
    hp.upload(ds.batch)
    return hp


@pytest.mark.gpu
def test_heavy_chains_equal_the_oracle(ds_heavy, want):
    ds = ds_heavy
    P = cl.default_params(kmer=ds.kmer)
    hp = _loaded(ds, P)
    start, cnt, _, S = hp.seeds(0)
    _preconditions(ds, start, cnt, S, want["chains"])
    _chains_equal(hp.chains(0), want["chains"])
    hp.close()


def _round_equals(hp, want):
    hp.reset()
    hp.map_round(0, True)
    st, cat, act = hp.download()
    assert (cat == want["cat"]).all(), np.nonzero(cat != want["cat"])[0][:10]
    assert (act == want["act"]).all()
    assert st.tobytes() == want["st"].tobytes(), first_diff(want["st"], st)


@pytest.mark.gpu
def test_all_rounds_equal_the_oracle(ds_heavy, want):
    hp = _loaded(ds_heavy, cl.default_params(kmer=ds_heavy.kmer))
    _round_equals(hp, want)
    hp.close()


@pytest.fixture(scope="module")
def others(ds_heavy, tmp_path_factory):
    """What the slot holds in the staleness test besides the data set itself: a second annotation of the same genome (genes of another
    seed) and a second genome under the first annotation (the first, rotated by 137 bp: the same repeats, every hit elsewhere
    relative to the exons), each with the oracle's own index / annotation."""
    ds = ds_heavy
    tmp = tmp_path_factory.mktemp("heavy_others")
    names = [t[0] for t in ds.d.chr_table]
    genes2 = synth.make_genes(np.random.default_rng(SEED + 1000), CHR_LENS, genes_per_mbp=synth.PRESETS["tiny"][1])
    gtf2 = os.path.join(str(tmp), "genes2.gtf")
    with open(gtf2, "w") as f:
        f.write(synth.gtf_text(genes2, names))
    hi2 = cl.HostIndex(ds.d.contigs, ds.d.chr_table, gtf2, kmer=ds.kmer)
    ohi2 = op.OracleIndex(ds.d.contigs, ds.d.chr_table, gtf2, kmer=ds.kmer)
    rot = [np.ascontiguousarray(np.roll(c, 137)) for c in ds.d.contigs]
    ohi_rot = op.OracleIndex(rot, ds.d.chr_table, ds.gtf, kmer=ds.kmer)
    P = cl.default_params(kmer=ds.kmer)
    return dict(annot2=hi2.annots[0], rot=rot[0], keep=(hi2, ohi2, ohi_rot),
                chains_annot2=op.chains(P, ohi2.views[0], ohi2.annots[0], ds.batch),
                chains_rot=op.chains(P, ohi_rot.views[0], ohi_rot.annots[0], ds.batch))


@pytest.mark.gpu
def test_entry_bits_follow_every_load_of_either_half(ds_heavy, want, others, tmp_path):
    ds = ds_heavy
    P = cl.default_params(kmer=ds.kmer)
    iv, av = ds.hi.views[0], ds.hi.annots[0]
    assert ds.hi.n_contigs == 1
    packed = str(tmp_path / "ref.fa.packed.fa")
    with open(packed, "w") as f:
        f.write(f">1\n{ds.d.contigs[0].tobytes().decode()}\n")
    idx = cl.write_index(packed, kmer=ds.kmer, n_threads=4)
    hp = cl.HotPath(P)
    hp.upload(ds.batch)

    def annotation(a):
        hp._chk(hp.L.cm_load_annotation(hp.h, 0, C.byref(a)), "cm_load_annotation")

    def check(ref):
        _chains_equal(hp.chains(0), ref)

    # (a) the annotation first, then the contig; and the usual order
    annotation(av)
    hp.load_contig(0, iv)
    check(want["chains"])
    hp._chk(hp.L.cm_unload_contig(hp.h, 0), "cm_unload_contig")
    hp.load_contig(0, iv, av)
    check(want["chains"])
    # (b) another annotation under the resident contig, and back
    annotation(others["annot2"])
    check(others["chains_annot2"])
    annotation(av)
    check(want["chains"])
    # (c) the contig replaced under the resident annotation, through every loader
    raw = cl.IndexFile(idx, n_threads=2, raw=True)
    for load in (lambda: hp.load_contig(0, iv), lambda: hp.load_contig_raw(0, next(raw)), lambda: hp.build_contig(0, 0, ds.d.contigs[0])):
        hp.build_contig(0, 0, others["rot"])
        check(others["chains_rot"])
        load()
        check(want["chains"])
    raw.close()
    hp.close()


@pytest.mark.gpu
def test_log_pool_recovery_on_heavy_problems(ds_heavy, want, monkeypatch):
    """a 64-KB improvement log that may grow to 256 KB: the stage is redone with a larger pool, then in halves on the
    one-lane-per-problem kernel (tests/test_gpu_parity.py test_improvement_log_pool_recovers, on problems of the heavy kernel)"""
    monkeypatch.setenv("CM_POOL_BYTES", "65536")
    monkeypatch.setenv("CM_POOL_MAX", "262144")
    hp = _loaded(ds_heavy, cl.default_params(kmer=ds_heavy.kmer))
    _chains_equal(hp.chains(0), want["chains"])
    _round_equals(hp, want)
    hp.close()


def test_host_emulation_on_the_heavy_data(emu, ds_heavy, want):
    """the kernel bodies shared with the device (cm_core.h: every problem through chain_kbest, the heavy ones in ChainStoreGlobal)"""
    ds = ds_heavy
    P = cl.default_params(kmer=ds.kmer)
    iv, av, b = ds.hi.views[0], ds.hi.annots[0], ds.batch
    S = b.max_len() // P.kmer
    start, cnt, _ = op.seeds(P, iv, b, S)
    _preconditions(ds, start, cnt, S, want["chains"])
    ch, n, h = (np.zeros_like(x) for x in want["chains"])
    assert emu.emu_chain_batch(C.byref(P), C.byref(iv), C.byref(av), C.byref(b.c), ch.ctypes.data, n.ctypes.data, h.ctypes.data) == 0
    _chains_equal((ch, n, h), want["chains"])
    st, act = op.default_state(P, b.n)
    cat = np.full(b.n, -1, np.int32)
    assert emu.emu_map_round(C.byref(P), C.byref(iv), C.byref(av), C.byref(b.c), 1, st.ctypes.data, act.ctypes.data, cat.ctypes.data) == 0
    assert (cat == want["cat"]).all() and (act == want["act"]).all() and st.tobytes() == want["st"].tobytes()
