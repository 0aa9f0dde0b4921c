"""k_chain_heavy's back-tracking against the oracle, path by path: the improvement log iterated in registers (up to
64 * CM_CHEAVY_LOG_REGS events) or level by level from memory, candidates of successive score levels walked as one batch, a batch
that ends within a level, the skip rule under each candidate's own score, the singleton path, and the log read again after a
pool retry.  Data: that of test_gpu_chain_heavy_bits.py (repeat families of 240 copies: problems over the heavy line), whole
reads at maxChainLen 30 / 12 / 5 / 1, and 45-bp windows of the same reads (two seeds: a log of at most cnt[0] * cnt[1] events).
Both batches run once more on a library whose register log holds 64 events (-DCM_CHEAVY_LOG_REGS=1), in a child process.

What the data must reach is counted from the oracle's seeds and chains alone (test_preconditions_from_the_oracle, no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from circminer_amd import lib as cl
from oracle import oracle_py as op
from conftest import DataSet, first_diff

CHR_LENS = [500_000, 300_000]
FAM_COPIES = 240
SEED = 51
N_PAIRS = 3000
N_CUT = 300                             # pairs appended again, cut to 39 bp: one seed per read
LIGHT_W, LIGHT_CELLS = 256, 96          # cm_hot.hip chain_light_w() / chain_light_cells()
CHAIN_LENS = (30, 12, 5, 1)
WIN, STRIDE, N_WIN_PAIRS = 45, 7, 1200
REG_EVENTS = 256                        # 64 * CM_CHEAVY_LOG_REGS of the product build
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Data:
    """DataSet-like: the genome, index and annotation of a DataSet under another read batch"""

    def __init__(self, ds, batch):
        self.d, self.hi, self.ohi, self.kmer, self.gtf, self.batch = ds.d, ds.hi, ds.ohi, ds.kmer, ds.gtf, batch


def _heavy(start, cnt, S):
    cnt = cnt.reshape(-1, S).astype(np.int64)
    cells = cnt.sum(1)
    later = np.cumsum(cnt[:, ::-1], 1)[:, ::-1] - cnt
    w = (cnt * later).sum(1)                             # (hit, later hit) pairs: k_chain_cls; an upper bound of the log's events
    return (cells > 0) & ((w > LIGHT_W) | (cells > LIGHT_CELLS)), w


@pytest.fixture(scope="module")
def data(tmp_path_factory, built):
    ds = DataSet(tmp_path_factory.mktemp("heavy_bt"), "tiny", N_PAIRS, SEED, chr_lens=CHR_LENS, fam_copies=FAM_COPIES)
    d = ds.d
    L = d.seq1.shape[1]
    s1 = np.concatenate([d.seq1.reshape(-1), d.seq1[:N_CUT, :39].reshape(-1)])
    s2 = np.concatenate([d.seq2.reshape(-1), d.seq2[:N_CUT, :39].reshape(-1)])
    ln = np.concatenate([np.full(N_PAIRS, L), np.full(N_CUT, 39)])
    full = _Data(ds, cl.ReadBatch(s1, s2, ln, ln))
    # 45-bp windows of every read at 7-bp strides; of these, pairs with a heavy problem whose log fits the registers for certain
    offs = np.arange(0, L - WIN + 1, STRIDE)
    w1 = np.concatenate([d.seq1[:, o:o + WIN] for o in offs])
    w2 = np.concatenate([d.seq2[:, o:o + WIN] for o in offs])
    n_all = len(w1)
    lw = np.full(n_all, WIN)
    allw = cl.ReadBatch(w1.reshape(-1), w2.reshape(-1), lw, lw)
    P = cl.default_params(kmer=ds.kmer)
    S = WIN // ds.kmer
    start, cnt, _ = op.seeds(P, ds.ohi.views[0], allw, S)
    hv, w = _heavy(start[:n_all * 4 * S], cnt[:n_all * 4 * S], S)
    ch, n, _ = op.chains(P, ds.ohi.views[0], ds.ohi.annots[0], allw)
    ch = ch.reshape(-1, cl.CM_BESTCHAINLIM)
    two = (n[:n_all * 4] > 0) & (ch[:n_all * 4, 0]["chain_len"] >= 2)         # (chain 0 is a longest one of the best score)
    wit = hv & (w > 0) & (w <= REG_EVENTS) & two
    pairs = np.nonzero(wit.reshape(-1, 4).any(1))[0][:N_WIN_PAIRS]
    cut = _Data(ds, cl.ReadBatch(w1[pairs].reshape(-1), w2[pairs].reshape(-1), lw[:len(pairs)], lw[:len(pairs)]))
    return dict(full=full, cut=cut, n_windows=n_all, cut_witnesses=int(wit.reshape(-1, 4)[pairs].sum()))


_want = {}


@pytest.fixture(scope="module")
def want(data):
    """the oracle's seeds, chains and states after the (one) round of a batch at a maxChainLen, each computed once"""
    def get(which, m):
        if (which, m) not in _want:
            ds = data[which]
            P = cl.default_params(kmer=ds.kmer, max_chain_len=m)
            S = ds.batch.max_len() // P.kmer
            ch = op.chains(P, ds.ohi.views[0], ds.ohi.annots[0], ds.batch)
            st, act = op.default_state(P, ds.batch.n)
            cat = op.map_round(P, ds.ohi.views[0], ds.ohi.annots[0], ds.batch, True, st, act)
            start, cnt, _ = op.seeds(P, ds.ohi.views[0], ds.batch, S)
            k = ds.batch.n * 4 * S
            _want[(which, m)] = dict(chains=ch, st=st, act=act, cat=cat, heavy=_heavy(start[:k], cnt[:k], S)[0], w=_heavy(start[:k], cnt[:k], S)[1])
        return _want[(which, m)]
    return get


def _records(wt):
    ch, n, _ = wt["chains"]
    return ch.reshape(-1, cl.CM_BESTCHAINLIM), n


def _frags(c):
    L = int(c["chain_len"])
    return [(int(c["rpos"][f]), int(c["qpos"][f])) for f in range(L)]


def test_preconditions_from_the_oracle(data, want):
    """Every path of the back-tracking has its witnesses in the data, counted from the oracle's output."""
    kmer = data["full"].kmer
    got = {}
    for m in (30, 12, 5):
        wt = want("full", m)
        ch, n = _records(wt)
        heavy = np.nonzero(wt["heavy"])[0]
        beyond = same = 0
        for r in heavy:
            if n[r] != m:
                continue
            c = ch[r, :m]
            sc = c["score"].astype(np.float64)
            # the suffix of an earlier chain of >= 3 fragments scores (its score - 2e4 * kmer + a gap cost): a candidate of a level
            # above the last chain's that the skip rule dropped, so the emitted chains are not the first maxChainLen candidates
            if ((c["chain_len"][:-1] >= 3) & (sc[-1] < sc[:-1] - 2e4 * kmer - 1)).any():
                beyond += 1
            if (sc == sc[0]).all() and c["chain_len"][0] >= 2:      # (out of the log, not the singleton path)
                same += 1
        got[m] = (beyond, same)
    assert all(got[m][0] >= 500 for m in got), got
    assert got[30][1] >= 5 and got[12][1] >= 15 and got[5][1] >= 25, got
    wt = want("full", 30)
    ch, n = _records(wt)
    heavy = np.nonzero(wt["heavy"])[0]
    exhausted = levels3 = big_log = single = 0
    for r in heavy:
        c = ch[r, :n[r]]
        if n[r] == 0:
            continue
        if (c["chain_len"] == 1).all():
            single += 1
        if len(np.unique(c["score"])) >= 3:
            levels3 += 1
        fr = [_frags(x) for x in c]
        if n[r] < 30 and len(fr[0]) >= 3 and all(f[0] != fr[0][1] for f in fr):
            exhausted += 1
        if len({f for x in fr for f in x[:-1]}) > 64:          # each is an improved cell, hence an event
            big_log += 1
    assert exhausted >= 100 and levels3 >= 300 and big_log >= 200 and single >= 20, (exhausted, levels3, big_log, single)
    assert data["n_windows"] == 48_000 and data["cut"].batch.n == N_WIN_PAIRS and data["cut_witnesses"] >= 1000, \
        (data["n_windows"], data["cut"].batch.n, data["cut_witnesses"])
    wc = want("cut", 30)
    reg = wc["heavy"] & (wc["w"] > 0) & (wc["w"] <= REG_EVENTS)
    assert reg.sum() >= 1000, reg.sum()
    print("witnesses:", got, dict(exhausted=exhausted, levels3=levels3, big_log=big_log, single=single, register_log=int(reg.sum())))


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


def _check(ds, wt, m):
    hp = cl.HotPath(cl.default_params(kmer=ds.kmer, max_chain_len=m))
    hp.load_contig(0, ds.hi.views[0], ds.hi.annots[0])
    hp.upload(ds.batch)
    _chains_equal(hp.chains(0), wt["chains"])
    hp.reset()
    hp.map_round(0, True)
    st, cat, act = hp.download()
    assert (cat == wt["cat"]).all(), np.nonzero(cat != wt["cat"])[0][:10]
    assert (act == wt["act"]).all()
    assert st.tobytes() == wt["st"].tobytes(), first_diff(wt["st"], st)
    hp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("m", CHAIN_LENS)
def test_whole_reads_equal_the_oracle(data, want, m):
    _check(data["full"], want("full", m), m)


@pytest.mark.gpu
def test_two_seed_windows_equal_the_oracle(data, want):
    _check(data["cut"], want("cut", 30), 30)


@pytest.mark.gpu
def test_log_pool_recovery(data, want, monkeypatch):
    """a 64-KB improvement log that may grow to 256 KB (test_gpu_chain_heavy_bits.py): after a retry the log of a problem lies
    elsewhere and is read again, from registers or from memory"""
    monkeypatch.setenv("CM_POOL_BYTES", "65536")
    monkeypatch.setenv("CM_POOL_MAX", "262144")
    _check(data["full"], want("full", 30), 30)


@pytest.mark.gpu
def test_register_log_of_64_events():
    """Both batches on a library built with -DCM_CHEAVY_LOG_REGS=1: the whole reads' logs of more than 64 events (the memory path:
    `big_log` of the preconditions) beside those that fit, the windows' logs on either side of 64.  ONE child process (the library
    is chosen at import time through CM_LIB)."""
    from circminer_amd import _build
    so = _build.build(tag="logregs1", flags=["-DCM_CHEAVY_LOG_REGS=1"])
    env = dict(os.environ, CM_LIB=so)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "test_whole_reads_equal_the_oracle and 30 or test_two_seed_windows_equal_the_oracle"],
                       env=env, capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and "\n2 passed" in r.stdout
