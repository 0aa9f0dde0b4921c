"""k_seed's k-mer word loads and per-wave counters on the device: HotPath.seeds against the oracle's seed batch on reads whose k-mer
spans reach the slack around the read buffers, sit at every byte alignment, hold lower case and N, and belong in part to retired
pairs; the three public counters against counts made on the host."""
import ctypes as C

import numpy as np
import pytest

from circminer_amd import lib as cl
from oracle import oracle_py as op
from seed_words_util import load_emu_seed, mixed_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ds_by_k(tmp_path_factory, built, ds_tiny2r):
    """tiny2r's genome under an index of k = 14, 20, 22 (k = 20: the session's data set)"""
    from conftest import DataSet
    made = {20: ds_tiny2r}

    def get(k):
        if k not in made:
            made[k] = DataSet(tmp_path_factory.mktemp(f"tiny2r_k{k}"), "tiny2r", 1200, 22, kmer=k)
        return made[k]
    return get


def _oracle(ds, P, batch, S):
    return op.seeds(P, ds.ohi.views[0], batch, S)          # (start, cnt, raw), one per (pair, mate, orientation, s)


def _compare(got, want, act, S):
    """cnt and raw everywhere, start where raw > 0; a retired pair has no seeds"""
    a1, b1, c1 = got
    keep = np.repeat(act != 0, 4 * S)
    a0, b0, c0 = (np.where(keep, x, 0) for x in want)
    assert (c0 == c1).all() and (b0 == b1).all()
    assert (a0[c0 > 0] == a1[c0 > 0]).all()
    return b0, c0


def test_the_data_set_as_it_is(ds_tiny2r):
    """(a) tiny2r's 1 200 pairs of 2 x 150"""
    ds, P = ds_tiny2r, cl.default_params()
    hp = cl.HotPath(P)
    hp.load_contig(0, ds.hi.views[0], ds.hi.annots[0])
    hp.upload(ds.batch)
    a1, b1, c1, S = hp.seeds(0)
    assert S == 7
    b0, c0 = _compare((a1, b1, c1), _oracle(ds, P, ds.batch, S), np.ones(ds.batch.n, np.uint8), S)
    assert (c0 > 0).sum() > 1000
    hp.close()


@pytest.mark.parametrize("k", [20, 14, 22])
def test_mixed_lengths_alignments_and_retired_pairs(ds_by_k, k):
    """(b) / (c) 512 pairs of mixed lengths (seed_words_util.mixed_batch), all active and again in the next slot after a round has
    retired some of them; then the counters of a profiled round over the pairs still active: probes counted from the lengths,
    retained hits from the oracle's counts, binary-search touches from the host emulation of cmc::seed_probe."""
    ds = ds_by_k(k)
    P = cl.default_params(kmer=k)
    whole = op.seeds(P, ds.ohi.views[0], ds.batch, 150 // k)[1].reshape(ds.batch.n, 2, 2, 150 // k)      # (pair, mate, orientation, s)
    first = [np.nonzero(whole[:, m, 0, 0] > 0)[0][0] for m in (0, 1)]                  # reads whose first seed hits as stored, and
    last = [np.nonzero(whole[:, m, 0, 2] > 0)[0][-1] for m in (0, 1)]                  # whose third does: the two ends of either buffer
    batch, l1, l2 = mixed_batch(ds.d, k, (*first, *last))
    hp = cl.HotPath(P)
    for slot in (0, 1):                                     # the same contig twice: "the next round" sees the same index
        hp.load_contig(slot, ds.hi.views[0], ds.hi.annots[0])
    hp.upload(batch)
    a1, b1, c1, S = hp.seeds(0)
    assert S == 150 // k
    want = _oracle(ds, P, batch, S)
    b0, c0 = _compare((a1, b1, c1), want, np.ones(batch.n, np.uint8), S)
    by = b0.reshape(batch.n, 2, 2, S)
    assert (c0 > 0).sum() > 200 and (by[0, :, 0, 0] > 0).all() and (by[-1, :, 0, 2] > 0).all()      # the k-mers next to the slack are found
    hp.map_round(0, False)
    act = hp.download()[2].copy()
    assert 0 < (act == 0).sum() < batch.n, "the batch must hold retired and active pairs"
    a2, b2, c2, _ = hp.seeds(1)
    b0, c0 = _compare((a2, b2, c2), want, act, S)
    # the counters of one more round, over the pairs still active
    hp.prof(True)
    hp.prof_reset()
    hp.map_rounds([1], True)
    hp.sync()
    cnt = hp.prof_get()[2]
    lens = np.stack([l1, l1, l2, l2], axis=1)               # (pair, mate x orientation)
    probes = ((np.arange(1, S + 1)[None, None, :] * k <= lens[:, :, None]) & (act != 0)[:, None, None]).sum()
    E = load_emu_seed()
    x, y, z = (np.zeros(batch.n * 4 * S, np.uint32) for _ in range(3))
    sums = np.zeros(3, np.uint64)
    assert E.seedw_seed_batch(C.byref(P), C.byref(ds.hi.views[0]), C.byref(batch.c), S, 1, act.ctypes.data, x.ctypes.data, y.ctypes.data, z.ctypes.data,
                              sums.ctypes.data) == 0
    assert (y == b0).all() and (z == c0).all()
    print(f"k {k}: retired {(act == 0).sum()} of {batch.n}; probes {cnt[0]} / {probes}, touches {cnt[1]} / {sums[1]}, hits {cnt[2]} / {b0.sum()}")
    assert cnt[0] == probes == sums[0]
    assert cnt[2] == b0.sum() == sums[2]
    assert cnt[1] == sums[1]
    hp.close()
