"""The round pipeline does not chain a problem whose chains nobody reads: it has retained hits, the other mate of its pair has
none in either orientation (process_read settles the pair as OEANCH from "has this mate a chain" alone; cm_hot.hip quad_dead).
States, flags and categories must equal the oracle's byte for byte on data full of such problems, on every path of the chain stage;
word 7 of cm_debug_counters must equal the number of such problems counted from the oracle's seeds; the test hooks (cm_seed_batch,
cm_chain_batch) still chain everything.

Data: two packed contigs of 0.4 Mbp with the genes of the `tiny2r` preset, two repeat families of 240 copies planted in each at
known places, a 16-kbp tandem repeat (every 20-mer beyond seedLim) in contig 1, and pairs built for the purpose:
  (a) one mate inside a repeat copy, the other random bases, both ways round  -> dead heavy problems
  (b) one mate a unique read of contig 1, the other random                    -> dead light problems
  (c) both mates inside one copy                                              -> live heavy problems
  (d) the preset's own transcriptomic / genomic / back-splice pairs
  (e) one mate from the tandem repeat (high_hits > 0, no retained hit) beside a mate with hits -> dead, and `high` must survive;
      both mates from it -> NOPROC_MANYHIT
  (f) a mate with an N in every seed, a mate shorter than k, beside a mate with hits
  (g) both mates random                                                       -> NOPROC_NOMATCH
  and (a), (c) again from contig 2: no hit at all in round 1, dead / live in round 2."""
import ctypes as C
import os

import numpy as np
import pytest

from circminer_amd import lib as cl, synth
from oracle import oracle_py as op
from conftest import first_diff

CHR_LEN = 400_000
SEED = 67
N_SYNTH = 1400
FAM_LEN, FAM_COPIES, N_FAM, FAM_DIV = 300, 240, 2, 0.03
GRID0, GRID = 20_000, 400                     # a copy or a unique read per 400-bp cell from GRID0 on; the tandem repeat lies before
TANDEM0, TANDEM_UNIT, TANDEM_N = 2_000, 23, 700
RL = 150
LIGHT_W, LIGHT_CELLS = 256, 96                # cm_hot.hip chain_light_w() / chain_light_cells()
_ACGT = np.frombuffer(b"ACGT", np.uint8)


class _Data:
    pass


def _plant(rng, contig, fams):
    """240 copies of every family into distinct cells of the grid; returns the copies' starts and the starts of cells left free"""
    n_cells = (len(contig) - GRID0 - 2000) // GRID
    cells = rng.permutation(n_cells)
    used = cells[:N_FAM * FAM_COPIES]
    for i, c in enumerate(used):
        copy = fams[i % N_FAM].copy()
        m = rng.random(FAM_LEN) < FAM_DIV
        copy[m] = _ACGT[rng.integers(0, 4, int(m.sum()))]
        p = GRID0 + int(c) * GRID
        contig[p:p + FAM_LEN] = copy
    return GRID0 + used.astype(np.int64) * GRID, GRID0 + cells[N_FAM * FAM_COPIES:].astype(np.int64) * GRID


@pytest.fixture(scope="module")
def ds_dead(tmp_path_factory, built):
    tmp = tmp_path_factory.mktemp("dead")
    d = synth.generate("tiny2r", n_pairs=N_SYNTH, seed=SEED, chr_lens=[CHR_LEN, CHR_LEN], contig_size=CHR_LEN + 50_000)
    assert len(d.contigs) == 2
    rng = np.random.default_rng(SEED + 1)
    fams = [_ACGT[rng.integers(0, 4, FAM_LEN)] for _ in range(N_FAM)]
    c1, c2 = d.contigs
    unit = _ACGT[rng.integers(0, 4, TANDEM_UNIT)]
    c1[TANDEM0:TANDEM0 + TANDEM_UNIT * TANDEM_N] = np.tile(unit, TANDEM_N)
    copies1, free1 = _plant(rng, c1, fams)
    copies2, _ = _plant(rng, c2, fams)

    def rand():
        return _ACGT[rng.integers(0, 4, RL)]

    def in_copy(contig, copies, second=False):
        p = int(copies[rng.integers(0, len(copies))])
        r = contig[p + RL:p + 2 * RL] if second else contig[p:p + RL]
        return synth.revcomp(r) if second else r.copy()

    def pair_in_copy(contig, copies):
        p = int(copies[rng.integers(0, len(copies))])
        return contig[p:p + RL].copy(), synth.revcomp(contig[p + RL:p + 2 * RL])

    def unique():
        p = int(free1[rng.integers(0, len(free1))]) + 100
        return c1[p:p + RL].copy()

    def tandem():
        p = TANDEM0 + int(rng.integers(0, TANDEM_UNIT * (TANDEM_N - 10)))
        return c1[p:p + RL].copy()

    def with_hits(i):
        return in_copy(c1, copies1) if i % 2 else unique()

    def n_in_every_seed(r):
        r = r.copy()
        r[10::20] = ord("N")
        return r

    pairs = [(d.seq1[i], d.seq2[i]) for i in range(N_SYNTH)]                       # (d)
    pairs += [(in_copy(c1, copies1), rand()) for _ in range(300)]                  # (a)
    pairs += [(rand(), in_copy(c1, copies1, second=True)) for _ in range(300)]
    pairs += [(unique(), rand()) if i % 2 else (rand(), synth.revcomp(unique())) for i in range(300)]      # (b)
    pairs += [pair_in_copy(c1, copies1) for _ in range(300)]                       # (c)
    pairs += [(tandem(), with_hits(i)) if i % 4 < 2 else (with_hits(i), tandem()) for i in range(120)]     # (e)
    pairs += [(tandem(), synth.revcomp(tandem())) for _ in range(40)]
    pairs += [(n_in_every_seed(unique()), with_hits(i)) for i in range(30)]        # (f)
    pairs += [(with_hits(i), unique()[:12]) for i in range(30)]
    pairs += [(rand(), rand()) for _ in range(100)]                                # (g)
    pairs += [(in_copy(c2, copies2), rand()) for _ in range(100)]                  # contig 2
    pairs += [pair_in_copy(c2, copies2) for _ in range(100)]
    order = rng.permutation(len(pairs))                                            # every tile gets every kind
    pairs = [pairs[i] for i in order]
    ds = _Data()
    ds.d, ds.kmer = d, 20
    ds.gtf = os.path.join(str(tmp), "dead.gtf")
    with open(ds.gtf, "w") as f:
        f.write(d.gtf_text)
    ds.hi = cl.HostIndex(d.contigs, d.chr_table, ds.gtf, kmer=ds.kmer)
    ds.ohi = op.OracleIndex(d.contigs, d.chr_table, ds.gtf, kmer=ds.kmer)
    ds.batch = cl.ReadBatch(np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs]),
                            np.array([len(a) for a, _ in pairs]), np.array([len(b) for _, b in pairs]))
    ds.order = order
    return ds


def dead_problems(cnt, S, active=None):
    """the rule on the oracle's seed counts: (dead, heavy) per problem; cells(r) > 0 and the pair's other mate has no cell"""
    cnt = cnt.reshape(-1, S).astype(np.int64)
    cells = cnt.sum(1)
    later = np.cumsum(cnt[:, ::-1], 1)[:, ::-1] - cnt
    w = (cnt * later).sum(1)
    mate = cells.reshape(-1, 2).sum(1)                       # per (pair, mate)
    other = mate.reshape(-1, 2)[:, ::-1].reshape(-1)
    dead = (cells > 0) & np.repeat(other == 0, 2)
    if active is not None:
        dead &= np.repeat(active != 0, 4)
    return dead, (cells > 0) & ((w > LIGHT_W) | (cells > LIGHT_CELLS)), cells


def _want(ds, P):
    """the oracle's side, computed once per parameter set: per-round states, the final ones, seeds and chains of contig 1"""
    b = ds.batch
    S = b.max_len() // P.kmer
    w = dict(S=S, rounds=[])
    st, act = op.default_state(P, b.n)
    for ci in range(2):
        cat = op.map_round(P, ds.ohi.views[ci], ds.ohi.annots[ci], b, ci == 1, st, act)
        w["rounds"].append((st.copy(), act.copy(), cat.copy()))
    fin = op.map_all_rounds(P, ds.ohi, b)
    assert fin[0].tobytes() == st.tobytes() and (fin[1] == act).all() and (fin[2][1] == w["rounds"][1][2]).all()
    w["seeds"] = op.seeds(P, ds.ohi.views[0], b, S)
    return w


@pytest.fixture(scope="module")
def want(ds_dead):
    ds = ds_dead
    P = cl.default_params(kmer=ds.kmer)
    w = _want(ds, P)
    w["chains"] = op.chains(P, ds.ohi.views[0], ds.ohi.annots[0], ds.batch)
    # ---- preconditions, from the oracle alone
    _, cnt, raw = w["seeds"]
    S = w["S"]
    dead, heavy, cells = dead_problems(cnt, S)
    n_dead_heavy, n_dead_light, n_live_heavy = int((dead & heavy).sum()), int((dead & ~heavy).sum()), int((~dead & heavy).sum())
    # (e): the other mate of a dead problem has high_hits > 0
    hh = ((raw.reshape(-1, S) > 0) & (cnt.reshape(-1, S) == 0)).sum(1)
    mate_hh = hh.reshape(-1, 2).sum(1)
    other_hh = np.repeat(mate_hh.reshape(-1, 2)[:, ::-1].reshape(-1), 2)
    n_e = int(np.unique(np.nonzero(dead & (other_hh > 0))[0] >> 2).size)
    cat0 = w["rounds"][0][2]
    print(f"dead heavy {n_dead_heavy}, dead light {n_dead_light}, live heavy {n_live_heavy}, pairs of kind (e) {n_e}, "
          f"round-1 categories {np.bincount(cat0[cat0 >= 0], minlength=14).tolist()}")
    assert n_dead_heavy >= 200 and n_dead_light >= 200, (n_dead_heavy, n_dead_light)
    assert n_e >= 50, n_e
    assert n_live_heavy >= 200, n_live_heavy
    for name in ("NOPROC_MANYHIT", "NOPROC_NOMATCH", "OEANCH"):
        assert (cat0 == cl.CAT[name]).sum() >= 10, name
    # the rule's premise on this data: a problem has a chain exactly when it has a retained hit; high_hits as counted above
    assert ((w["chains"][1] > 0) == (cells > 0)).all() and (w["chains"][2] == hh).all()
    # round 2 has dead problems too (its classes are made while round 1's pair stage reads the other chain records)
    _, cnt2, _ = op.seeds(P, ds.ohi.views[1], ds.batch, S)
    assert int(dead_problems(cnt2, S, w["rounds"][0][1])[0].sum()) >= 100
    w["n_dead"] = int(dead.sum())
    return w


def _ctx(ds, P):
    hp = cl.HotPath(P)
    for ci in range(2):
        hp.load_contig(ci, ds.hi.views[ci], ds.hi.annots[ci])
    return hp


def _equal(got, ref, what=""):
    (st1, cat1, act1), (st0, act0, cat0) = got, ref
    assert (cat0 == cat1).all(), (what, np.nonzero(cat0 != cat1)[0][:10])
    assert (act0 == act1).all(), what
    assert st0.tobytes() == st1.tobytes(), (what, first_diff(st0, st1))


def _counters(hp):
    raw = (C.c_ulonglong * 32)()
    hp._chk(hp.L.cm_debug_counters(hp.h, raw), "cm_debug_counters")
    return list(raw)


def _all_paths(ds, w, P):
    """rounds in one call, twice on one context; after stage / swap of a second batch (its first item prefetched); round by round"""
    hp = _ctx(ds, P)
    final = w["rounds"][1]
    hp.upload(ds.batch)
    for rep in range(2):
        hp.reset()
        hp.map_rounds([0, 1], True)
        _equal(hp.download(), final, f"one call, pass {rep}")
    hp.reset()
    hp.stage(ds.batch)
    hp.map_rounds([0, 1], True)                       # prefetches the staged batch's first item
    _equal(hp.download(), final, "before the swap")
    before = hp.prof_get()[1][7]
    hp.swap()
    hp.map_rounds([0, 1], True)
    assert hp.prof_get()[1][7] == before + 1          # taken over from the prefetch
    _equal(hp.download(), final, "prefetched first item")
    hp.reset()
    for ci in range(2):
        hp.map_round(ci, ci == 1)
        _equal(hp.download(), w["rounds"][ci], f"round {ci} on its own")
    hp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [None, "512"])
def test_rounds_equal_the_oracle(ds_dead, want, monkeypatch, tile):
    """default tile: one item per round; 512-pair tiles: seven items per round in round-major order, every item but the first with
    classes made ahead into the seed set's scratch (k_chain_apply)"""
    if tile:
        monkeypatch.setenv("CM_TILE_PAIRS", tile)
    _all_paths(ds_dead, want, cl.default_params(kmer=ds_dead.kmer))


@pytest.mark.gpu
def test_counter_equals_the_oracles_count(ds_dead, want):
    """a fresh batch, one round on contig 1: every pair is active, so the flags are exact and word 7 is the count from the seeds"""
    ds = ds_dead
    hp = _ctx(ds, cl.default_params(kmer=ds.kmer))
    hp.upload(ds.batch)
    hp.prof_reset()
    assert _counters(hp)[7] == 0
    hp.map_round(0, False)
    hp.sync()
    assert _counters(hp)[7] == want["n_dead"], (_counters(hp)[7], want["n_dead"])
    hp.prof_reset()
    assert _counters(hp)[7] == 0
    hp.close()


def _chains_equal(got, ref):
    (c1, n1, h1), (c0, n0, h0) = got, ref
    assert (n0 == n1).all(), np.nonzero(n0 != n1)[0][:10]
    assert (h0 == h1).all()
    a, b = c0.reshape(-1, cl.CM_BESTCHAINLIM), c1.reshape(-1, cl.CM_BESTCHAINLIM)
    for r in np.nonzero(n0)[0]:
        x, y = a[r, :n0[r]], b[r, :n0[r]]
        assert (x["chain_len"] == y["chain_len"]).all() and (x["score"] == y["score"]).all(), r
        for k in range(n0[r]):
            L = int(x[k]["chain_len"])
            assert (x[k]["rpos"][:L] == y[k]["rpos"][:L]).all() and (x[k]["qpos"][:L] == y[k]["qpos"][:L]).all(), (r, k)


@pytest.mark.gpu
def test_hooks_still_chain_everything(ds_dead, want):
    """cm_seed_batch / cm_chain_batch, also right after a round of the pipeline on the same context: dead problems included"""
    ds = ds_dead
    P = cl.default_params(kmer=ds.kmer)
    hp = _ctx(ds, P)
    hp.upload(ds.batch)
    hp.map_round(0, False)
    hp.reset()
    a1, b1, c1, S = hp.seeds(0)
    a0, b0, c0 = want["seeds"]
    assert S == want["S"] and (c0 == c1).all() and (b0 == b1).all() and (a0[b0 > 0] == a1[b0 > 0]).all()
    _chains_equal(hp.chains(0), want["chains"])
    hp.map_rounds([0, 1], True)                       # and the pipeline after the hooks
    _equal(hp.download(), want["rounds"][1])
    hp.close()


@pytest.mark.gpu
def test_log_pool_retry_with_dead_problems(ds_dead, want, monkeypatch):
    """a 64-KB improvement log that may grow to 256 KB: the stage is redone with a larger pool, then in halves on the
    one-lane-per-problem kernel, which must leave the dead problems alone too"""
    monkeypatch.setenv("CM_POOL_BYTES", "65536")
    monkeypatch.setenv("CM_POOL_MAX", "262144")
    ds = ds_dead
    hp = _ctx(ds, cl.default_params(kmer=ds.kmer))
    hp.upload(ds.batch)
    hp.map_rounds([0, 1], True)
    _equal(hp.download(), want["rounds"][1])
    hp.reset()
    for ci in range(2):
        hp.map_round(ci, ci == 1)
        _equal(hp.download(), want["rounds"][ci], f"round {ci} on its own")
    hp.close()


@pytest.mark.gpu
def test_one_chain_per_problem(ds_dead):
    """max_chain_len = 1, the smallest the parameters admit: a retained hit still makes a chain, the rule still holds"""
    ds = ds_dead
    P = cl.default_params(kmer=ds.kmer, max_chain_len=1)
    w = _want(ds, P)
    hp = _ctx(ds, P)
    hp.upload(ds.batch)
    hp.map_rounds([0, 1], True)
    _equal(hp.download(), w["rounds"][1])
    hp.close()
