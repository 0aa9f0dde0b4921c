"""How much of the chain stage works for nobody: the chaining problems of active pairs whose other mate has no retained hit in
either orientation (the pair is settled as OEANCH without a look at a chain; cm_hot.hip quad_dead, NOTES 67).  Counted on the CPU,
round by round, from the oracle's seeds (oracle_seed_batch) and the oracle's flags (oracle_map_round); no device is used.
A problem is heavy when w > 256 or cells > 96, as in k_chain_cls.

usage: dead_chains.py [--preset hg38like] [--scale 20] [--pairs 40000] [--seed 38] [--threads 16]
--scale N (dense presets only): chromosome lengths / N; the `dup` families scaled in number only (per-contig copy numbers stay the
real ones), the `alu` copy numbers scaled with the genome (their per-contig count must still exceed seedLim: checked)."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from circminer_amd import lib as cl, synth  # noqa: E402
from oracle import oracle_py as op  # noqa: E402

LIGHT_W, LIGHT_CELLS = 256, 96


def workload(preset, scale, pairs, seed):
    if scale == 1 or preset not in synth.DENSE:
        assert scale == 1, "only the dense presets scale"
        return synth.generate(preset, n_pairs=pairs, seed=seed)
    lens, gpm, cs, _ = synth.PRESETS[preset]
    lens = [L // scale for L in lens]
    tiers = []
    for t in synth.DENSE_TIERS:
        t = dict(t)
        if t["name"] == "dup":
            t["families"] = max(1, t["families"] // scale)
        else:
            t["copies"] = tuple(max(2, c // scale) for c in t["copies"])
        tiers.append(t)
    rng = np.random.default_rng(seed)
    names = [f"chr{i + 1}" for i in range(len(lens))]
    seqs = synth.make_genome_tiers(rng, lens, tiers)
    contigs, table = synth.pack_genome(names, seqs, cs // scale)
    alu = [t for t in tiers if t["name"] == "alu"][0]
    assert alu["copies"][0] // len(contigs) > cl.default_params().seed_lim, "the alu families no longer exceed seedLim per contig"
    genes = synth.make_genes(rng, lens, genes_per_mbp=gpm, spread=True)
    s1, s2, src, tc, lo, hi = synth.make_reads(rng, seqs, genes, pairs)
    return synth.SynthData(names, seqs, contigs, table, genes, synth.gtf_text(genes, names), s1, s2, src, tc, lo, hi)


def dead_problems(cnt, S, active):
    """(dead, heavy, cells, w) per problem r = (pair * 2 + mate) * 2 + orientation, from the retained-hit counts per seed"""
    cnt = cnt.reshape(-1, S).astype(np.int64)
    cells = cnt.sum(1)
    later = np.cumsum(cnt[:, ::-1], 1)[:, ::-1] - cnt
    w = (cnt * later).sum(1)
    mate = cells.reshape(-1, 2).sum(1)
    other = mate.reshape(-1, 2)[:, ::-1].reshape(-1)
    act4 = np.repeat(active != 0, 4)
    dead = (cells > 0) & np.repeat(other == 0, 2) & act4
    heavy = (cells > 0) & ((w > LIGHT_W) | (cells > LIGHT_CELLS)) & act4
    return dead, heavy, cells, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="hg38like")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=40000)
    ap.add_argument("--seed", type=int, default=38)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    op.build()
    d = workload(a.preset, a.scale, a.pairs, a.seed)
    with tempfile.TemporaryDirectory() as td:
        gtf = os.path.join(td, "a.gtf")
        with open(gtf, "w") as f:
            f.write(d.gtf_text)
        hi = cl.HostIndex(d.contigs, d.chr_table, gtf, kmer=20, n_threads=a.threads)
    P = cl.default_params()
    batch = cl.ReadBatch(d.seq1, d.seq2)
    S = batch.max_len() // P.kmer
    n = batch.n
    st, act = op.default_state(P, n)
    print(f"{a.preset} / {a.scale}: {hi.n_contigs} contigs of {[len(c) for c in d.contigs]} bp, {n} pairs, seed {a.seed}")
    print("| round | active pairs | neither mate has hits | one mate has hits | heavy problems (dead) | dead share of heavy w / cells | light problems (dead) |")
    print("|---|---|---|---|---|---|---|")
    tot_dead = tot_chained = tot_active = 0
    for ci in range(hi.n_contigs):
        _, cnt, _ = op.seeds(P, hi.views[ci], batch, S)
        dead, heavy, cells, w = dead_problems(cnt, S, act)
        live = (cells > 0) & np.repeat(act != 0, 4)
        light = live & ~heavy
        mate = (cells.reshape(-1, 2).sum(1) > 0).reshape(-1, 2)
        on = act != 0
        neither, one = int((on & ~mate[:, 0] & ~mate[:, 1]).sum()), int((on & (mate[:, 0] != mate[:, 1])).sum())
        hw, hc = w[heavy].sum(), cells[heavy].sum()
        dh, dl = dead & heavy, dead & light
        print(f"| {ci} | {int(on.sum())} | {neither} | {one} | {int(heavy.sum())} ({int(dh.sum())} = {100 * dh.sum() / max(heavy.sum(), 1):.0f} %) | "
              f"{100 * w[dh].sum() / max(hw, 1):.1f} % / {100 * cells[dh].sum() / max(hc, 1):.1f} % | "
              f"{int(light.sum())} ({int(dl.sum())} = {100 * dl.sum() / max(light.sum(), 1):.0f} %) |")
        tot_dead += int(dead.sum())
        tot_chained += int(live.sum())
        tot_active += int(on.sum())
        cat = np.full(n, -1, np.int32)

        def work(p0, p1):
            rc = op.load().oracle_map_round(C.byref(P), C.byref(hi.views[ci]), C.byref(hi.annots[ci]), C.byref(batch.c),
                                            int(ci == hi.n_contigs - 1), st.ctypes.data, act.ctypes.data, cat.ctypes.data, p0, p1)
            assert rc == 0, rc

        T = max(1, a.threads)
        th = [threading.Thread(target=work, args=((n * i) // T, (n * (i + 1)) // T)) for i in range(T)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert (cat[dead.reshape(-1, 4).any(1)] == cl.CAT["OEANCH"]).all()        # every pair of a dead problem was settled as OEANCH
    print(f"all rounds: {tot_dead} dead of {tot_chained} problems with hits = {100 * tot_dead / max(tot_chained, 1):.2f} %; "
          f"{tot_dead / max(tot_active, 1):.4f} dead problems per active pair and round")


if __name__ == "__main__":
    main()
