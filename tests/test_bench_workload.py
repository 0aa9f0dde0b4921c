"""bench.py's own generator of its inputs (class Workload: synth.generate()'s specification on several host threads, written
straight into the caller's buffers) against synth.make_reads on the same genome, judged by what the oracle makes of the reads."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from circminer_amd import lib as cl, synth  # noqa: E402

N = 20000


def _make(seed=38, n_batches=3):
    import bench
    w = bench.Workload("small", N, seed, n_batches, 0, 4)
    w.start()
    bufs = [(np.empty((N, bench.READ_LEN), np.uint8), np.empty((N, bench.READ_LEN), np.uint8)) for _ in range(n_batches)]
    w.set_buffers(bufs)
    w.wait(w.genome_ready)
    w.wait(w.reads_ready)
    for f in w.reads:
        f.result()
    w.pool.shutdown()
    return w, bufs


def test_inputs_are_a_function_of_the_arguments_and_batches_differ():
    w1, b1 = _make()
    w2, b2 = _make()
    assert all((x == y).all() for x, y in zip(w1.contigs, w2.contigs)) and w1.gtf_text == w2.gtf_text
    assert all((p[0] == q[0]).all() and (p[1] == q[1]).all() for p, q in zip(b1, b2))
    assert (b1[0][0] != b1[1][0]).mean() > 0.5 and (b1[1][0] != b1[2][0]).mean() > 0.5
    w3, b3 = _make(seed=39, n_batches=1)
    assert (b3[0][0] != b1[0][0]).mean() > 0.5
    for w in (w1, w2, w3):
        w.tmp.cleanup()


def test_reads_map_like_the_generators(built):
    """Same genome and genes, reads from synth.make_reads and from bench.make_reads_fast: the oracle's classes of the pairs have
    the same shares.  A share p of N = 20000 pairs has a standard deviation of sqrt(p (1 - p) / N) <= 0.0036; two independent
    samples differ by less than 6 x sqrt(2) x that = 0.03 unless the generators differ.  Mean edit distance of the concordant
    pairs' first mates (0.4 % substitutions over 150 bases = 0.6 expected): within 0.05."""
    from oracle import oracle_py as op
    w, bufs = _make(n_batches=2)
    ref = synth.make_reads(np.random.default_rng(5), w.chr_seqs, w.genes, N)[:2]
    hi = cl.HostIndex(w.contigs, w.chr_table, w.gtf, kmer=20)
    P = cl.default_params()

    def shares(s1, s2):
        st, act, _ = op.map_all_rounds(P, hi, cl.ReadBatch(s1, s2))
        t = st["type"].astype(np.int64)
        return np.bincount(t + 1, minlength=16)[:16] / N, act.mean(), float(st["ed_r1"][t == 0].mean())
    want, want_act, want_ed = shares(*ref)
    for s1, s2 in bufs:
        assert s1.shape == (N, 150) and np.isin(s1, np.frombuffer(b"ACGTN", np.uint8)).all()
        got, got_act, got_ed = shares(s1, s2)
        assert np.abs(got - want).max() < 0.03, (got, want)
        assert abs(got_act - want_act) < 0.03 and got_act > 0.02
        assert abs(got_ed - want_ed) < 0.05
    w.tmp.cleanup()


def test_dense_genome_is_made_in_place_in_synths_packing():
    """The dense presets' chromosomes are written straight into the packed contigs: same contigs and table as synth.pack_genome
    makes of those chromosomes (two contigs here, Ns between neighbours), and the planted repeats are there (multi-hit 20-mers)."""
    import bench
    w = bench.Workload("hg38like", 1000, 7, 1, 0, 4, chr_lens=[300_000, 200_000, 250_000, 100_000], contig_size=520_000)
    w.start()
    w.wait(w.genome_ready)
    w.cancel()
    names = [t[0] for t in w.chr_table]
    contigs, table = synth.pack_genome(names, [np.array(s) for s in w.chr_seqs], 520_000)
    assert table == w.chr_table and len(contigs) == 2 and [len(c) for c in contigs] == [len(c) for c in w.contigs]
    assert all((a == b).all() for a, b in zip(contigs, w.contigs))
    assert np.isin(np.concatenate(w.chr_seqs), np.frombuffer(b"ACGTN", np.uint8)).all() and len(w.genes) > 5
