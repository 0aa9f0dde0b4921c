"""Data sets the session fixtures of conftest.py lack, and the per-attempt work counters of the host emulation; shared by the
CPU suite (test_hostemu_parity.py) and the GPU suites, which wrap them in module-level fixtures."""
import ctypes as C
import os

import numpy as np

from circminer_amd import lib as cl, synth
from conftest import DataSet

# The parameter sets that change the retirement rule of finish_round (cm_core.h): scan level 0 retires a concordant pair, 1 only a
# perfect genome-compatible one, 2 nothing before the last round.
SCHED_PARAMS = [{}, dict(scan_level=1), dict(scan_level=2, max_ed=8, seed_lim=1000)]
SCHED_IDS = ["default", "scan1", "scan2"]


def inverted_dup_dataset(tmpdir, n_pairs=1200, seed=22, kmer=20):
    """`tiny2r` with 40 kb of contig 0 overwritten by the reverse complement of another 40 kb of it, before any index is built.
    The generator's repeat families are same-strand copies, so on the stock presets the second orientation attempt of
    process_read (R2 forward, R1 reverse) never has chains on both reads; a read pair drawn from either copy of the inverted
    block has them in both orientations.  Pairs planted inside the overwritten block no longer map there."""
    d = synth.generate("tiny2r", n_pairs=n_pairs, seed=seed)
    c0 = d.contigs[0]
    assert len(c0) >= 110000 and c0.flags.writeable
    c0[70000:110000] = synth.revcomp(c0[10000:50000].copy())
    ds = DataSet.__new__(DataSet)                      # what DataSet.__init__ does, on the modified genome
    ds.d = d
    ds.gtf = os.path.join(str(tmpdir), f"invdup_{seed}.gtf")
    with open(ds.gtf, "w") as f:
        f.write(d.gtf_text)
    ds.hi = cl.HostIndex(d.contigs, d.chr_table, ds.gtf, kmer=kmer)
    ds.batch = cl.ReadBatch(d.seq1, d.seq2)
    ds.kmer = kmer
    from oracle import oracle_py
    ds.ohi = oracle_py.OracleIndex(d.contigs, d.chr_table, ds.gtf, kmer=kmer)
    return ds


def attempt_counts(E, ds, P, ci=0, is_last=False):
    """One round of the host emulation on contig `ci` from fresh states.  Per pair: mate-pair tasks of the first attempt and of the
    second, unpaired-chain extensions of the first attempt and of the second (cm_stats [0], [2] less [16], [17]; [16], [17]), and the
    active flag after the round: (t0, t1, u0, u1, active)."""
    n = ds.batch.n
    E.emu_set_stats_out.argtypes = [C.c_void_p]
    W = E.emu_stats_width()
    assert W >= 18
    stats = np.zeros((n, W), np.uint64)
    from oracle import oracle_py as op
    st, act = op.default_state(P, n)
    cat = np.full(n, -1, np.int32)
    E.emu_set_stats_out(stats.ctypes.data)
    try:
        rc = E.emu_map_round(C.byref(P), C.byref(ds.hi.views[ci]), C.byref(ds.hi.annots[ci]), C.byref(ds.batch.c), int(is_last), st.ctypes.data,
                             act.ctypes.data, cat.ctypes.data)
    finally:
        E.emu_set_stats_out(None)
    assert rc == 0
    s = stats.astype(np.int64)
    return s[:, 0] - s[:, 16], s[:, 16], s[:, 2] - s[:, 17], s[:, 17], act


def block_and_unique_pairs(ds, n_each=800, seed=1):
    """Read pairs for inverted_dup_dataset's contig 0 with one mate inside a copy of the duplicated block and the other in unique
    sequence between the copies, 150 bp each, in four strand / copy combinations.  About one in a hundred of them has no
    unpaired-chain extension in the first orientation attempt and one or two in the second (the mirror case of the pairs that
    have more mate-pair tasks there); found by a search with attempt_counts over such constructions."""
    c0 = ds.d.contigs[0]
    rng = np.random.default_rng(seed)
    ar = np.arange(150)
    src = rng.integers(10000, 49800, n_each)
    dup = rng.integers(70000, 109800, n_each)
    out = rng.integers(52000, 68000, n_each)
    s1, s2 = [], []
    for blk, rc1, rc2 in ((src, 0, 0), (src, 1, 1), (dup, 0, 1), (dup, 1, 0)):
        a, b = c0[blk[:, None] + ar], c0[out[:, None] + ar]
        s1.append(synth.revcomp(a) if rc1 else a)
        s2.append(synth.revcomp(b) if rc2 else b)
    return cl.ReadBatch(np.concatenate(s1), np.concatenate(s2))
