"""The launch counts cm_prof_get reports are part of what bench.py prints (its "kernels" object): every counted launch bumps
the count of its profile class where it is made (cm_hot.hip: launch(), counting_sort()).  One small batch through cm_map_rounds,
as one tile, as two and as three (the round-major walk), with the heavy-pair pipeline on, and two staged half batches one after the
other (the second one's first item prepared under the first one's last pair stage and taken over): the eight counts equal what the
kernel sequences of an earlier commit launched for the same calls (403b9cf for the first two lists, 11728b1 for the other two:
recorded by running this file's body against that commit's library, not derived from the code under test).
A kernel added to or dropped from a counted sequence moves a count and has to be entered here on purpose."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

# classes: seed, chain, pair, collect, heavy pairs, ordering, heavy chains, prefetched items taken over
# recorded on commit 403b9cf: this file's body against that commit's library (two items of one tile; four items of two tiles,
# two of whose pair stages launched the pipeline's fall-back kernel late: 74 = 4 x 18 + 2)
ONE_TILE = [2, 2, 2, 6, 38, 28, 2, 0]
TWO_TILES = [4, 4, 4, 12, 74, 56, 4, 0]
# recorded on commit 11728b1 in the same way (six items of three tiles; two half batches of one tile each, the second one's first
# item taken over: class 7)
THREE_TILES = [6, 6, 6, 18, 110, 84, 6, 0]
STAGED = [4, 4, 4, 12, 76, 56, 4, 1]


def _launch_counts(ds, staged=False):
    """ds_tiny2r (1 200 pairs, two contigs) through both slots in one call, profiling on -> the eight launch counts
    staged: its two halves as batches A and B -- stage A, swap, stage B, map_rounds, swap, map_rounds -> the counts of both calls"""
    from circminer_amd import lib as cl
    hp = cl.HotPath(cl.default_params(kmer=ds.kmer))
    try:
        for ci in range(ds.hi.n_contigs):
            hp.load_contig(ci, ds.hi.views[ci], ds.hi.annots[ci])
        hp.prof(True)
        slots = list(range(ds.hi.n_contigs))
        if staged:
            h = ds.batch.n // 2
            hp.stage(hp.pinned_batch(ds.d.seq1[:h], ds.d.seq2[:h]))
            hp.swap()
            hp.stage(hp.pinned_batch(ds.d.seq1[h:2 * h], ds.d.seq2[h:2 * h]))
            hp.prof_reset()
            hp.map_rounds(slots)
            hp.swap()
        else:
            hp.upload(ds.batch)
            hp.prof_reset()
        hp.map_rounds(slots)
        hp.sync()
        return [int(x) for x in hp.prof_get()[1]]
    finally:
        hp.close()


def test_launch_counts_one_tile(ds_tiny2r, monkeypatch):
    monkeypatch.delenv("CM_TILE_PAIRS", raising=False)
    got = _launch_counts(ds_tiny2r)
    print("launches, one tile:", got, flush=True)
    assert got == ONE_TILE


def test_launch_counts_staged_take_over(ds_tiny2r, monkeypatch):
    monkeypatch.delenv("CM_TILE_PAIRS", raising=False)
    got = _launch_counts(ds_tiny2r, staged=True)
    print("launches, two staged batches:", got, flush=True)
    assert got == STAGED


def _child_counts(tile):
    """a child process of its own (the knobs are read once per process) with CM_TILE_PAIRS = tile"""
    env = dict(os.environ, CM_TILE_PAIRS=tile)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_launch_counts_two_tiles():
    """CM_TILE_PAIRS = 600: two tiles, walked round-major"""
    got = _child_counts("600")
    print("launches, two tiles:", got, flush=True)
    assert got == TWO_TILES


def test_launch_counts_three_tiles():
    """CM_TILE_PAIRS = 400: three tiles (the seeding ahead of an item waits for flags that are final already, not for pair kernels)"""
    got = _child_counts("400")
    print("launches, three tiles:", got, flush=True)
    assert got == THREE_TILES


if __name__ == "__main__":      # the child: the same data set as the ds_tiny2r fixture, the same body
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest
    conftest._build.build()
    from oracle import oracle_py
    oracle_py.build()
    with tempfile.TemporaryDirectory() as td:
        print(json.dumps(_launch_counts(conftest.DataSet(td, "tiny2r", 1200, 22))))
