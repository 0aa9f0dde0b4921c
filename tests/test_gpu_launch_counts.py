"""The launch counts cm_prof_get reports are part of what bench.py prints (its "kernels" object): every counted launch bumps
the count of its profile class where it is made (cm_hot.hip: launch(), counting_sort()).  One small batch through cm_map_rounds,
as one tile and as two (the round-major walk), with the heavy-pair pipeline on: the eight counts equal what the kernel sequences
of commit 403b9cf launched for the same calls (recorded there by running this file's body, not derived from the code under test).
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


def _launch_counts(ds):
    """ds_tiny2r (1 200 pairs, two contigs) through both slots in one call, profiling on -> the eight launch counts"""
    from circminer_amd import lib as cl
    hp = cl.HotPath(cl.default_params(kmer=ds.kmer))
    try:
        for ci in range(ds.hi.n_contigs):
            hp.load_contig(ci, ds.hi.views[ci], ds.hi.annots[ci])
        hp.prof(True)
        hp.upload(ds.batch)
        hp.prof_reset()
        hp.map_rounds(list(range(ds.hi.n_contigs)))
        hp.sync()
        return [int(x) for x in hp.prof_get()[1]]
    finally:
        hp.close()


def test_launch_counts_one_tile(ds_tiny2r, monkeypatch):
    monkeypatch.delenv("CM_TILE_PAIRS", raising=False)
    got = _launch_counts(ds_tiny2r)
    print("launches, one tile:", got, flush=True)
    assert got == ONE_TILE


def test_launch_counts_two_tiles():
    """CM_TILE_PAIRS = 600: two tiles, walked round-major; a child process of its own (the knobs are read once per process)"""
    env = dict(os.environ, CM_TILE_PAIRS="600")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print("launches, two tiles:", got, flush=True)
    assert got == TWO_TILES


if __name__ == "__main__":      # the child: the same data set as the ds_tiny2r fixture, the same body
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest
    conftest._build.build()
    from oracle import oracle_py
    oracle_py.build()
    with tempfile.TemporaryDirectory() as td:
        print(json.dumps(_launch_counts(conftest.DataSet(td, "tiny2r", 1200, 22))))
