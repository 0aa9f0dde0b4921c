"""The annotation look-ups of cm_core.h ON THE DEVICE, request by request, against the oracle (bit-exact on every result field and
every kept transcript id): cm_annot_batch runs the requests of annot_requests_util.py -- the ones test_annot_requests_cpu.py proves
against the oracle and a brute force through the host emulation -- over what only the device has: the AoS records, the bucket
table and the pair_reach that cm_load_annotation put into the slot, read through to_core() with the qualified pointers of the
real kernels, 64 different look-ups per wave.

Each GTF-built annotation is asked twice on one slot: as loaded (with the product's bucket table), one launch per kind, so that every
wave holds one kind; then reloaded without the table, kinds interleaved lane by lane.  The numpy-built views are asked once, as they
are, interleaved.  Two annotations go through the library's second kernel build as well, interleaved.  The cross is partial on
purpose (the module stays well under a million requests): one kind per wave is asked with the product's table only, and
interleaved lanes with a table only on the numpy-built views and in the second build.  Nothing is loaded but the annotation: no index, no
reads.  A failing request prints itself with the three answers there are for it."""
import ctypes as C

import numpy as np
import pytest

from circminer_amd import lib as cl
import annot_requests_util as aq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp():
    h = cl.HotPath(cl.default_params())
    yield h
    h.close()


@pytest.fixture(scope="module")
def hp24():
    """the build for reads of more than 16 seeds (cm_dispatch.cpp): its own loader, its own slots"""
    h = cl.HotPath(cl.default_params(kmer=14, max_read_len=300))
    yield h
    h.close()


def _without_table(av):
    v = cl.AnnotView()
    C.memmove(C.byref(v), C.byref(av), C.sizeof(cl.AnnotView))
    v.iv_bucket, v.iv_bucket_shift, v.n_iv_bucket = None, 0, 0
    return v


def _interleaved(q):
    """a permutation that puts the kinds next to each other, lane by lane: request i of kind k before request i + 1 of any kind"""
    rank = np.zeros(len(q), np.int64)
    for k in np.unique(q["kind"]):
        m = q["kind"] == k
        rank[m] = np.arange(m.sum())
    return np.lexsort((q["kind"], rank))


def _ask(h, slot, b, interleave):
    for part, (P, q, _, _) in enumerate(b.parts):
        if interleave:
            order = _interleaved(q)
            got, tids = h.annot_batch(slot, P, q[order])
        else:                                                                    # a launch per kind: every wave holds one kind
            order = None
            got, tids = np.zeros(len(q), aq.RES), np.zeros((len(q), aq.TIDS), np.uint32)
            for k in np.unique(q["kind"]):
                idx = np.flatnonzero(q["kind"] == k)
                got[idx], tids[idx] = h.annot_batch(slot, P, q[idx])
        bad = b.mismatch(part, got, tids, order)
        assert bad is None, ("kinds interleaved\n" if interleave else "one kind per wave\n") + bad


@pytest.mark.parametrize("name", tuple(aq.GTF_SETS) + aq.PRESET_VIEWS)
def test_lookups_equal_oracle_with_and_without_the_table(hp, name):
    b = aq.batch(name)
    assert b.A.av.iv_bucket and b.A.av.n_iv_bucket >= 2
    hp.load_annotation(1, b.A.av)
    _ask(hp, 1, b, interleave=False)
    hp.load_annotation(1, _without_table(b.A.av))                               # the same slot, reloaded: the plain search
    _ask(hp, 1, b, interleave=True)


@pytest.mark.parametrize("name", aq.NUMPY_VIEWS)
def test_lookups_equal_oracle_on_numpy_built_views(hp, name):
    """no table, shifts 6 and 14, no slack bucket, one interval, intervals without segments, and (np-nbits) bitsets whose last
    word is a partial one: cm_load_annotation uploads ceil(n_bits / 64) words"""
    b = aq.batch(name)
    hp.load_annotation(2, b.A.av)
    _ask(hp, 2, b, interleave=True)


@pytest.mark.parametrize("name", aq.WIDE_ANNOTS)
def test_lookups_equal_oracle_in_the_second_kernel_build(hp24, name):
    b = aq.batch(name)
    hp24.load_annotation(0, b.A.av)
    _ask(hp24, 0, b, interleave=True)


def test_hook_refuses_what_it_cannot_run(hp):
    b = aq.batch("twochr")
    P, q = b.parts[0][0], b.parts[0][1]
    with pytest.raises(RuntimeError, match="annotation of slot 5 not loaded"):
        hp.annot_batch(5, P, q[:64])
    hp.load_annotation(3, b.A.av)

    def one(kind, **kw):
        return aq._mk(kind, kw.pop("p0", 0), **kw)

    for bad in (one(12), one(-1), one(3, p0=100, p1=0), one(4, p0=10, p1=50, i0=b.A.n_iv, i1=20, i2=20), one(7, i0=-1), one(8, i0=0, i1=b.A.n_iv),
                one(9, i0=-2, i1=0), one(10, p0=101, p2=100)):
        with pytest.raises(RuntimeError, match="cm_annot_batch"):
            hp.annot_batch(3, P, np.concatenate([q[:70], bad, q[70:90]]))
    with pytest.raises(RuntimeError, match="slot"):
        hp.annot_batch(99, P, q[:64])
    assert len(hp.annot_batch(3, P, q[:0])[0]) == 0
    v, keep = aq.view_of(b.A.a, aq.bucket_table(b.A.a, 10, b.A.n_bucket), 0)        # loads, but its `b + 1` wraps: not asked
    hp.load_annotation(3, v)
    with pytest.raises(RuntimeError, match="iv_bucket_shift 0"):
        hp.annot_batch(3, P, q[:64])
    hp.load_annotation(3, b.A.av)
    _ask(hp, 3, b, interleave=False)                                             # the context is as good as before
