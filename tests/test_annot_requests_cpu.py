"""The annotation look-ups of cm_core.h asked directly, on the build box: the request generator of annot_requests_util.py, the
oracle (oracle_annot_batch: its own functions over the structure-of-arrays view, plain binary search, no quick reject), the host
build of cmc::annot_req_run (emu_annot_batch in tests/hostemu.cpp: AoS records, bucket table, pair_reach) and, for kinds 0, 1, 5
and 6, a linear scan in numpy, proven against each other before test_gpu_annot_queries.py sends the same requests to the device.
Bit-exact on every result field and every kept transcript id, no request left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from circminer_amd import lib as cl
import annot_requests_util as aq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu_annot(emu):
    emu.emu_annot_batch.restype = C.c_int
    emu.emu_annot_batch.argtypes = [C.POINTER(cl.Params), C.POINTER(cl.AnnotView), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    emu.emu_annot_pair_reach.restype = C.c_uint32
    emu.emu_annot_pair_reach.argtypes = [C.POINTER(cl.AnnotView)]

    def run(P, av, req, want_rc=0):
        req = np.ascontiguousarray(req, dtype=aq.REQ)
        out, tids = np.zeros(len(req), aq.RES), np.zeros((len(req), aq.TIDS), np.uint32)
        rc = emu.emu_annot_batch(C.byref(P), C.byref(av), req.ctypes.data, len(req), out.ctypes.data, tids.ctypes.data)
        assert rc == want_rc, rc
        return out, tids
    run.pair_reach = lambda av: int(emu.emu_annot_pair_reach(C.byref(av)))
    return run


@pytest.mark.parametrize("name", aq.ALL_ANNOTS)
def test_emulation_equals_oracle_equals_brute_force(emu_annot, name):
    b = aq.batch(name)
    assert len(b) > 0
    bad = b.brute_mismatch()
    assert bad is None, bad
    for part, (P, q, _, _) in enumerate(b.parts):
        bad = b.mismatch(part, *emu_annot(P, b.A.av, q))
        assert bad is None, bad


def test_batches_stay_small():
    """what test_gpu_annot_queries.py sends: every GTF-built batch twice, the numpy-built ones once, two of them through the
    second kernel build as well -- well under a million requests"""
    n = {name: len(aq.batch(name)) for name in aq.ALL_ANNOTS}
    sent = sum(v * (1 if k in aq.NUMPY_VIEWS else 2) for k, v in n.items()) + sum(n[k] for k in aq.WIDE_ANNOTS)
    print(n, sent)
    assert sent < 700_000


def test_annotations_are_what_they_are_meant_to_be():
    d = aq.annot("dense")
    spos, epos = d.a["iv_spos"].astype(np.int64), d.a["iv_epos"].astype(np.int64)
    assert 4096 in spos and 4095 in epos and spos[0] == 60
    ss, se = d.a["seg_start"].astype(np.int64), d.a["seg_end"].astype(np.int64)
    inb = (ss >> 10) == 5
    assert np.bincount(spos >> 10).max() >= 40 and inb.sum() >= 40 and ((se[inb] >> 10) == 5).all() and ((se - ss + 1)[inb] >= 8).all() and ((se - ss + 1)[inb] <= 30).all()
    assert epos.max() < 16384 - 3072 and d.a["n_bits"] % 64 == 0
    assert (d.nseg >= 3).any()                                                   # overlapping genes: intervals with several segments
    assert int(d.av.n_iv_bucket) == (d.a["n_bits"] >> 10) + 2 and int(d.av.iv_bucket_shift) == 10
    lg = aq.annot("long")
    assert aq.brute_pair_reach(lg) > aq.MAXDISCRDTLEN and lg.contig_len == 65536
    assert len(aq.annot("twochr").a["chr_shift"]) == 2
    assert not aq.annot("np-nobucket").av.iv_bucket
    ns = aq.annot("np-noslack")
    assert int(ns.av.n_iv_bucket) == ns.a["n_bits"] >> 10
    assert aq.annot("np-single").n_iv == 1 and (aq.annot("np-nseg0").nseg == 0).sum() >= 20
    assert aq.annot("np-nbits").a["n_bits"] == 16384 - 7 and len(aq.annot("np-nbits").a["near_border_bits"]) == 256
    for name in ("dense", "variety-0", "tiny2r-1"):                            # the two builders agree on what they build
        A = aq.annot(name)
        pa = aq.arrays_of(A.av)
        assert all(np.array_equal(pa[k], A.a[k]) for k in A.a if k != "n_bits") and pa["n_bits"] == A.a["n_bits"], name


def test_hook_refuses_what_it_cannot_run(emu_annot):
    """the checks cm_annot_batch makes before it launches (cmc::annot_req_check, shared with the emulation): CM_EINVAL"""
    A = aq.annot("dense")
    P = aq.params(4, 0)
    good = aq.batch("dense").parts[0][1]

    def one(kind, **kw):
        return aq._mk(kind, kw.pop("p0", 0), **kw)

    emu_annot(P, A.av, good[:64])
    for bad in (one(12), one(-1), one(2, p0=100, p1=0, p2=5), one(3, p0=100, p1=0, p2=5), one(4, p0=10, p1=50, i0=A.n_iv, i1=20, i2=20),
                one(7, i0=-1), one(7, i0=A.n_iv), one(8, i0=-1, i1=0), one(8, i0=0, i1=-1), one(8, i0=0, i1=A.n_iv), one(9, i0=-2, i1=0),
                one(9, i0=0, i1=A.n_iv), one(10, p0=101, p2=100)):
        emu_annot(P, A.av, bad, want_rc=-1)
        emu_annot(P, A.av, np.concatenate([good[:70], bad, good[70:90]]), want_rc=-1)
    for fine in (one(4, p0=10, p1=50, i0=-7, i1=20, i2=20), one(9, i0=-1, i1=-1), one(10, p0=100, p2=100), one(0, p0=0xFFFFFFFF), one(6, p0=0xFFFFFFFF),
                 one(2, p0=0xFFFFFFFF, p1=1, p2=1), one(11, p0=0x7FFFFFFF, p1=0x7FFFFFFF + 20, p2=0, p3=20, i0=13)):
        emu_annot(P, A.av, fine)
    assert len(emu_annot(P, A.av, good[:0])[0]) == 0
    for shift in (0, 32):                                                        # a table whose `b + 1` wraps, or whose shift is none
        v, keep = aq.view_of(A.a, aq.bucket_table(A.a, 10, A.n_bucket), shift)
        emu_annot(P, v, good[:64], want_rc=-1)
    v, keep = aq.view_of(A.a, aq.bucket_table(A.a, 31, 2), 31)
    bad = aq.batch("dense").mismatch(0, *emu_annot(P, v, good))
    assert bad is None, bad


# ---- the generator is not vacuous: counts of requests by what the ORACLE's answers and its view say they reach (nothing here looks at
# ---- the code under test).  Every batch has floors: at least 20 requests of each category its annotation and its kinds can
# ---- express.  What a batch is excused from, and why:
# ----   `find: hit with nseg == 0`: no GTF gives an interval without segments (np-nseg0 has them);
# ----   `kind 9 with more`: needs 65 transcripts in two intervals (the 70-isoform gene of dense, and the views made of dense that ask kind 9);
# ----   `kind 11 with d > MAXDISCRDTLEN, d <= pair_reach and a non-zero answer`: needs pair_reach > 20 000 (long);
# ----   `epos > iv.epos keeps some, drops others`: needs an interval whose segments end at different places (overlapping exons);
# ----   `kind 10 with a skipped zero state`: needs a transcript that skips an interval between two of its own (long has one such
# ----   transcript and four such requests; twochr and np-single have none);
# ----   np-single (one interval, one segment without a next exon): no gap, no max_next, no junction, no second gene;
# ----   the batches outside aq.FULL do not ask kinds 4 and 9.
FIND = ("find: miss before the first interval", "find: miss beyond the last interval")
KIND3 = ("kind 2 with the bit clear", "kind 3: no overlap, next interval", "kind 3: no overlap, no next interval", "kind 3: max_end - mlen + 1", "kind 3: return 0")
KIND11 = ("kind 11 returning 0", "kind 11 returning 1", "kind 11 returning 3", "kind 11 with d > pair_reach")
GENES = FIND + KIND3 + KIND11 + ("find: miss in a gap", "kind 3: max_next", "kind 10 with sti == eti", "kind 11 returning 2")
JUNCTIONS = ("kind 4: false", "kind 4: true by trans_dist", "kind 4: true by td2intron")
SUBSET, SKIPPED, MORE = "kind 3: epos > iv.epos keeps some segments and drops others", "kind 10 with a skipped zero state", "kind 9 with more"
TABLE_VIEW = GENES + (SUBSET, SKIPPED)                                           # views made of dense's arrays: the table and bitset kinds
FLOORS = {
    "dense": GENES + JUNCTIONS + (SUBSET, SKIPPED, MORE),
    "long": GENES + JUNCTIONS + ("kind 11 with d > MAXDISCRDTLEN, d <= pair_reach and a non-zero answer",),
    "twochr": GENES + JUNCTIONS,
    "variety-0": GENES + JUNCTIONS + (SUBSET, SKIPPED), "variety-1": GENES + JUNCTIONS + (SUBSET, SKIPPED),
    "tiny2r-0": GENES + JUNCTIONS + (SKIPPED,), "tiny2r-1": GENES + JUNCTIONS + (SKIPPED,),
    "np-nobucket": TABLE_VIEW, "np-shift6": TABLE_VIEW, "np-shift14": TABLE_VIEW, "np-noslack": TABLE_VIEW, "np-nbits": TABLE_VIEW,
    "np-single": FIND + KIND3 + KIND11 + ("kind 4: false", "kind 10 with sti == eti"),
    "np-nseg0": GENES + JUNCTIONS + (SUBSET, SKIPPED, MORE, "find: hit with nseg == 0"),
}


@pytest.mark.parametrize("name", aq.ALL_ANNOTS)
def test_batch_is_not_vacuous(name):
    """at least 20 requests of each category, the kind-11 ones included.  If a floor fails, the generator is to be repaired, not
    the floor."""
    c = aq.categories(aq.batch(name))
    print(name, c)
    for cat in FLOORS[name]:
        assert c.get(cat, 0) >= 20, (name, cat, c.get(cat, 0))


def test_every_category_has_a_batch():
    held = {c for cats in FLOORS.values() for c in cats}
    assert held == set(GENES + JUNCTIONS) | {SUBSET, SKIPPED, MORE, "find: hit with nseg == 0", "kind 11 with d > MAXDISCRDTLEN, d <= pair_reach and a non-zero answer"}
    assert set(FLOORS) == set(aq.ALL_ANNOTS)


@pytest.mark.parametrize("name", aq.ALL_ANNOTS)
def test_pair_reach_bounds_every_pair_the_predicate_can_accept(emu_annot, name):
    """pair_code's quick reject is exact only if no two intervals that share a transcript, and no interval and gene span that
    same_gene_span can accept, reach farther than AnnotDev::pair_reach: every such extent is <= it and the largest equals it"""
    A = aq.annot(name)
    a = A.a
    reach = emu_annot.pair_reach(A.av)
    ext = [0]
    by_t = {}
    for i in range(A.n_iv):
        for sg in aq._segs(A, i):
            g = int(a["seg_gene_id"][sg])
            ext.append(max(int(a["iv_epos"][i]), int(a["gene_end"][g])) - min(int(a["iv_spos"][i]), int(a["gene_start"][g])))
            for t in a["seg_tid"][a["seg_tid_off"][sg]:a["seg_tid_off"][sg + 1]]:
                by_t.setdefault(int(t), []).append(i)
    for ivs in by_t.values():
        ext.append(int(a["iv_epos"][max(ivs)]) - int(a["iv_spos"][min(ivs)]))
    assert max(ext) == reach == aq.brute_pair_reach(A), (max(ext), reach)


def test_partial_last_word_of_the_bitsets(emu_annot):
    """n_bits = 16 Ki - 7: the arrays hold ceil(n_bits / 64) words and every p < n_bits is answered from them -- the bits of the
    last, partial word included; p >= n_bits is 0"""
    A = aq.annot("np-nbits")
    p = np.arange(16320, 16400)
    out, _ = emu_annot(aq.params(4, 0), A.av, aq._mk(6, p))
    want = aq.brute_bits(A, "near_border_bits", p)
    assert want[p < aq.SMALL_NBITS].sum() >= 8 and (want[p >= aq.SMALL_NBITS] == 0).all()
    assert np.array_equal(out["ret"], want) and np.array_equal(out["aux"], aq.brute_bits(A, "intronic_bits", p))


def test_lookups_stay_inside_their_arrays(tmp_path):
    """tests/diag/annot_san_main.cpp: the host build of annot_req_run under AddressSanitizer and UBSan as a stand-alone program, every
    array of the annotation in a heap block of exactly its size, with the bucket table and without"""
    exe = str(tmp_path / "annot_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "circminer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "diag", "annot_san_main.cpp"), os.path.join(ROOT, "tests", "hostemu.cpp"), "-o", exe])
    files = []
    for name in ("dense", "long", "np-nbits"):
        files.append(str(tmp_path / f"{name}.anq"))
        aq.dump(name, files[-1])
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(" 0 differ") == 12 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-2000:]
