"""The producer side of a batch on the device -- cm_reads_upload, cm_reads_stage, cm_reads_stage_text, cm_reads_swap -- where the
existing tests do not go: what a refused stage leaves of the batch staged before it, and what becomes of the names and qualities a
stage kept when its buffer set is taken again by a stage that keeps less.  Fresh contexts, no index: peek_reads, peek_quals and the
formatters on first-round states, against the project's own host parser and writers (fastq_text_util, pam_text_util, sam_text_util,
remain_text_util)."""
import ctypes as C

import numpy as np
import pytest

from circminer_amd import lib as cl
from fastq_text_util import HostParse, malformed, records, text_of
from pam_text_util import CHRS
from remain_text_util import CM_EINVAL, CM_ESTATE, HostRemain, remain_pair_text
from sam_text_util import HostSam

pytestmark = pytest.mark.gpu
ALL = dict(keep_names=True, keep_quals=True, keep_names2=True)


def _rc(call, *a, **kw):
    """(error code, message) of a call that is refused"""
    with pytest.raises(RuntimeError) as e:
        call(*a, **kw)
    return int(str(e.value).split("(")[1].split(")")[0]), str(e.value)


def _resident_is(hp, b):
    s1, o1, s2, o2 = hp.peek_reads()
    return all(np.array_equal(x, y) for x, y in ((s1, b.seq1), (o1, b.off1), (s2, b.seq2), (o2, b.off2)))


def test_a_refused_stage_and_the_batch_staged_before_it(built):
    """8 pairs of 40 bases.  A stage refused for its arguments (cm_reads_stage: a pair longer than max_read_len; cm_reads_stage_text:
    a null text with a length) leaves the batch staged before it in place: swap succeeds and makes it resident.  A cm_reads_stage_text
    refused for its content (a short quality line) has dropped it: swap finds no staged batch, the resident batch stays."""
    n, ln, lim = 8, 40, 100
    rng = np.random.default_rng(71)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    good = cl.ReadBatch(acgt[rng.integers(0, 4, (n, ln))], acgt[rng.integers(0, 4, (n, ln))])
    lens = np.full(n, ln)
    lens[5] = lim + 1
    long5 = cl.ReadBatch(acgt[rng.integers(0, 4, int(lens.sum()))], acgt[rng.integers(0, 4, n * ln)], lens, np.full(n, ln))
    recs = records(rng, n, lo=ln, hi=ln)
    t_bad, t2 = text_of(malformed(recs, 3, "qual_short")), text_of(records(rng, n, lo=ln, hi=ln, mate=2))
    hp = cl.HotPath(cl.default_params(max_read_len=lim))
    try:
        hp.stage(good)                                            # refused for its arguments
        rc, msg = _rc(hp.stage, long5)
        assert rc == CM_EINVAL and "pair 5 longer than max_read_len %d" % lim in msg
        hp.swap()
        assert _resident_is(hp, good)
        hp.stage(good)                                            # refused for its content
        rc, msg = _rc(hp.stage_text, t_bad, t2, n)
        assert rc == CM_EINVAL and "FASTQ file 1, record 3 of the block: the quality line is not as long as the sequence line" in msg
        rc, msg = _rc(hp.swap)
        assert rc == CM_ESTATE and "no staged batch" in msg
        assert _resident_is(hp, good)
        other = cl.ReadBatch(good.seq2.reshape(n, ln), good.seq1.reshape(n, ln))
        hp.upload(other)
        hp.stage(good)                                            # a null text with a length
        tb = cl.TextBatch()
        b2 = np.frombuffer(t2, np.uint8)
        assert hp.L.cm_reads_stage_text(hp.h, None, 100, b2.ctypes.data, b2.size, n, 3, None, None, C.byref(tb)) == CM_EINVAL
        assert "null text" in hp.L.cm_last_error(hp.h).decode()
        assert _resident_is(hp, other)
        hp.swap()
        assert _resident_is(hp, good)
    finally:
        hp.close()


@pytest.fixture(scope="module")
def two_texts(tmp_path_factory, built):
    """65 pairs twice (A, B), a run of long names in both files that crosses a wave of the row kernels, with the host parser's and
    the host writers' view of each, made once"""
    tmp = tmp_path_factory.mktemp("batch_staging")
    n = 65
    out = {"n": n}
    for tag, seed in (("A", 171), ("B", 271)):
        t1, t2 = remain_pair_text(np.random.default_rng(seed), n, (n // 2, n))
        out[tag] = (t1, t2, HostParse(tmp, t1, t2, n, tag="p" + tag), HostRemain(tmp, t1, t2, n, tag="r" + tag), HostSam(tmp, t1, t2, n, tag="s" + tag))
    yield out
    for tag in "AB":
        out[tag][3].close()
        out[tag][4].close()


def _refusals(hp, names, quals, names2):
    """every reader of kept data that misses some refuses with CM_ESTATE and names exactly the missing bits"""
    def check(call, need, *a):
        miss = [(bit, noun) for has, bit, noun in need if not has]
        if not miss:
            return
        rc, msg = _rc(call, *a)
        want = "flag bit%s %s (%s)" % ("s" if len(miss) > 1 else "", ", ".join(b for b, _ in miss), ", ".join("no " + x for _, x in miss))
        assert rc == CM_ESTATE and msg.endswith(want), (msg, want)
    check(hp.peek_quals, [(quals, "3", "qualities")])
    check(hp.format_pam, [(names, "2", "names")], CHRS)
    check(hp.format_sam, [(names, "2", "names"), (quals, "3", "qualities")], CHRS)
    check(hp.format_remain, [(names, "2", "R1 names"), (quals, "3", "qualities"), (names2, "4", "R2 names")], CHRS)


def test_kept_data_goes_away_with_its_buffer_set(two_texts):
    """A buffer set that held every kept array (bits 2 | 3 | 4) is taken again by stages that keep nothing, or less: the readers of
    what is no longer kept refuse and name exactly the missing bits, the others give the new batch's bytes; then a host batch
    through stage + swap and through upload: all refuse."""
    n = two_texts["n"]
    a1, a2, pa, ra, sa = two_texts["A"]
    b1, b2, _, rb, _ = two_texts["B"]
    host = cl.ReadBatch(np.full((n, 40), ord("A"), np.uint8), np.full((n, 40), ord("C"), np.uint8))
    hp = cl.HotPath(cl.default_params())

    def staged(t1, t2, **bits):
        assert hp.stage_text(t1, t2, n, **bits)[0].n_pairs == n
        hp.swap()
        return hp.download()[0]
    try:
        st = staged(a1, a2, **ALL)                                # 1: the first set keeps everything
        assert hp.format_pam(CHRS)[0] == ra.rows(st) and hp.format_sam(CHRS)[0] == sa.rows(st)
        assert hp.format_remain(CHRS)[:2] == ra.files(st, np.arange(n))
        staged(b1, b2)                                            # 2: the other set
        _refusals(hp, False, False, False)
        staged(a1, a2)                                            # 3: the first set again, nothing kept
        _refusals(hp, False, False, False)
        s1, o1, s2, o2 = hp.peek_reads()
        assert np.array_equal(o1, pa.off1) and np.array_equal(s1, pa.seq1) and np.array_equal(o2, pa.off2) and np.array_equal(s2, pa.seq2)
        st = staged(b1, b2, keep_names=True)                      # 4: the other set, R1 names only
        assert hp.format_pam(CHRS)[0] == rb.rows(st)
        _refusals(hp, True, False, False)
        hp.stage(host)                                            # 5: a host batch through the first set
        hp.swap()
        _refusals(hp, False, False, False)
        assert _resident_is(hp, host)
        hp.upload(host)                                           # 6
        _refusals(hp, False, False, False)
        staged(a1, a2, **ALL)                                     # ... and an upload over a resident set that keeps everything
        hp.upload(host)
        _refusals(hp, False, False, False)
        assert _resident_is(hp, host)
    finally:
        hp.close()
