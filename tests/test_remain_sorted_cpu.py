"""The sorted remain formatter without a device: the bodies of circminer_amd/csrc/cm_remain_order.h run by a host emulation
(tests/hostemu_remain_order.cpp: lanes and groups in shuffled order, the records through the plan under shadow buffers) against the
project's own host path -- cm_write_remain_records on files holding the same bytes, then cm_sort_remain --, byte for byte; the merge
of sorted runs (cm_remain_runs) against cm_sort_remain of the concatenation; cm_circ_run on files sorted beforehand."""
import os

import numpy as np
import pytest

from circminer_amd import lib as cl
from pam_text_util import CHRS
from remain_sorted_util import (TIE_CAP, EmuSorted, check_sorted, emu_remain_order, order_of, parts, sorted_files, split4, tie_kinds, tie_text)
from remain_text_util import CM_EINVAL, CM_ELIMIT, ROOT, Emu, HostRemain, key_value, parsed_key, selections

CM_EIO = -7
GROUP_SIZES = (65, 64, 17, 16, 2, 1)
KINDS = {"prefix", "low", "high", "star", "fields", "bases", "shorter", "quals", "identical"}


@pytest.fixture(scope="module")
def emu_ord(built):
    return emu_remain_order()


def mixed_sizes(n):
    """groups of 65, 64, 17, 16, 2 and 1 members, again and again, until n pairs are laid out"""
    out, k = [], 0
    while sum(out) < n:
        out.append(min(GROUP_SIZES[k % len(GROUP_SIZES)], n - sum(out)))
        k += 1
    return out


def _setup(E, tmp_path, rng, sizes, hi=300, tag="srt"):
    t1, t2, st, group = tie_text(rng, sizes, hi)
    n = len(st)
    h = HostRemain(tmp_path, t1, t2, n, tag=tag)
    return h, EmuSorted(E, Emu(E, h)), st, group, n


def _run(es, h, st, sel, first=0, count=None, **kw):
    rc, got, bufs, keys, offs, n_rec, stats, ties = es.format(st, sel, first, count, **kw)
    assert rc == 0 and n_rec == len(sel), (rc, n_rec)
    for m in (0, 1):
        assert bool((bufs[m][got[m]:] == 0xA5).all())
    out = check_sorted(bufs[0][:got[0]].tobytes(), bufs[1][:got[1]].tobytes(), keys, offs, h, st, sel, first, count)
    return out + (ties, stats)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4100])
@pytest.mark.parametrize("shape", ["distinct", "equal", "mixed"])
def test_emulated_order_equals_sort_remain(emu_ord, tmp_path, n, shape):
    """Every size under every shape, all five selections of remain_text_util.selections, every range.  The keys are
    remain_sorted_util.tie_case's: it lays out the
    same boundaries remain_states has (contig_num of CONTIG_VALUES: negative, beyond 2^32, 20-byte keys; a sum that wraps 2^32;
    star forms and a mapped 0) but with one key per tie group, which remain_states' cycles cannot give; remain_states itself is
    poked over the set mapping leaves active in the GPU test."""
    rng = np.random.default_rng(n * 3 + len(shape))
    sizes = {"distinct": [1] * n, "equal": [n], "mixed": mixed_sizes(n)}[shape]
    h, es, st, group, n = _setup(emu_ord, tmp_path, rng, sizes)
    if shape == "equal" and n > TIE_CAP:                                         # one group above the cap: the refusal, nothing written
        rc, got, bufs, keys, offs, n_rec, stats, ties = es.format(st, np.arange(n))
        assert rc == CM_ELIMIT and got == [0, 0] and n_rec == n and stats == [0, 0, 0, 0] and ties[0] == n and bool((keys == -7).all())
        h.close()
        return
    for tag, sel in selections(rng, n).items():
        (unsorted, want, keys, ties, stats) = _run(es, h, st, sel, seed=n + 1)
        k = len(sel)
        if tag == "all":
            biggest = max(np.bincount(group)) if shape != "distinct" else 1
            assert ties[0] == (biggest if biggest > 1 else 0)
            if n <= 65:
                _, _, _, _, stats = _run(es, h, st, sel, seed=n + 2, window=1)   # every span direct
                assert stats[2] == 0
        # ranges: empty ones, the last record, and -- where keys tie -- ranges that begin and end inside a tie group
        ranges = [(0, 0), (k, 0), (k, None), (max(k - 1, 0), min(k, 1)), (k // 3, None)]
        tied = [i for i in range(1, k) if keys[i] == keys[i - 1]]
        if tied:
            i = tied[len(tied) // 2]
            ranges += [(i, min(3, k - i)), (0, i), (i, None)]
        else:
            assert shape == "distinct" or k < 2 or tag != "all"
        for first, count in ranges:
            _run(es, h, st, sel, first, count, seed=first + 11)
    # refusals of the range and of the caps, as cm_format_remain's
    sel = np.arange(n)
    for first, count in ((n, 1), (0, n + 1), (n + 1, None)):
        rc, got, _, _, _, n_rec, _, _ = es.format(st, sel, first, count, caps=(10, 10))
        assert rc == CM_EINVAL and got == [0, 0] and n_rec == n
    u1, u2, _, _ = sorted_files(h, st, sel)
    rc, got, bufs, keys, _, n_rec, stats, _ = es.format(st, sel, caps=(len(u1) - 1, len(u2)))
    assert rc == CM_ELIMIT and got == [len(u1), len(u2)] and n_rec == n and stats == [0, 0, 0, 0] and all(bool((b == 0xA5).all()) for b in bufs) and bool((keys == -7).all())
    h.close()


def test_the_data_ties_in_every_way(emu_ord, tmp_path):
    """on the checker's files alone: every way a tie is decided occurs in either file, the two files order the pairs differently,
    the keys are negative, beyond 2^32, and 0 for star forms and for a mapped state among them; reads of 0, 1, 150 and 300 bases"""
    rng = np.random.default_rng(7)
    h, es, st, group, n = _setup(emu_ord, tmp_path, rng, mixed_sizes(700))
    sel = np.arange(n)
    unsorted, want, keys, ties, _ = _run(es, h, st, sel)
    for m in (0, 1):
        assert tie_kinds(want[m], keys) >= KINDS, (m, KINDS - tie_kinds(want[m], keys))
        assert [parsed_key(r.split(b"\n")[0]) for r in want[m]] == keys           # the value is what the text says: no name moves field 2
        assert {0, 1, 150, 300} <= {len(parts(r)[2]) for r in want[m]}
    assert order_of(unsorted[0], want[0]) != order_of(unsorted[1], want[1])
    assert min(keys) < -2 ** 61 and max(keys) > 2 ** 61 and sum(k == 0 for k in keys) == 65
    zero = [parts(r)[1] for r, k in zip(want[0], keys) if k == 0]
    assert any(f.startswith(b" * ") for f in zero) and any(f.startswith(b" 0 ") for f in zero)
    assert ties == [65, sum(s > 1 for s in mixed_sizes(700)), sum(s for s in mixed_sizes(700) if s > 1)]
    assert any(b"chr_of_forty_bytes_" in r for r in want[0])
    h.close()


def test_a_tie_group_at_the_cap_and_above_it(emu_ord, tmp_path):
    rng = np.random.default_rng(11)
    for sizes, ok in (([64, 3, 1, 64], True), ([65, 3, 1], False), ([5, 65], False)):
        h, es, st, group, n = _setup(emu_ord, tmp_path, rng, sizes, hi=150, tag=f"cap{sizes[0]}{ok}")
        sel = np.arange(n)
        if ok:
            _run(es, h, st, sel, tie_cap=64)
        else:
            rc, got, bufs, keys, offs, n_rec, stats, ties = es.format(st, sel, tie_cap=64)
            assert rc == CM_ELIMIT and got == [0, 0] and n_rec == n and stats == [0, 0, 0, 0] and ties[0] == 65
            _run(es, h, st, sel, tie_cap=65)                                         # (the same data under a cap that holds it)
        h.close()


# ---- cm_remain_runs ----------------------------------------------------------------------------------------------------------------
def _run_of(recs1, recs2):
    """a sorted run's arguments from its records"""
    keys = [parsed_key(r.split(b"\n")[0]) for r in recs1]
    off = [np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.uint32) if rr else np.zeros(1, np.uint32) for rr in (recs1, recs2)]
    return b"".join(recs1), off[0], b"".join(recs2), off[1], np.array(keys, np.int64)


@pytest.mark.parametrize("cuts", [(), (300,), (0, 1, 1, 200, 201, 650), (0, 0, 700)], ids=["one", "two", "seven", "empty_ends"])
def test_merged_runs_equal_sort_remain_of_the_concatenation(emu_ord, tmp_path, cuts):
    """1, 2 and 7 runs and empty ones among them, a run of one record; the pairs are cut into runs wherever they stand, so that keys
    tie across runs and identical records lie in different runs (asserted below)"""
    rng = np.random.default_rng(5)
    t1, t2, st, group = tie_text(rng, mixed_sizes(700), 150)
    n = len(st)
    h = HostRemain(tmp_path, t1, t2, n, tag="runs")
    u1, u2, s1, s2 = sorted_files(h, st, np.arange(n))
    bounds = [0] + list(cuts) + [n]
    p = [str(tmp_path / f"merged_R{m}.srt") for m in (1, 2)]
    runs = cl.RemainRuns(p[0], p[1])
    seen, across, run_groups = {}, 0, []
    for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
        sel = np.arange(a, b)
        c1, c2, r1, r2 = sorted_files(h, st, sel, tag=f"run{k}")
        if k % 2:
            runs.add_unsorted(c1, c2)                                            # the fall-back: ordered by the library
        else:
            runs.add(*_run_of(split4(r1), split4(r2)))
        for r in split4(r1):
            across += 1 if seen.get(r, k) != k else 0
            seen[r] = k
        run_groups.append({int(g) for g in group[a:b]})
    if sum(1 for g in run_groups if g) > 1:
        assert across > 0 and any(x & y for i, x in enumerate(run_groups) for y in run_groups[i + 1:])
    assert runs.finish() == 0
    runs.close()
    assert open(p[0], "rb").read() == s1 and open(p[1], "rb").read() == s2
    h.close()


def test_runs_refusals_and_a_short_write(built, tmp_path):
    rec = b"@a 5 0\nAC\n+\nII\n"
    off = np.array([0, len(rec)], np.uint32)
    L = cl.load()
    runs = cl.RemainRuns(str(tmp_path / "a.srt"), str(tmp_path / "b.srt"))
    assert L.cm_remain_runs_add(runs.h, None, None, None, None, None, 0) == 0      # an empty run
    assert L.cm_remain_runs_add(runs.h, rec, off.ctypes.data, None, off.ctypes.data, np.array([5], np.int64).ctypes.data, 1) == CM_EINVAL
    two = np.array([0, len(rec), 2 * len(rec)], np.uint32)
    assert L.cm_remain_runs_add(runs.h, rec * 2, two.ctypes.data, rec * 2, two.ctypes.data, np.array([5, 4], np.int64).ctypes.data, 2) == CM_EINVAL   # keys that fall
    assert L.cm_remain_runs_add(runs.h, rec[:-1] + b"x", off.ctypes.data, rec, off.ctypes.data, np.array([5], np.int64).ctypes.data, 1) == CM_EINVAL   # no line feed
    assert runs.finish() == 0 and open(tmp_path / "a.srt", "rb").read() == b"" and open(tmp_path / "b.srt", "rb").read() == b""
    runs.close()
    assert L.cm_remain_runs_open(None, b"x", None) == CM_EINVAL and L.cm_remain_runs_finish(None) == CM_EINVAL
    L.cm_remain_runs_close(None)
    if os.path.exists("/dev/full"):
        for paths in (("/dev/full", str(tmp_path / "c.srt")), (str(tmp_path / "c.srt"), "/dev/full")):
            runs = cl.RemainRuns(*paths)
            runs.add(rec, off, rec, off, [5])
            assert runs.finish() == CM_EIO
            runs.close()
    runs = cl.RemainRuns(str(tmp_path / "no_such_dir" / "a.srt"), str(tmp_path / "b.srt"))
    assert runs.finish() == CM_EIO
    runs.close()


# ---- cm_circ_run on files sorted beforehand -------------------------------------------------------------------------------------------
def test_circ_run_takes_presorted_files(built, tmp_path, monkeypatch):
    from test_circ_call import _case
    d, gtf, (hi, ohi), P, prefix, r1, r2 = _case(tmp_path, "tiny2r", 1500, 23)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    packed, info = cl.pack_genome(fa, 150_000)
    idx = cl.write_index(packed, kmer=20, n_threads=4)
    outs = [prefix + ".candidates.pam", prefix + ".circ_report"]
    monkeypatch.delenv("CM_CIRC_PRESORTED", raising=False)
    st0 = cl.run_circ(idx, gtf, prefix, hi.n_contigs, cl.default_params(kmer=0))
    want = [open(p, "rb").read() for p in outs]
    assert st0.calls > 0 and want[0] and want[1]
    # the sorted files by way of the runs; the unsorted ones out of the way: nothing sorts them again
    for r in (r1, r2):
        os.remove(r + ".srt")
    runs = cl.RemainRuns(r1 + ".srt", r2 + ".srt")
    runs.add_unsorted(open(r1, "rb").read(), open(r2, "rb").read())
    assert runs.finish() == 0
    runs.close()
    for r in (r1, r2):
        os.rename(r, r + ".away")
    for p in outs:
        os.remove(p)
    with pytest.raises(RuntimeError):                                            # without the variable the remain files are needed
        cl.run_circ(idx, gtf, prefix, hi.n_contigs, cl.default_params(kmer=0))
    monkeypatch.setenv("CM_CIRC_PRESORTED", "1")
    st1 = cl.run_circ(idx, gtf, prefix, hi.n_contigs, cl.default_params(kmer=0))
    assert [open(p, "rb").read() for p in outs] == want and (st1.pairs, st1.candidate_rows, st1.calls) == (st0.pairs, st0.candidate_rows, st0.calls)
    os.remove(r2 + ".srt")
    with pytest.raises(RuntimeError, match=r"\(-7\).*_remain_R2\.fastq\.srt"):   # CM_EIO, and the file named
        cl.run_circ(idx, gtf, prefix, hi.n_contigs, cl.default_params(kmer=0))


def test_the_constants_are_the_headers():
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    assert f"TIE_CAP = {TIE_CAP};" in open(os.path.join(csrc, "cm_remain_order.h")).read()
