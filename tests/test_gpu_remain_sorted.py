"""cm_format_remain_sorted on the device: the resident batch's active set ordered by k_remain_keys, the radix sort, k_remain_heads /
k_remain_gstart / k_remain_gsizes and k_remain_rank, then formatted by the kernels of cm_format_remain over either file's own list,
against the project's own host path -- cm_write_remain_records on files holding the same bytes, then cm_sort_remain -- byte for
byte; cm_mapping_run with CM_REMAIN_SORTED=1 and cm_circ_run with CM_CIRC_PRESORTED=1 on what it leaves.

The data are remain_sorted_util.tie_case's: tie groups of 1, 2, 16, 17, 64 and 65 members, scattered over the batch, whose members
differ in the name (a prefix, a byte below 0x20, one above 0x7f), in the fields, the bases, the qualities, or not at all, and in
another way in file 2 than in file 1.  The runs of cm_mapping_run share the process: the variables are read by every call."""
import ctypes as C
import os

import numpy as np
import pytest

from circminer_amd import lib as cl
from fastq_text_util import whole_records
from pam_text_util import CHRS
from remain_sorted_util import check_sorted, parts, sorted_files, split4, tie_kinds, tie_text
from remain_text_util import CM_ELIMIT, SPAN_RECS, HostRemain, key_value, parsed_key, remain_states

pytestmark = pytest.mark.gpu
BITS = dict(keep_names=True, keep_quals=True, keep_names2=True)
GROUP_SIZES = (65, 64, 17, 16, 2, 1)


def mixed_sizes(n):
    out, k = [], 0
    while sum(out) < n:
        out.append(min(GROUP_SIZES[k % len(GROUP_SIZES)], n - sum(out)))
        k += 1
    return out


@pytest.fixture(scope="module")
def hp_plain(built):
    hp = cl.HotPath(cl.default_params())
    yield hp
    hp.close()


@pytest.fixture(scope="module")
def hp_wide(built):
    hp = cl.HotPath(cl.default_params(kmer=14))                  # 300 / 14 = 21 seeds per read: the library's 24-seed build
    yield hp
    hp.close()


def _stage(hp, t1, t2, st):
    n = len(st)
    assert hp.stage_text(t1, t2, n, **BITS)[0].n_pairs == n
    hp.swap()
    hp.poke_states(st)


def _sorted(hp, h, st, sel, first=0, count=None, chrs=CHRS):
    f1, f2, keys, offs, n_rec, stats = hp.format_remain_sorted(chrs, first=first, count=count)
    assert n_rec == len(sel)
    c = len(sel) - first if count is None else count
    assert stats[:2] == [2 * c, len(f1) + len(f2)] and stats[2] + stats[3] == 2 * ((c + SPAN_RECS - 1) // SPAN_RECS)
    return check_sorted(f1, f2, keys, offs, h, st, sel, first, count, chrs=chrs) + (stats,)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("shape,n", [("distinct", 1), ("equal", 2), ("equal", 65), ("distinct", 64), ("mixed", 63), ("mixed", 700), ("mixed", 4100)])
def test_directed_cases(hp_plain, hp_wide, monkeypatch, tmp_path, shape, n, wide):
    """stage with bits 2 | 3 | 4 -> swap -> poke the tie groups' states -> format_remain_sorted: the whole set, ranges that cut a tie
    group, the unsorted sibling before and after with its old bytes; in both kernel builds (reads of 300 bp in the 24-seed one)"""
    monkeypatch.delenv("CM_REMAIN_TIE_CAP", raising=False)
    hp = hp_wide if wide else hp_plain
    rng = np.random.default_rng(n + 31 * wide)
    sizes = {"distinct": [1] * n, "equal": [n], "mixed": mixed_sizes(n)}[shape]
    t1, t2, st, group = tie_text(rng, sizes, 300 if wide else 150)
    h = HostRemain(tmp_path, t1, t2, n, tag="d")
    _stage(hp, t1, t2, st)
    sel = np.arange(n)
    before = hp.format_remain(CHRS, keys=True)
    assert before[:2] == h.files(st, sel) and before[2].tolist() == [key_value(st[i], CHRS) for i in range(n)]
    unsorted, want, keys, stats = _sorted(hp, h, st, sel)
    after = hp.format_remain(CHRS, keys=True)
    assert after[:2] == before[:2] and np.array_equal(after[2], before[2]) and after[3:] == before[3:]
    tied = [i for i in range(1, n) if keys[i] == keys[i - 1]]
    assert bool(tied) == (shape != "distinct")
    ranges = [(0, 0), (n, None), (n - 1, 1), (n // 3, None)]
    if tied:
        i = tied[len(tied) // 2]
        ranges += [(i, min(3, n - i)), (0, i), (i, None)]
    for first, count in ranges:
        _sorted(hp, h, st, sel, first, count)
    if n == 700:
        for m in (0, 1):
            assert tie_kinds(want[m], keys) >= {"prefix", "low", "high", "star", "fields", "bases", "shorter", "quals", "identical"}
        assert stats[2] > 0                                                      # spans staged in the window (the direct path, stats[3]: the long names below)
        _sorted(hp, h, st, sel, chrs=[])                                         # another chromosome table (none): other keys, other ties
        _sorted(hp, h, st, sel)
    h.close()


def test_long_names_take_the_direct_path(hp_plain, monkeypatch, tmp_path):
    monkeypatch.delenv("CM_REMAIN_TIE_CAP", raising=False)
    rng = np.random.default_rng(3)
    t1, t2, st, group = tie_text(rng, mixed_sizes(130), 150, long_names=600)
    n = len(st)
    h = HostRemain(tmp_path, t1, t2, n, tag="long")
    _stage(hp_plain, t1, t2, st)
    unsorted, want, keys, stats = _sorted(hp_plain, h, st, np.arange(n))
    assert stats[3] >= 130 // SPAN_RECS * 2                                      # every full span of either file: 16 names alone exceed the window
    assert tie_kinds(want[0], keys) >= {"prefix", "low", "high", "fields", "quals", "identical"}
    h.close()


def test_the_cap(built, monkeypatch, tmp_path):
    """CM_REMAIN_TIE_CAP=64: a group of 64 is ordered; a group of 65 is CM_ELIMIT with nothing written and n_records set, the message
    names both numbers, and a good call follows"""
    hp = cl.HotPath(cl.default_params())
    L = cl.load()
    try:
        monkeypatch.setenv("CM_REMAIN_TIE_CAP", "64")
        rng = np.random.default_rng(9)
        t1, t2, st, _ = tie_text(rng, [64, 3, 1, 64], 150)
        h = HostRemain(tmp_path, t1, t2, len(st), tag="c64")
        _stage(hp, t1, t2, st)
        _sorted(hp, h, st, np.arange(len(st)))
        h.close()
        t1, t2, st, _ = tie_text(rng, [5, 65, 1], 150)
        n = len(st)
        h = HostRemain(tmp_path, t1, t2, n, tag="c65")
        _stage(hp, t1, t2, st)
        u1, u2, _, _ = sorted_files(h, st, np.arange(n))
        bufs = [np.full(len(u) + 8, 0xA5, np.uint8) for u in (u1, u2)]
        keys, offs = np.full(n, -7, np.int64), [np.full(n + 1, 0xA5A5A5A5, np.uint32) for _ in (0, 1)]
        got, n_rec, stats = (C.c_uint64 * 2)(7, 7), C.c_uint64(99), (C.c_uint64 * 4)(1, 1, 1, 1)
        rc = L.cm_format_remain_sorted(hp.h, cl.chr_array(CHRS), len(CHRS), 0, n, bufs[0].ctypes.data, len(u1), bufs[1].ctypes.data, len(u2), got, keys.ctypes.data,
                                       offs[0].ctypes.data, offs[1].ctypes.data, C.byref(n_rec), stats)
        assert rc == CM_ELIMIT and list(got) == [0, 0] and n_rec.value == n and list(stats) == [0, 0, 0, 0]
        assert all(bool((b == 0xA5).all()) for b in bufs) and bool((keys == -7).all()) and all(bool((o == 0xA5A5A5A5).all()) for o in offs)
        msg = L.cm_last_error(hp.h).decode()
        assert "65" in msg and "64" in msg and "cm_format_remain_sorted" in msg, msg
        assert hp.download()[0].tobytes() == st.tobytes() and hp.format_remain(CHRS)[:2] == (u1, u2)     # the batch is as it was
        monkeypatch.setenv("CM_REMAIN_TIE_CAP", "65")                            # read by every call
        _sorted(hp, h, st, np.arange(n))
        monkeypatch.delenv("CM_REMAIN_TIE_CAP")
        _sorted(hp, h, st, np.arange(n))
        h.close()
    finally:
        hp.close()


def test_the_set_mapping_leaves_active(ds_tiny2r, monkeypatch, tmp_path):
    """stage A -> swap -> stage B -> map_rounds (B's first round is prefetched): the sorted records of the pairs mapping left
    active, then of the directed states (keys that tie) over the same set; after the swap B's.  ms[7] covers the sort."""
    monkeypatch.delenv("CM_REMAIN_TIE_CAP", raising=False)
    ds = ds_tiny2r
    hp = cl.HotPath(cl.default_params(kmer=ds.kmer))
    try:
        for ci in range(ds.hi.n_contigs):
            hp.load_contig(ci, ds.hi.views[ci], ds.hi.annots[ci])
        slots = list(range(ds.hi.n_contigs))
        n = ds.batch.n
        half = n // 2
        rng = np.random.default_rng(5)
        texts = []
        for mate, arr in ((1, ds.d.seq1), (2, ds.d.seq2)):        # names shared by three pairs each and differing between the files
            texts.append(b"".join(b"@pair%d%s/%d\n%s\n+\n%s\n" % (i // 3, (b"n" if mate == 1 else b"mm") * (i % 9 // 3), mate, arr[i].tobytes(),
                                                                 bytes(rng.integers(33, 74, len(arr[i])).astype(np.uint8))) for i in range(n)))
        t1, t2 = texts
        r1, r2 = whole_records(t1, True)[0], whole_records(t2, True)[0]
        a = (t1[:int(r1[half])], t2[:int(r2[half])])
        b = (t1[int(r1[half]):], t2[int(r2[half]):])
        chrs = list(ds.d.chr_table)
        ha, hb = HostRemain(tmp_path, *a, half, tag="A", chrs=chrs), HostRemain(tmp_path, *b, n - half, tag="B", chrs=chrs)
        assert hp.stage_text(*a, half, **BITS)[0].n_pairs == half
        hp.swap()
        assert hp.stage_text(*b, n, **BITS)[0].n_pairs == n - half
        hp.map_rounds(slots)
        for hx, m in ((ha, half), (hb, n - half)):
            sel = hp.collect_records()["pair"].astype(np.int64).copy()
            assert 0 < len(sel) < m
            st = hp.download()[0]
            plain = hp.format_remain(chrs)[:2]
            hp.prof(True)
            hp.prof_reset()
            _sorted(hp, hx, st, sel, chrs=chrs)
            assert hp.prof_get()[0][7] > 0
            hp.prof(False)
            _sorted(hp, hx, st, sel, 1, len(sel) - 1, chrs=chrs)
            assert hp.format_remain(chrs)[:2] == plain
            ds_st = remain_states(m, len(chrs))                   # keys that tie, over the active set mapping chose
            hp.poke_states(ds_st)
            _, want, keys, _ = _sorted(hp, hx, ds_st, sel, chrs=chrs)
            assert len(set(keys)) < len(keys) and tie_kinds(want[0], keys) & {"name", "prefix"}
            if hx is ha:
                hp.swap()
                hp.map_rounds(slots)                              # takes B's first round over from the prefetch
        ha.close()
        hb.close()
    finally:
        hp.close()


# ---- cm_mapping_run with CM_REMAIN_SORTED=1, cm_circ_run with CM_CIRC_PRESORTED=1 ------------------------------------------------------
N_BASE = 800


@pytest.fixture(scope="module")
def run_files(tmp_path_factory, built):
    """the data set's pairs three times under names that say where they stand: the first half as triples side by side (ties inside
    a batch), the second half as three blocks of 400 (the first and the last copy of a pair are 800 records apart: other batches)"""
    from circminer_amd import synth
    from stage2_util import write_fastq_pair
    tmp = tmp_path_factory.mktemp("remain_sorted_run")
    d = synth.generate("tiny2r", n_pairs=N_BASE, seed=45, mix=(0.3, 0.1, 0.6))
    fa = str(tmp / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    packed, info = cl.pack_genome(fa, 150_000)
    idx = cl.write_index(packed, kmer=20, n_threads=4)
    gtf = str(tmp / "ref.gtf")
    open(gtf, "w").write(d.gtf_text)
    h = N_BASE // 2
    order = np.concatenate([np.repeat(np.arange(h), 3), np.tile(np.arange(h, N_BASE), 3)])

    class _Sub:
        seq1, seq2 = d.seq1[order], d.seq2[order]
    fq1, fq2 = write_fastq_pair(tmp, _Sub, len(order), name=lambda i: f"r{i:05d}")
    return tmp, len(order), idx, gtf, fq1, fq2


def _run(run_files, out, monkeypatch, sorted_=False, cap=None, world=1):
    tmp, n, idx, gtf, fq1, fq2 = run_files
    for var, val in (("CM_FASTQ_DEVICE", "1"), ("CM_FASTQ_DEVICE_BLOCK", "65536"), ("CM_REMAIN_DEVICE", "1"), ("CM_REMAIN_TRACE", "1")):
        monkeypatch.setenv(var, val)
    for var, val in (("CM_REMAIN_SORTED", "1" if sorted_ else None), ("CM_REMAIN_TIE_CAP", cap)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    for var in ("CM_PAM_DEVICE", "CM_SAM_DEVICE"):
        monkeypatch.delenv(var, raising=False)
    out = str(tmp / out)
    sts = [cl.run_mapping(idx, gtf, fq1, fq2, out, cl.default_params(kmer=0), report=0, n_threads=4, batch_pairs=512, rank=r, world=world) for r in range(world)]
    cl.merge_parts(out, 2, world, 0)
    files = tuple(open(f"{out}_2_remain_R{m}.fastq", "rb").read() for m in (1, 2))
    srt = tuple(open(f"{out}_2_remain_R{m}.fastq.srt", "rb").read() if os.path.exists(f"{out}_2_remain_R{m}.fastq.srt") else None for m in (1, 2))
    return (sum(s.pairs for s in sts), sum(s.bsj_pairs for s in sts), [sum(s.by_type[t] for s in sts) for t in range(14)],
            [s.device_parsed_batches for s in sts]), files, srt, out


def test_files_to_files_with_sorted_runs(run_files, monkeypatch, capfd):
    tmp, n, idx, gtf, fq1, fq2 = run_files
    base_counts, base, base_srt, base_out = _run(run_files, "base", monkeypatch)
    assert base_srt == (None, None) and base_counts[0] == n and base_counts[1] > 50 and base_counts[3][0] >= 3
    capfd.readouterr()
    counts, files, srt, out = _run(run_files, "srt", monkeypatch, sorted_=True)
    trace = [ln for ln in capfd.readouterr().err.split("\n") if ln.startswith("[remain] sorted runs:")]
    assert counts == base_counts and files == base                              # the remain files and the statistics are unchanged
    want = tuple(open(cl.sort_remain(f"{base_out}_2_remain_R{m}.fastq", str(tmp / f"want_R{m}.srt")), "rb").read() for m in (1, 2))
    assert srt == want
    assert len(trace) == 1 and f"{counts[3][0]} batches, 0 sorted on the host, {counts[1]} records" in trace[0], trace
    # on the checker's files: keys tie inside a batch (copies side by side) and across batches (copies more than a batch apart)
    where = {}
    for r in split4(want[0]):
        hdr = r.split(b"\n")[0]
        where.setdefault(parsed_key(hdr), []).append(int(parts(r)[0][1:]))
    near = sum(1 for v in where.values() if any(0 < abs(p - q) <= 2 and p // 3 == q // 3 and p < 3 * N_BASE // 2 for p in v for q in v))
    far = sum(1 for v in where.values() if max(v) - min(v) > 512)
    assert near > counts[3][0] and far > 0                                       # (more than there are batch boundaries to split them)
    # stage 2 on the sorted files as they are
    monkeypatch.delenv("CM_CIRC_PRESORTED", raising=False)
    cl.run_circ(idx, gtf, base_out, 2, cl.default_params(kmer=0))
    monkeypatch.setenv("CM_CIRC_PRESORTED", "1")
    for m in (1, 2):
        os.rename(f"{out}_2_remain_R{m}.fastq", f"{out}_2_remain_R{m}.fastq.away")     # nothing sorts them again
    cl.run_circ(idx, gtf, out, 2, cl.default_params(kmer=0))
    monkeypatch.delenv("CM_CIRC_PRESORTED")
    for ext in (".candidates.pam", ".circ_report"):
        assert open(out + ext, "rb").read() == open(base_out + ext, "rb").read()
    assert os.path.getsize(base_out + ".candidates.pam") > 0
    # a cap of two: batches with three copies side by side are ordered on the host, the files are the same
    capfd.readouterr()
    counts2, files2, srt2, _ = _run(run_files, "cap2", monkeypatch, sorted_=True, cap="2")
    trace = [ln for ln in capfd.readouterr().err.split("\n") if ln.startswith("[remain] sorted runs:")]
    assert counts2 == base_counts and files2 == base and srt2 == want
    assert len(trace) == 1 and int(trace[0].split(" batches, ")[1].split(" ")[0]) >= 1, trace
    # two ranks: the variable has no effect
    counts3, files3, srt3, out3 = _run(run_files, "w2", monkeypatch, sorted_=True, world=2)
    assert counts3[:3] == base_counts[:3] and files3 == base and srt3 == (None, None)
    assert not [f for f in os.listdir(str(tmp)) if ".srt" in f and os.path.basename(out3) in f]
