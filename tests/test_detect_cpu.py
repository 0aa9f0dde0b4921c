"""What cm_detect_run is made of, without a device: the memory reader (cm_fastq_open_mem) against the file reader on the same bytes,
the memory finish of the sorted runs (cm_remain_runs_finish_mem) against the file finish, the struct mirrors, and the refusals of
cm_detect_run and cm_circ_call_resident."""
import ctypes as C
import os

import numpy as np
import pytest

from circminer_amd import lib as cl
import circ_chain_util as u
from remain_sorted_util import sorted_files, split4, tie_text
from remain_text_util import HostRemain, parsed_key

CM_EINVAL, CM_ENODEV = -1, -2
GROUP_SIZES = (65, 64, 17, 16, 2, 1)


def _arrays(b):
    """every array of a batch and its prior, as bytes"""
    if b is None:
        return None
    n = b.n
    out = [n]
    for seq, off, qual, names, name_off in ((b.c.seq1, b.c.off1, b.fb.qual1, b.fb.names1, b.fb.name_off1), (b.c.seq2, b.c.off2, b.fb.qual2, b.fb.names2, b.fb.name_off2)):
        o = np.ctypeslib.as_array(off, (n + 1,)).copy()
        no = np.ctypeslib.as_array(name_off, (n + 1,)).copy()
        out += [o.tobytes(), no.tobytes(), C.string_at(C.cast(seq, C.c_void_p), int(o[n])), C.string_at(C.cast(qual, C.c_void_p), int(o[n])), C.string_at(names, int(no[n]))]
    out.append(None if b.prior is None else b.prior.tobytes())
    return out


def _drain(reader, max_pairs):
    """the batches of a reader to its end as _arrays, the error text of the call that failed in the last place"""
    got = []
    try:
        while True:
            b = reader.next_batch(max_pairs)
            got.append(_arrays(b))
            if b is None:
                return got
            assert len(got) < 10_000
    except RuntimeError as e:
        got.append(str(e))
        return got
    finally:
        reader.close()


def _both(tmp_path, chr_table, max_ed, t1, t2, max_pairs, tag):
    p = [str(tmp_path / f"{tag}_{m}.fq") for m in (1, 2)]
    for path, t in zip(p, (t1, t2)):
        open(path, "wb").write(t)
    from_files = _drain(cl.FastqReader(p[0], p[1], chr_table, max_ed), max_pairs)
    from_mem = _drain(cl.fastq_open_mem(t1, t2, chr_table, max_ed), max_pairs)
    assert from_mem == from_files, (tag, max_pairs, len(from_mem), len(from_files))
    return from_mem


@pytest.mark.parametrize("name", ["tiny", "tiny2r"])
def test_memory_reader_equals_file_reader(built, tmp_path, name):
    s = u.remain_set(name)
    t1, t2 = open(s.s1, "rb").read(), open(s.s2, "rb").read()
    n = t1.count(b"\n") // 4
    assert n > 100 and t1.split(b"\n")[0].count(b" ") >= 22                      # sorted remain records: 23-token headers, so `prior` is set
    ct, ed = s.d.chr_table, s.P.max_ed
    whole = _both(tmp_path, ct, ed, t1, t2, 1 << 30, "whole")
    assert len(whole) == 2 and whole[0][0] == n and whole[0][-1] is not None and whole[1] is None
    assert whole[0] == _arrays(s.b)                                              # (and both are what the set's own reader gave)
    parts = _both(tmp_path, ct, ed, t1, t2, 97, "parts")                         # several cm_fastq_next calls
    assert len(parts) == (n + 96) // 97 + 1 and sum(p[0] for p in parts[:-1]) == n
    # an empty text
    assert _both(tmp_path, ct, ed, b"", b"", 50, "empty") == [None]
    # the last record without its final line feed
    cut = _both(tmp_path, ct, ed, t1[:-1], t2[:-1], 1 << 30, "nolf")
    assert cut[0] == whole[0]
    # a text cut in the middle of its last record: the same error, in the same call
    r1 = split4(t1)
    mid = b"".join(r1[:-1]) + b"\n".join(r1[-1].split(b"\n")[:2]) + b"\n"
    for max_pairs in (1 << 30, 97):
        bad = _both(tmp_path, ct, ed, mid, t2, max_pairs, f"mid{max_pairs}")
        assert isinstance(bad[-1], str) and "(-1)" in bad[-1], bad[-1]
    # R2 shorter than R1
    bad = _both(tmp_path, ct, ed, t1, b"".join(split4(t2)[:-3]), 1 << 30, "short2")
    assert isinstance(bad[-1], str)
    L = cl.load()
    h = C.c_void_p()
    assert L.cm_fastq_open_mem(None, 5, None, 0, None, 0, 4, C.byref(h)) == CM_EINVAL and not h
    assert L.cm_fastq_open_mem(None, 0, None, 0, None, 0, 4, None) == CM_EINVAL


def mixed_sizes(n):
    out, k = [], 0
    while sum(out) < n:
        out.append(min(GROUP_SIZES[k % len(GROUP_SIZES)], n - sum(out)))
        k += 1
    return out


def _run_of(recs1, recs2):
    keys = [parsed_key(r.split(b"\n")[0]) for r in recs1]
    off = [np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.uint32) if rr else np.zeros(1, np.uint32) for rr in (recs1, recs2)]
    return b"".join(recs1), off[0], b"".join(recs2), off[1], np.array(keys, np.int64)


@pytest.mark.parametrize("cuts", [(), (300,), (0, 1, 1, 200, 201, 650)], ids=["one", "two", "seven"])
def test_memory_finish_equals_file_finish(built, tmp_path, cuts):
    """the runs of test_remain_sorted_cpu (1, 2 and 7 of them, every second one added unsorted): the two buffers are the two files"""
    rng = np.random.default_rng(5)
    t1, t2, st, group = tie_text(rng, mixed_sizes(700), 150)
    n = len(st)
    h = HostRemain(tmp_path, t1, t2, n, tag="runs")
    _, _, s1, s2 = sorted_files(h, st, np.arange(n))
    bounds = [0] + list(cuts) + [n]
    p = [str(tmp_path / f"merged_R{m}.srt") for m in (1, 2)]
    with_files, without = cl.RemainRuns(p[0], p[1]), cl.RemainRuns()
    unsorted_runs = 0
    for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
        c1, c2, r1, r2 = sorted_files(h, st, np.arange(a, b), tag=f"run{k}")
        for runs in (with_files, without):
            if k % 2 or len(bounds) == 2:
                runs.add_unsorted(c1, c2)
            else:
                runs.add(*_run_of(split4(r1), split4(r2)))
        unsorted_runs += 1 if (k % 2 or len(bounds) == 2) else 0
    assert unsorted_runs >= 1
    assert without.finish_mem() == (s1, s2)
    assert without.finish_mem() == (s1, s2)                                      # (made anew by a second call)
    assert without.finish() == CM_EINVAL                                         # opened without paths: no file finish
    assert with_files.finish_mem() == (s1, s2)
    assert with_files.finish() == 0 and open(p[0], "rb").read() == s1 and open(p[1], "rb").read() == s2
    with_files.close()
    without.close()
    h.close()
    L = cl.load()
    assert L.cm_remain_runs_finish_mem(None, None, None, None, None) == CM_EINVAL
    empty = cl.RemainRuns()
    assert empty.finish_mem() == (b"", b"")
    empty.close()
    hh = C.c_void_p()
    assert L.cm_remain_runs_open(b"x", None, C.byref(hh)) == CM_EINVAL and L.cm_remain_runs_open(None, b"x", C.byref(hh)) == CM_EINVAL


def test_detect_struct_mirrors(built):
    L = cl.load()
    two = (C.c_uint32 * 2)()
    assert L.cm_detect_abi_sizes(two, 2) == 2 and list(two) == [C.sizeof(cl.DetectArgs), C.sizeof(cl.DetectStats)]
    assert C.sizeof(cl.DetectArgs) == C.sizeof(cl.MappingArgs) + 16
    assert C.sizeof(cl.DetectStats) == C.sizeof(cl.MappingStats) + C.sizeof(cl.CircStats) + 8 + 3 * 8 + 2 * 8
    assert L.cm_detect_abi_sizes(two, 1) == CM_EINVAL and L.cm_detect_abi_sizes(None, 2) == CM_EINVAL
    got = (C.c_uint32 * 32)()
    assert L.cm_abi_sizes(got, 32) == 19                                         # the old list stays closed


def test_detect_run_refusals(built, tmp_path):
    """no device: CM_ENODEV, a message that names it, and not one output file; world = 2: CM_EINVAL"""
    import torch
    from circminer_amd import synth
    from stage2_util import write_fastq_pair
    d = synth.generate("tiny", n_pairs=50, seed=3)
    src = tmp_path / "in"
    src.mkdir()
    fa = str(src / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    packed, info = cl.pack_genome(fa, 150_000)
    gtf = str(src / "ref.gtf")
    open(gtf, "w").write(d.gtf_text)
    fq1, fq2 = write_fastq_pair(src, d, 50)
    out = tmp_path / "out"
    out.mkdir()
    P = cl.default_params(kmer=20)
    with pytest.raises(RuntimeError, match=r"\(-1\).*world") as e:
        cl.run_detect(packed, gtf, fq1, fq2, str(out / "o"), P, index_info=info, world=2)
    assert e.value.rc == CM_EINVAL and os.listdir(str(out)) == []
    with pytest.raises(RuntimeError, match=r"\(-1\).*handover"):
        cl.run_detect(packed, gtf, fq1, fq2, str(out / "o"), P, index_info=info, handover=2)
    if torch.cuda.is_available():
        return                                                                   # (the runs themselves: tests/test_gpu_detect.py)
    for handover in (0, 1):
        with pytest.raises(RuntimeError, match=r"\(-2\).*no HIP device \(CM_ENODEV\)") as e:
            cl.run_detect(packed, gtf, fq1, fq2, str(out / "o"), P, index_info=info, handover=handover)
        assert e.value.rc == CM_ENODEV and os.listdir(str(out)) == []


def test_call_resident_without_a_context(built):
    L = cl.load()
    P = cl.default_params()
    st = cl.CircStats()
    assert L.cm_circ_call_resident(None, C.byref(P), 0, 0, None, None, None, 0, None, b"x", b"y", C.byref(st)) == CM_EINVAL
    assert not os.path.exists("x") and not os.path.exists("y")
