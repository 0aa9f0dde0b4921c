"""The device-side remain formatter without a device: the bodies of circminer_amd/csrc/cm_remain_text.h and the plan of
cm_rows_text.h run by a host emulation (tests/hostemu_remain.cpp, tests/hostemu_rows.h: shuffled items, spans and lanes, every write
of every call caught in shadow buffers and counted) against the project's own host writer -- cm_fastq_next on files holding the same
bytes, then cm_write_remain_records with the same (pair, state) records -- and against a plain restatement of the format."""
import ctypes as C
import os

import numpy as np
import pytest

from circminer_amd import lib as cl
from pam_text_util import CHRS, MAPPED_TYPES
from remain_text_util import (CM_EINVAL, CM_ELIMIT, CM_ESTATE, ROOT, SPAN_RECS, WINDOW, Emu, HostRemain, emu_remain, gspos_of, key_value, parsed_key,
                              plain_record, remain_pair_text, remain_states, selections, split_records)

N_MANY = 4100


@pytest.fixture(scope="module")
def emu_rem(built):
    return emu_remain()


def _check(e, h, st, sel, first=0, count=None, chrs=CHRS, **kw):
    """the emulated records of a range of a selection == the host writer's, in both files; every byte written once; the keys are
    the values of the states"""
    sel = np.asarray(sel, np.int64)
    count_ = len(sel) - first if count is None else count
    rc, got, bufs, keys, n_rec, stats, writes = e.format(st, sel, first, count, chrs=chrs, **kw)
    want = h.files(st, sel[first:first + count_], chrs=chrs)
    assert rc == 0 and n_rec == len(sel) and got == [len(want[0]), len(want[1])], (first, count, got, [len(x) for x in want])
    for m in (0, 1):
        assert bufs[m][:got[m]].tobytes() == want[m] and bool((bufs[m][got[m]:] == 0xA5).all()), (m, first, count)
    if count_:
        assert writes == [1, 1], writes
        assert keys.tolist() == [key_value(st[int(p)], chrs) for p in sel[first:first + count_]]
        assert stats[0] == 2 * count_ and stats[1] == sum(got) and stats[2] + stats[3] == 2 * ((count_ + SPAN_RECS - 1) // SPAN_RECS)
    else:
        assert stats == [0, 0, 0, 0] and got == [0, 0]
    return want, stats


@pytest.mark.parametrize("n", [1, 63, 64, 65, N_MANY])
def test_emulated_records_equal_the_host_writer(emu_rem, tmp_path, n):
    rng = np.random.default_rng(n)
    st = remain_states(n)
    long_run = (n // 2, min(n, n // 2 + 40)) if n > 16 else None              # names of 300 - 400 bytes in both files: spans that cross the window
    t1, t2 = remain_pair_text(rng, n, long_run, hi=300)
    h = HostRemain(tmp_path, t1, t2, n)
    e = Emu(emu_rem, h)
    paths = [0, 0]
    for tag, sel in selections(rng, n).items():
        for states in ((st,) if tag != "all" else (st, np.zeros(n, cl.MAPPED_DTYPE))):
            want, stats = _check(e, h, states, sel, seed=n + 1)
            paths = [paths[0] + stats[2], paths[1] + stats[3]]
            if tag in ("all", "third") or n < N_MANY:
                _, stats = _check(e, h, states, sel, seed=n + 2, window=1)       # every span direct
                assert stats[2] == 0
                _check(e, h, states, sel, seed=n + 3, window=3000)                # a small window: the paths split elsewhere
    if n == N_MANY:
        assert paths[0] > 0 and paths[1] > 0                                     # both paths of the span body under the device's window
    # the whole batch again: the plain restatement, the keys as `sort -k2,2n` reads them, what the directed states reach
    sel = np.arange(n)
    want, _ = _check(e, h, st, sel, seed=5)
    n1, n2 = h.names(), h.names2()
    for m, names, off, seq, qual in ((0, n1, e.off1, e.seq1, e.qual1), (1, n2, e.off2, e.seq2, e.qual2)):
        lens = np.diff(off.astype(np.int64))
        recs = split_records(want[m], lens)
        for i, (hdr, s, q) in enumerate(recs):
            a, b = int(off[i]), int(off[i + 1])
            assert hdr + b"\n" + s + b"\n+\n" + q + b"\n" == plain_record(names[i], st[i], seq[a:b].tobytes(), qual[a:b].tobytes(), CHRS), (m, i)
            if m == 0 and b" " not in names[i] and b"\t" not in names[i]:        # (a name with a blank moves the text's second field)
                assert parsed_key(hdr) == key_value(st[i], CHRS), (i, hdr)
    if n == N_MANY:
        types = set(st["type"].tolist())
        assert set(range(14)) <= types and {-1, 14} <= types
        for t in types:                                                          # every type meets every contig_num, both forms
            assert len(set(st["contig_num"][st["type"] == t].tolist())) == 7
        mapped = np.isin(st["type"], MAPPED_TYPES)
        wraps = mapped & (st["spos_r1"] == 4294967295) & (st["chr_id"] == len(CHRS) - 1) & (np.abs(st["contig_num"].astype(np.int64)) < 100)
        assert wraps.any() and all(gspos_of(st[i], CHRS) - int(st[i]["contig_num"]) * 1_100_000_000 == CHRS[-1][2] - 1 for i in np.flatnonzero(wraps))
        g = [gspos_of(st[i], CHRS) for i in np.flatnonzero(mapped)]
        assert min(g) < -2 ** 61 and max(g) > 2 ** 61                            # contig_num INT32_MIN / INT32_MAX: 20 bytes of key
        assert any(n1[i] != n2[i] for i in range(n)) and b"" in n2 and b"mu" in n2 and b"nu" in n1
        assert {0, 1, 150, 300} <= set(np.diff(e.off1.astype(np.int64)).tolist()) and {0, 1, 150, 300} <= set(np.diff(e.off2.astype(np.int64)).tolist())
    # ranges that cut a span, an empty one, one at the end, "to the end"
    for tag, sel in selections(rng, n).items():
        k = len(sel)
        for first, count in ((0, 0), (k, 0), (k, None), (max(k - 1, 0), min(k, 1)), (k // 3, None), (min(SPAN_RECS - 1, k), min(2, k - min(SPAN_RECS - 1, k))),
                             (0, min(k, SPAN_RECS + 1)), (k // 2, min(k - k // 2, 70))):
            _check(e, h, st, sel, first, count, seed=first + 11)
    # a cap that is too small, of either file: the needed sizes, and nothing written
    sel = np.arange(n)
    want = h.files(st, sel)
    sizes = [len(want[0]), len(want[1])]
    for caps in ((sizes[0] - 1, sizes[1]), (sizes[0], sizes[1] - 1), (0, 0), (sizes[0] // 2, sizes[1] + 5)):
        rc, got, bufs, keys, n_rec, stats, _ = e.format(st, sel, caps=caps)
        assert rc == CM_ELIMIT and got == sizes and n_rec == n and stats == [0, 0, 0, 0] and all(bool((b == 0xA5).all()) for b in bufs) and bool((keys == -7).all())
    assert e.format(st, sel, caps=sizes)[:2] == (0, sizes)
    # refusals of the range: beyond the set
    for first, count in ((n, 1), (0, n + 1), (n + 1, 0), (n + 1, None)):
        rc, got, _, _, n_rec, _, _ = e.format(st, sel, first, count, caps=(10, 10))
        assert rc == CM_EINVAL and got == [0, 0] and n_rec == n
    h.close()


def test_emulated_records_without_a_chromosome_table(emu_rem, tmp_path):
    """n_chr = 0: every chromosome prints '-' and no shift enters the key"""
    n = 23 * 7 + 9
    st = remain_states(n)
    t1, t2 = remain_pair_text(np.random.default_rng(3), n)
    h = HostRemain(tmp_path, t1, t2, n, chrs=[])
    e = Emu(emu_rem, h)
    want, _ = _check(e, h, st, np.arange(n), chrs=[])
    assert b" - " in want[0] and b" - " in want[1]
    h.close()


@pytest.mark.parametrize("n", [1, 64, 700])
def test_r2_names_and_qualities_through_the_tokeniser_emulation(emu_rem, tmp_path, n):
    """the names of both files by k_ft_name_len / k_ft_name_copy's bodies and the qualities by k_ft_qual_copy's, out of the text ==
    the host parser's; the records formatted from them == the host writer's"""
    rng = np.random.default_rng(100 + n)
    long_run = (n // 2, n // 2 + 40) if n > 100 else None
    t1, t2 = remain_pair_text(rng, n, long_run, hi=300)
    h = HostRemain(tmp_path, t1, t2, n)
    kept = []
    for text, want in ((t1, h.names()), (t2, h.names2())):
        a = np.frombuffer(text, np.uint8)
        names, off = np.full(len(text) + 1, 0xA5, np.uint8), np.zeros(n + 1, np.uint32)
        assert emu_rem.emu_names(a.ctypes.data, len(text), n, n + 7, names.ctypes.data, off.ctypes.data) == 0
        assert [names[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)] == want and bool((names[int(off[n]):] == 0xA5).all())
        kept.append((names, off))
    _, off1, _, off2, q1, q2 = h.arrays()
    quals = []
    for text, off, want in ((t1, off1, q1), (t2, off2, q2)):
        a = np.frombuffer(text, np.uint8)
        q = np.full(int(off[n]) + 1, 0xA5, np.uint8)
        assert emu_rem.emu_quals(a.ctypes.data, len(text), n, off.ctypes.data, n, q.ctypes.data) == 0
        assert np.array_equal(q[:-1], want) and q[-1] == 0xA5
        quals.append(q)
    if n == 700:
        n1, n2 = h.names(), h.names2()
        assert sum(a != b for a, b in zip(n1, n2)) > n // 2 and b"" in n1 and b"" in n2 and b"mu" in n2 and b"same" in n2 and b"a/b" in n2
        assert max(len(x) for x in n2) >= 300
    e = Emu(emu_rem, h, names=kept[0], names2=kept[1], quals=quals)
    for tag, sel in selections(rng, n).items():
        _, stats = _check(e, h, remain_states(n), sel, seed=n)
        if n == 700 and tag == "all":
            assert stats[2] > 0 and stats[3] > 0                                 # the run of long names went direct
    h.close()


def test_a_batch_without_its_kept_arrays_is_refused(emu_rem, tmp_path):
    n = 5
    t1, t2 = remain_pair_text(np.random.default_rng(1), n)
    h = HostRemain(tmp_path, t1, t2, n)
    e = Emu(emu_rem, h)
    st, table = remain_states(n), cl.chr_array(CHRS)
    got, n_rec = np.zeros(2, np.uint64), C.c_uint64(77)
    sel = np.arange(n, dtype=np.uint32)
    a = [x.ctypes.data for x in (e.nm[0][0], e.nm[0][1], e.nm[1][0], e.nm[1][1], e.seq1, e.off1, e.seq2, e.off2, e.qual1, e.qual2)]
    for missing in (1, 3, 8, 9):                                                 # name_off1, name_off2, qual1, qual2
        b = list(a)
        b[missing] = None
        rc = emu_rem.emu_format_remain(st.ctypes.data, n, sel.ctypes.data, n, *b, table, len(CHRS), 0, n, None, 0, None, 0, got.ctypes.data, None, C.byref(n_rec), None, 1, 0, None)
        assert rc == CM_ESTATE and n_rec.value == n and not got.any()
    rc = emu_rem.emu_format_remain(st.ctypes.data, 0, None, 0, *a, table, len(CHRS), 0, 0, None, 0, None, 0, got.ctypes.data, None, C.byref(n_rec), None, 1, 0, None)
    assert rc == CM_ESTATE and n_rec.value == 0
    rc = emu_rem.emu_format_remain(st.ctypes.data, n, sel.ctypes.data, n, *a, table, len(CHRS), 0, n, None, 5, None, 0, got.ctypes.data, None, C.byref(n_rec), None, 1, 0, None)
    assert rc == CM_EINVAL                                                       # a null output with a cap
    h.close()


def test_write_bytes2_is_a_plain_write_to_the_second_file(built, tmp_path):
    rng = np.random.default_rng(8)
    pieces = [bytes(rng.integers(0, 256, k).astype(np.uint8)) for k in (0, 1, 4095, 70000, 5 << 20, 3, 0, 4 << 20, 17)]
    p1, p2 = str(tmp_path / "a_R1"), str(tmp_path / "a_R2")
    w = cl.RecordWriter(p1, p2, CHRS)
    for k, x in enumerate(pieces):
        w.write_bytes2(x)
        if k % 2:
            w.write_bytes(x[::-1])
    w.close()
    assert open(p2, "rb").read() == b"".join(pieces) and open(p1, "rb").read() == b"".join(x[::-1] for x in pieces[1::2])
    w = cl.RecordWriter(p1, None, CHRS)                                          # a writer without a second file
    assert w.L.cm_write_bytes2(w.h, None, 0) == CM_EINVAL
    with pytest.raises(RuntimeError):
        w.write_bytes2(b"x")
    w.write_bytes(b"kept")
    w.close()
    assert open(p1, "rb").read() == b"kept"
    w = cl.RecordWriter(p1, p2, CHRS)
    assert w.L.cm_write_bytes2(w.h, None, 3) == CM_EINVAL and w.L.cm_write_bytes2(None, b"abc", 3) == CM_EINVAL
    w.close()


def test_the_constants_are_the_headers():
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    text = open(os.path.join(csrc, "cm_remain_text.h")).read()
    assert f"SPAN_RECS = {SPAN_RECS};" in text and '#define CMRM_STARS " * * * * * * * * * * * * * * * * * * * *"' in text
    assert f"WINDOW = {WINDOW};" in open(os.path.join(csrc, "cm_rows_text.h")).read()
    assert "1100000000u" in open(os.path.join(ROOT, "include", "circminer_hot.h")).read()
