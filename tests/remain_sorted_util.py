"""Helpers of the sorted remain formatter's tests (test_remain_sorted_cpu.py, test_gpu_remain_sorted.py): the host emulation
(tests/hostemu_remain_order.cpp) built here, pairs laid out in tie groups whose members the comparator has to tell apart at every
place a record has (name, fields, bases, qualities, nowhere), and the project's own host path as the checker -- cm_fastq_next on
files holding the same bytes, cm_write_remain_records with (pair, state) records, then cm_sort_remain on those files.  No name
holds a TAB: the device orders by the key's value, cm_sort_remain by the text's second field."""
import ctypes as C
import os
import subprocess

import numpy as np

from circminer_amd import lib as cl
from fastq_text_util import BASES, text_of
from pam_text_util import CHRS, MAPPED_TYPES, directed_states
from remain_text_util import CM_ELIMIT, CONTIG_VALUES, ROOT, key_value

TIE_CAP = 4096                                                              # cmro::TIE_CAP
STAR_TYPES = (6, 8, 9, 10, 11, 12, 13, -1, 14)


def emu_remain_order(built=None):
    """tests/hostemu_remain_order.cpp as a shared library, built when it is older than what it includes"""
    out_dir = os.path.join(ROOT, "tests", "_hostemu")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libcmemu_remain_order.so")
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", x) for x in ("hostemu_remain_order.cpp", "hostemu_remain.cpp", "hostemu_pam.cpp", "hostemu_sam.cpp", "hostemu_rows.h")] + \
           [os.path.join(csrc, x) for x in ("cm_remain_order.h", "cm_remain_text.h", "cm_pam_text.h", "cm_sam_text.h", "cm_rows_text.h", "cm_fastq_text.h")] + \
           [os.path.join(ROOT, "include", "circminer_hot.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-I", os.path.join(ROOT, "tests"),
                               srcs[0], "-o", so])
    E = C.CDLL(so)
    vp = C.c_void_p
    E.emu_format_remain_sorted.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(cl.ChrInfo), C.c_uint32, C.c_uint64,
                                           C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp, C.POINTER(C.c_uint64), vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]
    E.emu_format_remain_sorted.restype = C.c_int
    E.emu_remain_cmp.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(cl.ChrInfo), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    E.emu_remain_cmp.restype = C.c_int
    return E


def tie_case(rng, sizes, hi=150, long_names=0):
    """(records of R1, records of R2, states, group of every pair) for tie groups of the sizes given; the members of a group are
    scattered over the pairs.  Group 0 has key 0: star forms and, among them, mapped states with gspos == 0; every other group a
    mapped key of its own -- negative, beyond 2^32 and wrapping ones among them (remain_text_util.CONTIG_VALUES, a spos_r1 that
    wraps under its shift).  Member j of a group plays case j % 8 in file 1 and case 7 - j % 8 in file 2, so that the two files
    order a group differently:
      0 the group's own name, state, bases and qualities      4 the name again, another state (group 0: a mapped 0 among stars)
      1 the name + "x" (the name is a prefix)                  5 name and state again, other bases (odd groups: a shorter read)
      2 the name + a byte below 0x20                           6 name, state and bases again, other qualities
      3 the name + a byte above 0x7f                           7 wholly the same record as case 0
    Reads of 0, 1, 150 and hi bases lead the groups' lengths.  long_names: bytes added to every name (the span kernel's direct path)."""
    n = int(sum(sizes))
    perm = rng.permutation(n)
    st = np.zeros(n, cl.MAPPED_DTYPE)
    group = np.zeros(n, np.int64)
    recs = ([None] * n, [None] * n)
    base = directed_states(len(sizes) + 1)
    at = 0
    for g, size in enumerate(sizes):
        members = np.sort(perm[at:at + size])
        at += size
        lead = base[g].copy()
        if g == 0:
            lead["type"] = STAR_TYPES[int(rng.integers(len(STAR_TYPES)))]
        else:
            lead["type"] = MAPPED_TYPES[g % len(MAPPED_TYPES)]
            lead["contig_num"] = CONTIG_VALUES[g % 7]
            lead["chr_id"] = (-1, 0, len(CHRS) - 1, len(CHRS), 1)[g % 5]
            lead["spos_r1"] = g * 100000 + 7
            if g == 3:                                                          # the sum wraps 2^32 under the last chromosome's shift
                lead["spos_r1"], lead["chr_id"] = 4294967295, len(CHRS) - 1
        other = lead.copy()
        if g == 0:
            other["type"], other["contig_num"], other["spos_r1"], other["chr_id"] = MAPPED_TYPES[size % len(MAPPED_TYPES)], 0, 0, (-1, 0)[size % 2]
        else:
            other["epos_r2"] = int(lead["epos_r2"]) ^ 1
        ln = (0, 1, 150, hi)[g] if g < 4 else int(rng.integers(2, hi + 1))
        pad = bytes(rng.integers(ord("a"), ord("z") + 1, long_names).astype(np.uint8)) if long_names else b""
        own = []
        for mate in (0, 1):
            seq = bytes(BASES[rng.integers(0, len(BASES), ln)])
            qual = bytes(rng.integers(33, 74, ln).astype(np.uint8))
            own.append((pad + (b"g%d" % g if mate == 0 else b"h%dm" % g), seq, qual))
        for j, p in enumerate(members):
            p = int(p)
            group[p] = g
            st[p] = other if j % 8 in (3, 4) else lead
            for mate in (0, 1):
                name, seq, qual = own[mate]
                case = j % 8 if mate == 0 else 7 - j % 8
                if case in (1, 2, 3):
                    name = name + (b"x", b"\x01", b"\xfe")[case - 1] + (b"%d" % j if j >= 8 else b"")
                if case == 5 and ln:
                    if g % 2:
                        seq, qual = seq[:ln // 2], qual[:ln // 2]
                    else:
                        seq = seq[:-1] + (b"A" if seq[-1:] != b"A" else b"C")
                if case == 6 and ln:
                    qual = qual[:-1] + (b"!" if qual[-1:] != b"!" else b"#")
                recs[mate][p] = [b"@" + name + (b"/%d" % (mate + 1)) + (b" 1:N:0" if j % 3 == 0 else b""), seq, b"+", qual]
    return recs[0], recs[1], st, group


def tie_text(rng, sizes, hi=150, long_names=0):
    r1, r2, st, group = tie_case(rng, sizes, hi, long_names)
    return text_of(r1), text_of(r2), st, group


def split4(data: bytes):
    """the records of a remain file whose strings hold no line feed: every four lines"""
    lines = data.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[k:k + 4]) + b"\n" for k in range(0, len(lines) - 1, 4)]


def sorted_files(h, states, sel, chrs=None, tag="chk"):
    """the checker: cm_write_remain_records of the pairs `sel`, then cm_sort_remain on either file -> (unsorted 1, unsorted 2,
    sorted 1, sorted 2)"""
    u = h.files(states, sel, chrs=chrs)
    out = []
    for m in (0, 1):
        p = os.path.join(h.dir, f"{tag}_{h._k}_R{m + 1}.fastq")
        open(p, "wb").write(u[m])
        out.append(open(cl.sort_remain(p), "rb").read())
    return u[0], u[1], out[0], out[1]


def parts(rec: bytes):
    """(name, fields, bases, qualities) of a record"""
    hdr, seq, plus, qual, _ = rec.split(b"\n")
    sp = hdr.index(b" ")
    return hdr[1:sp], hdr[sp:], seq, qual


def tie_kinds(sorted_recs, keys):
    """what decided between neighbours of equal key in a sorted file: the set of 'prefix', 'low', 'high', 'name', 'star', 'fields',
    'bases', 'shorter', 'quals', 'identical'"""
    kinds = set()
    for a, b, ka, kb in zip(sorted_recs, sorted_recs[1:], keys, keys[1:]):
        if ka != kb:
            continue
        (na, fa, sa, qa), (nb, fb, sb, qb) = parts(a), parts(b)
        if a == b:
            kinds.add("identical")
        elif na != nb:
            short, long_ = (na, nb) if len(na) < len(nb) else (nb, na)
            if long_.startswith(short):
                x = long_[len(short)]
                kinds.add("low" if x < 0x20 else "high" if x > 0x7f else "prefix")
            else:
                i = next(k for k in range(len(short)) if na[k] != nb[k])
                kinds.add("low" if min(na[i], nb[i]) < 0x20 else "high" if max(na[i], nb[i]) > 0x7f else "name")
        elif fa != fb:
            kinds.add("star" if fa.startswith(b" * ") != fb.startswith(b" * ") else "fields")
        elif sa != sb:
            kinds.add("shorter" if sb.startswith(sa) or sa.startswith(sb) else "bases")
        else:
            kinds.add("quals")
    return kinds


def order_of(unsorted_recs, sorted_recs):
    """the permutation a sorted file is of its unsorted one (identical records in their order)"""
    where = {}
    for i, r in enumerate(unsorted_recs):
        where.setdefault(r, []).append(i)
    taken = {}
    out = []
    for r in sorted_recs:
        k = taken.get(r, 0)
        out.append(where[r][k])
        taken[r] = k + 1
    return out


class EmuSorted:
    """emu_format_remain_sorted over the host parser's arrays of a batch (remain_text_util.Emu holds them)"""

    def __init__(self, E, emu):
        self.E, self.e = E, emu

    def format(self, states, sel, first=0, count=None, caps=None, seed=1, chrs=CHRS, window=0, tie_cap=0):
        e = self.e
        st = np.ascontiguousarray(states, dtype=cl.MAPPED_DTYPE)
        sel = np.ascontiguousarray(sel, dtype=np.uint32)
        cnt = (1 << 64) - 1 if count is None else count
        n_out = max(len(sel) - first, 0) if count is None else count
        table = cl.chr_array(list(chrs))
        got, n_rec, stats, ties = np.zeros(2, np.uint64), C.c_uint64(0), np.zeros(4, np.uint64), np.zeros(3, np.uint32)
        kk = np.full(n_out + 1, -7, np.int64)
        oo = [np.full(n_out + 2, 0xA5A5A5A5, np.uint32) for _ in (0, 1)]
        a = [x.ctypes.data for x in (e.nm[0][0], e.nm[0][1], e.nm[1][0], e.nm[1][1], e.seq1, e.off1, e.seq2, e.off2, e.qual1, e.qual2)]

        def call(b1, c1, b2, c2):
            return self.E.emu_format_remain_sorted(st.ctypes.data, e.n, sel.ctypes.data if len(sel) else None, len(sel), *a, table, len(chrs), first, cnt,
                                                   b1, c1, b2, c2, got.ctypes.data, kk.ctypes.data, oo[0].ctypes.data, oo[1].ctypes.data, C.byref(n_rec),
                                                   stats.ctypes.data, seed, window, tie_cap, ties.ctypes.data)
        if caps is None:
            rc = call(None, 0, None, 0)
            if rc == CM_ELIMIT and not got.any():                                # a tie group above the cap
                return rc, [0, 0], [np.zeros(0, np.uint8)] * 2, kk[:-1], oo, int(n_rec.value), [int(x) for x in stats], [int(x) for x in ties]
            assert rc == (CM_ELIMIT if got.any() else 0), rc
            caps = (int(got[0]), int(got[1]))
        bufs = [np.full(c + 64, 0xA5, np.uint8) for c in caps]
        rc = call(bufs[0].ctypes.data, caps[0], bufs[1].ctypes.data, caps[1])
        assert kk[-1] == -7 and all(o[-1] == 0xA5A5A5A5 for o in oo)
        return rc, [int(x) for x in got], bufs, kk[:-1], [o[:-1] for o in oo], int(n_rec.value), [int(x) for x in stats], [int(x) for x in ties]


def check_sorted(out1, out2, keys, offs, h, states, sel, first=0, count=None, chrs=CHRS):
    """the two files, the keys and the offsets of a sorted call against the checker for the active set `sel`; returns the checker's
    (unsorted records, sorted records) of either file and the sorted keys of the whole set"""
    sel = np.asarray(sel, np.int64)
    count_ = len(sel) - first if count is None else count
    u1, u2, s1, s2 = sorted_files(h, states, sel, chrs=chrs)
    all_keys = sorted(key_value(states[int(p)], chrs) for p in sel)
    want = [split4(s1), split4(s2)]
    for m, out, off in ((0, out1, offs[0]), (1, out2, offs[1])):
        rng_ = want[m][first:first + count_]
        assert out == b"".join(rng_), (m, first, count_)
        if count_:
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rng_])]).tolist(), (m, first, count_)
    if count_:
        assert keys.tolist() == all_keys[first:first + count_]                      # non-decreasing, a permutation of the unsorted call's
    return (split4(u1), split4(u2)), want, all_keys
