"""Shared by tests/test_seed_words_cpu.py and tests/test_gpu_seed_words.py: the host emulation of the seed stage's k-mer word path
(tests/hostemu_seed.cpp), and the read batches the device test seeds."""
import ctypes as C
import os
import subprocess

import numpy as np

from circminer_amd import lib as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_emu_seed():
    out_dir = os.path.join(ROOT, "tests", "_hostemu")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libcmemu_seed.so")
    srcs = [os.path.join(ROOT, "tests", "hostemu_seed.cpp"), os.path.join(ROOT, "circminer_amd", "csrc", "cm_core.h"),
            os.path.join(ROOT, "include", "circminer_hot.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "circminer_amd", "csrc"), srcs[0], "-o", so])
    E = C.CDLL(so)
    vp, pp = C.c_void_p, C.POINTER
    E.seedw_kmer.argtypes = [vp, C.c_int, C.c_int, vp]
    E.seedw_kmer.restype = None
    E.seedw_sweep.argtypes = [C.c_uint64, C.c_int, vp]
    E.seedw_sweep.restype = C.c_longlong
    E.seedw_each_position.argtypes = [C.c_uint64, vp]
    E.seedw_each_position.restype = C.c_longlong
    E.seedw_seed_batch.argtypes = [pp(cl.Params), pp(cl.IndexView), pp(cl.Reads), C.c_uint32, C.c_int, vp, vp, vp, vp, vp]
    E.seedw_seed_batch.restype = C.c_int
    return E


MIXED_LENGTHS = (19, 20, 21, 39, 40, 41, 59, 60, 61, 150)


def mixed_batch(d, k, ends, n=512, seed=5):
    """n pairs cut from the pairs of data set d (reads drawn from its genome) to the lengths of MIXED_LENGTHS: the first read of
    either buffer is one seed long and the last ends with a seed, so the k-mer loads of both reach into the slack around the reads;
    the byte offsets of both mates take every residue mod 8; some reads are lower-cased; some carry an N at the first, a middle or
    the last base of a seed.  ends: the pairs of d that the first read of either mate and the last read of either mate are cut from (the caller
    picks reads whose seeds there are found, so that a wrong load next to the slack shows).  Returns (ReadBatch, len1, len2)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, d.seq1.shape[0], n)
    src = np.stack([src, src])                          # per mate
    src[0, 0], src[1, 0], src[0, -1], src[1, -1] = ends
    L = np.array(MIXED_LENGTHS)
    l1, l2 = L[rng.integers(0, len(L), n)], L[rng.integers(0, len(L), n)]
    l1[0] = l2[0] = k                                   # the first read: its reverse-strand span begins in front of the buffer
    l1[-1] = l2[-1] = 3 * k                             # the last read: the span of its last forward seed ends behind the buffer
    s1, s2 = [], []
    for i in range(n):
        for mate, (out, ln) in enumerate(((s1, l1[i]), (s2, l2[i]))):
            r = (d.seq1, d.seq2)[mate][src[mate, i], :ln].copy()
            kind = (i + 3 * mate) % 16 if 0 < i < n - 1 else 0
            if kind == 5:
                r = np.frombuffer(bytes(r).lower(), np.uint8).copy()
            elif kind == 6 and ln >= 2 * k:
                r[k:2 * k] |= 0x20                      # one seed in lower case
            elif kind in (7, 8, 9) and ln >= k:
                s = int(rng.integers(0, ln // k))       # N at the first / a middle / the last base of seed s
                r[s * k + (0, k // 2, k - 1)[kind - 7]] = ord("N")
            out.append(r)
    b = cl.ReadBatch(np.concatenate(s1), np.concatenate(s2), l1, l2)
    assert set(int(x) % 8 for x in b.off1[:-1]) == set(range(8)) and set(int(x) % 8 for x in b.off2[:-1]) == set(range(8))
    return b, l1, l2
