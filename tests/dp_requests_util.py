"""Requests for the DP test hook (cm_dp_batch on the device, emu_dp_batch in the host emulation) and what the oracle answers.

A request is one call of one_side_banded (kind 0), local_alignment_side (kind 1) or local_alignment_sc (kind 2) of
circminer_amd/csrc/cm_core.h on two views into a byte arena.  Everything here is laid out in READ SPACE first: `sv` / `tv` are
the strings in the order the DP walks them (for a left extension that is the reverse of what the oracle is handed, the convention
of emu_edit_side / emu_drop_sc in tests/hostemu.cpp).  Each string then gets 64 bytes (CM_STAGE_PAD) on either side in the
arena, and those pads are bait, not filler: behind the last character of a view comes the continuation that would keep matching
the other string, so a compare or a staging load that runs one character too far changes the answer.

The reference of a request is the oracle (oracle_one_side / oracle_edit_side / oracle_drop_sc, pinned by brute force in
test_oracle.py) on the materialised strings, with err == 0; for strings longer than the staging buffers that do not take a
closed form it is the wrapper's documented return (cm_core.h, `dp_fits` callers):
    one_side_banded       :1415   ret = max_ed + 1
    local_alignment_side  :1426   ret = max_ed + 1, indel = band + 1, score = -(max_ed + 1)
    local_alignment_sc    :1538   ret = max_ed + 1, sc_len = max(max_sc, m) + 1, indel = band + 1, score = 0
each with ERR_BAND (8) in the request's err word (dp_fits, :1402-1406).
"""
import ctypes as C

import numpy as np

from circminer_amd import lib as cl
from oracle import oracle_py as op

PAD = 64
ERR_BAND = 8
ACGT = np.frombuffer(b"ACGT", np.uint8)
PARAM_SETS = ((3, 4), (2, 4), (5, 8))                      # (band, max_ed)
FILLS = (0x00000000, 0x45454545)                           # eight matching 'A' codes per word / the two "other" codes alternating
ALPHABETS = (b"ACGT", b"AC", b"A", b"AAC", b"ACGTACGA")    # test_xdrop_long_prefixes_and_low_complexity
# device views of (s, t) before a left extension turns them round: both forward; t complemented-reversed (Read::view() of an rc
# read); both reversed; s reversed and t complemented forward (what .rev() makes of the second)
VIEW_CONFIGS = (((1, 0), (1, 0)), ((1, 0), (-1, 1)), ((-1, 0), (-1, 0)), ((-1, 0), (1, 1)))

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMP[_a] = _b


_OTHER = np.arange(256, dtype=np.uint8)                   # a base that is not this one
for _a, _b in zip(b"ACGT", b"CGTA"):
    _OTHER[_a] = _b


def _valid(x):
    u = x & 0xDF
    return (u == 65) | (u == 67) | (u == 71) | (u == 84)


def same_prefix(a, b, k):
    """the first k characters of a and b are the same bases (case-insensitive; anything but ACGT never matches)"""
    if k > len(a) or k > len(b):
        return False
    x, y = a[:k], b[:k]
    return bool((((x & 0xDF) == (y & 0xDF)) & _valid(x)).all())


class LR:
    """one logical request, in read space"""
    __slots__ = ("kind", "sv", "tv", "arg", "left", "vc", "cont_s", "cont_t", "nul_s", "tag")

    def __init__(self, kind, sv, tv, arg=0, left=0, vc=0, cont_s=None, cont_t=None, nul_s=False, tag=""):
        self.kind, self.arg, self.left, self.vc, self.nul_s, self.tag = kind, arg, left, vc, nul_s, tag
        self.sv = np.ascontiguousarray(sv, dtype=np.uint8)
        self.tv = np.ascontiguousarray(tv, dtype=np.uint8)
        self.cont_s, self.cont_t = cont_s, cont_t


class Batch:
    def __init__(self, P, str_cap, lrs, arena, req, exp):
        self.P, self.str_cap, self.lrs, self.arena, self.req, self.exp = P, str_cap, lrs, arena, req, exp

    def __len__(self):
        return len(self.req)

    def subset(self, idx):
        idx = np.asarray(idx)
        return Batch(self.P, self.str_cap, [self.lrs[i] for i in idx], self.arena, self.req[idx].copy(), self.exp[idx].copy())

    def kind2(self):
        return self.subset(np.flatnonzero(self.req["kind"] == 2))

    def describe(self, i):
        q, r = self.req[i], self.lrs[i]
        return (f"request {i} [{r.tag}] kind {q['kind']} arg {q['arg']} left {r.left} band {self.P.band} max_ed {self.P.max_ed} str_cap {self.str_cap}\n"
                f"  s view off {q['s_off']} step {q['s_step']} mode {q['s_mode']} n {q['n']}\n"
                f"  t view off {q['t_off']} step {q['t_step']} mode {q['t_mode']} m {q['m']}\n"
                f"  s (read space) {bytes(r.sv)!r}{' (all NUL on the device)' if r.nul_s else ''}\n  t (read space) {bytes(r.tv)!r}\n"
                f"  expected (ret, sc_len, indel, score, err) {tuple(int(x) for x in self.exp[i])}")

    def first_mismatch(self, got):
        """None, or a printable reproducer of the first request whose five result fields differ from the oracle's"""
        bad = np.flatnonzero(got.view(np.int32).reshape(-1, 5) != self.exp.view(np.int32).reshape(-1, 5)) // 5
        if len(bad) == 0:
            return None
        i = int(bad[0])
        return f"{len(np.unique(bad))} of {len(self)} requests differ; first:\n{self.describe(i)}\n  got {tuple(int(x) for x in got[i])}"


def expected_one(O, P, str_cap, r):
    """(ret, sc_len, indel, score, err) of a logical request: the oracle, or the documented over-capacity return"""
    sv = np.zeros(len(r.sv), np.uint8) if r.nul_s else r.sv
    tv = r.tv
    n, m = len(sv), len(tv)
    fits = n <= str_cap and m <= str_cap
    if r.kind == 0:
        w = r.arg
        closed = (w == 0 and m == n) or (w > 0 and n > w and m == n + w and same_prefix(sv, tv, n))
        if not fits and not closed:
            return (P.max_ed + 1, 0, 0, 0, ERR_BAND)
        return (O.oracle_one_side(sv.ctypes.data, n, tv.ctypes.data, m, w), 0, 0, 0, 0)
    closed = m >= 1 and n >= m and same_prefix(sv, tv, m)
    sf, tf = (np.ascontiguousarray(sv[::-1]), np.ascontiguousarray(tv[::-1])) if r.left else (sv, tv)
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    if r.kind == 1:
        if not fits and not closed:
            return (P.max_ed + 1, 0, P.band + 1, -(P.max_ed + 1), ERR_BAND)
        ret = O.oracle_edit_side(C.byref(P), sf.ctypes.data, n, tf.ctypes.data, m, r.left, C.byref(b), C.byref(c))
        return (ret, 0, b.value, c.value, 0)
    if not fits and not closed:
        return (P.max_ed + 1, max(P.max_sc, m) + 1, P.band + 1, 0, ERR_BAND)
    ret = O.oracle_drop_sc(C.byref(P), sf.ctypes.data, n, tf.ctypes.data, m, r.left, C.byref(a), C.byref(b), C.byref(c))
    return (ret, a.value, b.value, c.value, 0)


def build(P, str_cap, lrs, seed=0):
    """arena + requests + the oracle's answers for the logical requests `lrs`"""
    O = op.load()
    rng = np.random.default_rng(1000 + seed)
    chunks, pos = [], 0
    req = np.zeros(len(lrs), cl.DP_REQ_DTYPE)
    exp = np.zeros(len(lrs), cl.DP_RES_DTYPE)
    fill = ACGT[rng.integers(0, 4, 1 << 16)]              # valid bases for the parts of a pad nothing is planted in
    fpos = 0

    def filler(k):
        nonlocal fpos
        if fpos + k > len(fill):
            fpos = 0
        fpos += k
        return fill[fpos - k:fpos]

    def place(core, cont, step, mode):
        nonlocal pos
        cont = cont[:PAD]
        e = np.concatenate([filler(PAD), core, cont, filler(PAD - len(cont))])
        if step < 0:
            e = e[::-1]
        if mode == 1:
            e = _COMP[e]
        chunks.append(e)
        off = pos + PAD if step > 0 else pos + PAD + len(core) - 1
        pos += len(e)
        return off

    for i, r in enumerate(lrs):
        n, m = len(r.sv), len(r.tv)
        (ss, sm_), (ts, tm) = VIEW_CONFIGS[r.vc]
        turn = -1 if (r.kind == 2 and r.left) else 1      # kind 2: the caller hands over views already turned round
        ss, ts = ss * turn, ts * turn
        s_off = place(r.sv, r.tv[n:] if r.cont_s is None else r.cont_s, ss, sm_)
        t_off = place(r.tv, r.sv[m:] if r.cont_t is None else r.cont_t, ts, tm)
        if r.kind == 1 and r.left:                        # kind 1: the wrapper turns the views round itself (SV::rev)
            s_off, ss = s_off + (n - 1) * ss, -ss
            t_off, ts = t_off + (m - 1) * ts, -ts
        req[i] = (r.kind, s_off, ss, 2 if r.nul_s else sm_, n, t_off, ts, tm, m, r.left if r.kind == 1 else r.arg)
        exp[i] = expected_one(O, P, str_cap, r)
    arena = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    return Batch(P, str_cap, list(lrs), np.ascontiguousarray(arena), req, exp)


# ---------------------------------------------------------------------------------------------------------------------- families
SUBS = (0, 0, 1, 2, 4, 1, 1, 9)


def mutate(rng, t, case, band, alpha=ACGT):
    """family (a)'s cases: s = t with SUBS[case] substitutions, one base deleted (cases 5, 7) and / or inserted (6, 7), extended with
    random bases and cut to len(t) + band"""
    s = t.copy()
    for _ in range(SUBS[case]):
        s[int(rng.integers(0, len(s)))] = alpha[rng.integers(0, len(alpha))]
    if case in (5, 7) and len(s) > 1:
        s = np.delete(s, int(rng.integers(0, len(s))))
    if case in (6, 7):
        s = np.insert(s, int(rng.integers(0, len(s) + 1)), alpha[rng.integers(0, len(alpha))])
    return np.concatenate([s, alpha[rng.integers(0, len(alpha), band + 2)]])[:len(t) + band]


def family_a(band, n_pairs=4096, seed=11):
    """random pairs: each as kind 2, as kind 1 where n > m, plus one kind-0 draw of test_dp_bodies_fuzz"""
    rng = np.random.default_rng(seed + band)
    out = []
    for i in range(n_pairs):
        m = int(rng.integers(1, 141))
        t = ACGT[rng.integers(0, 4, m)].copy()
        s = mutate(rng, t, i % 8, band)
        if rng.random() < 0.1:
            s[int(rng.integers(0, len(s)))] = ord("N")
        if rng.random() < 0.1:
            t[int(rng.integers(0, m))] = ord("n")
        if rng.random() < 0.1:
            t = t | 0x20
        left, vc = int(rng.integers(0, 2)), int(rng.integers(0, 3))
        # read space: half of the left extensions walk the pair as it is (a DP over the whole length in either direction), the other
        # half get it turned round as test_dp_bodies_fuzz does -- the surplus of s comes first, the alignment is shifted by the band
        # or the X-drop ends within a few anti-diagonals
        sv, tv = (s[::-1], t[::-1]) if left and rng.random() < 0.5 else (s, t)
        out.append(LR(2, sv, tv, 0, left, vc, tag=f"a pair {i} case {i % 8}"))
        if len(s) > m:
            out.append(LR(1, sv, tv, 0, left, vc, tag=f"a pair {i} case {i % 8}"))
        w, n3 = int(rng.integers(0, band + 1)), int(rng.integers(0, 60))
        s3 = ACGT[rng.integers(0, 4, n3)]
        t3 = np.concatenate([s3, ACGT[rng.integers(0, 4, w)]])
        if rng.random() < 0.5 and n3:
            t3[int(rng.integers(0, n3))] = ACGT[rng.integers(0, 4)]
        out.append(LR(0, s3, t3, w, 0, vc, tag=f"a pair {i} one-sided"))
    return out


B_LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49)


def family_b(band, seed=21):
    """tail masks of the closed forms: compare length L, two strings equal but for ONE place p (p < L: a request per p; p = L ..
    L + 15: beyond the compare length, the closed form must still be taken), N against N, lower against upper case.  Each as kind 2
    (n = L + 16, m = L) forward and left, and kind 0 with w = 0 (n = m = L) and w = band (n = L, m = L + band)."""
    rng = np.random.default_rng(seed + band)
    out = []

    def emit(A, B, L, tag):
        # each string is followed by its OWN continuation: a place p >= L where A and B differ lies inside s (kind 2) or in the pad
        # behind a view, where a compare without its tail mask finds it
        for left in (0, 1):
            out.append(LR(2, A[:L + 16], B[:L], 0, left, int(rng.integers(0, 4)), cont_s=A[L + 16:], cont_t=B[L:], tag=tag))
        out.append(LR(0, A[:L], B[:L], 0, 0, int(rng.integers(0, 4)), cont_s=A[L:], cont_t=B[L:], tag=tag + " hamming"))
        out.append(LR(0, A[:L], B[:L + band], band, 0, int(rng.integers(0, 4)), cont_s=A[L:], cont_t=B[L + band:], tag=tag + " w=band"))

    for L in B_LENGTHS:
        def fresh():
            return ACGT[rng.integers(0, 4, L + 16 + PAD)].copy()
        A = fresh()
        emit(A, A.copy(), L, f"b L {L} equal")
        emit(A, A | 0x20, L, f"b L {L} lower against upper")
        for p in range(L + 16):
            A = fresh()
            B = A.copy()
            B[p] = ACGT[(int(np.flatnonzero(ACGT == A[p])[0]) + 1 + int(rng.integers(0, 3))) % 4]
            emit(A, B, L, f"b L {L} first difference at {p}")
        for p in sorted({0, L // 2, L - 1}):
            A = fresh()
            A[p] = ord("N")
            emit(A, A.copy(), L, f"b L {L} N against N at {p}")
    for n in (143, 144, 145, 300):                         # Hamming beyond the buffers: no dp_fits on that path, the count is exact
        for p in (None, 0, 142, 143, 144, n - 1, n):       # (p = n: the difference sits in the pad)
            A = ACGT[rng.integers(0, 4, n + PAD)].copy()
            B = A.copy()
            if p is not None:
                B[p] = ACGT[(int(np.flatnonzero(ACGT == A[p])[0]) + 1) % 4]
                if p + 7 < n:
                    B[p + 7] = ord("N")
            out.append(LR(0, A[:n], B[:n], 0, 0, int(rng.integers(0, 4)), cont_s=A[n:], cont_t=B[n:], tag=f"b hamming n {n} difference at {p}"))
    return out


def family_c(band, cap, seed=31, reps=2):
    """strings that end at, or just below, the capacity of the staging buffers: n in {cap - 9, cap - 8, cap - 7, cap - 1, cap}, m = n - band
    (kind 2 also m = n; kind 0: the longer string is the one of n characters), real DPs (family (a)'s cases), differences within
    the last 8 characters of both strings, and strings whose last 8 characters are the only ones that match"""
    rng = np.random.default_rng(seed + cap)
    out = []
    for n in (cap - 9, cap - 8, cap - 7, cap - 1, cap):
        for m in (n - band, n):
            if m < 0 or n < 0:
                continue                                   # (cap = 8 has no such string)
            variants = []
            for case in (2, 3, 4, 5, 6, 7):
                for _ in range(reps):
                    t = ACGT[rng.integers(0, 4, m)].copy()
                    s = mutate(rng, t, case, n - m) if m else ACGT[rng.integers(0, 4, n)].copy()
                    s = np.concatenate([s, ACGT[rng.integers(0, 4, n)]])[:n]
                    variants.append((s, t, f"case {case}"))
            for _ in range(reps):                          # differences within the last 8 characters of both
                t = ACGT[rng.integers(0, 4, m)].copy()
                s = np.concatenate([t, ACGT[rng.integers(0, 4, n - m)]])
                for x in (s, t):
                    for _k in range(int(rng.integers(1, 3))):
                        if len(x):
                            p = len(x) - 1 - int(rng.integers(0, min(8, len(x))))
                            x[p] = ACGT[(int(np.flatnonzero(ACGT == x[p])[0]) + 1) % 4]
                variants.append((s, t, "differences in the last 8"))
                t = ACGT[rng.integers(0, 4, m)].copy()      # only the last 8 match
                s = ACGT[rng.integers(0, 4, n)].copy()
                k = min(8, m)
                if k:
                    s[m - k:m] = t[m - k:]
                variants.append((s, t, "only the last 8 match"))
            for s, t, what in variants:
                for left in (0, 1):
                    vc = int(rng.integers(0, 4))
                    sv, tv = s, t
                    tag = f"c cap {cap} n {n} m {m} {what}"
                    out.append(LR(2, sv, tv, 0, left, vc, tag=tag))
                    if m == n - band:
                        out.append(LR(1, sv, tv, 0, left, vc, tag=tag))
                        if not left:
                            out.append(LR(0, t, s, band, 0, vc, tag=tag + " one-sided"))      # (n_s = m, m_t = n = n_s + band)
    return out


def family_d(band, cap, seed=41):
    """one character more than the staging buffers hold, on either side: with a mismatch the wrapper's documented return and
    ERR_BAND, with s[:m] == t the closed form (it comes before dp_fits) and no error"""
    rng = np.random.default_rng(seed + cap)
    out = []
    for n, m in ((cap + 1, cap + 1 - band), (cap + 1, cap + 1), (cap + 1 + band, cap + 1), (cap + 1, 20), (cap, cap + 1)):
        for equal in (True, False):
            for left in (0, 1):
                t = ACGT[rng.integers(0, 4, m)].copy()
                s = np.concatenate([t, ACGT[rng.integers(0, 4, max(n - m, 0))]])[:n]
                if not equal:
                    p = int(rng.integers(0, min(n, m)))
                    s[p] = ACGT[(int(np.flatnonzero(ACGT == s[p])[0]) + 1) % 4]
                vc = int(rng.integers(0, 4))
                tag = f"d cap {cap} n {n} m {m} {'equal' if equal else 'one mismatch'}"
                # behind t comes what does NOT match the rest of s: a compare that runs past m misses the closed form, and here,
                # beyond the buffers, no DP stands in for it
                rest = np.concatenate([s[m:], ACGT[rng.integers(0, 4, PAD)]])[:PAD]
                bait = _OTHER[rest]
                out.append(LR(2, s, t, 0, left, vc, cont_s=rest[max(n - m, 0):], cont_t=bait, tag=tag))
                out.append(LR(1, s, t, 0, left, vc, cont_s=rest[max(n - m, 0):], cont_t=bait, tag=tag))
                if n == m + band and not left:
                    out.append(LR(0, t, s, band, 0, vc, cont_s=bait, cont_t=rest[n - m:], tag=tag + " one-sided"))
                if n == m and not left:
                    out.append(LR(0, t, s, 0, 0, vc, tag=tag + " hamming"))
    return out


def family_e(band, seed=51):
    """degenerate requests: empty strings, n < m, the tiny full DPs (kind 0 with n <= w, kind 1 with n <= 2w or m <= w), an all-NUL
    reference window, and low-complexity alphabets (ties between the diagonal and shifted alignments)"""
    rng = np.random.default_rng(seed + band)
    out = []

    def rnd(k, alpha=ACGT):
        return alpha[rng.integers(0, len(alpha), k)].copy()

    for n, m in ((0, 0), (0, 1), (1, 0), (0, 7), (7, 0), (1, 1), (2, 9), (5, 30), (30, 40), (60, 64)):       # empty, and n < m
        for left in (0, 1):
            t = rnd(m)
            s = np.concatenate([t[:n], rnd(max(n - m, 0))])[:n]
            if n > 2:
                s[int(rng.integers(0, n))] = ord("N")
            for kind in (1, 2):
                out.append(LR(kind, s, t, 0, left, int(rng.integers(0, 4)), tag=f"e n {n} m {m}"))
    for w in range(band + 1):                              # kind 0: the tiny full DP (n <= w) and its neighbours
        for n in range(0, 2 * band + 3):
            for _ in range(2):
                s = rnd(n)
                t = np.concatenate([s, rnd(w)])
                if rng.random() < 0.7 and len(t):
                    t[int(rng.integers(0, len(t)))] = ACGT[rng.integers(0, 4)]
                out.append(LR(0, s, t, w, 0, int(rng.integers(0, 4)), tag=f"e one-sided n {n} w {w}"))
    for n in range(0, 2 * band + 4):                       # kind 1: n <= 2w or m <= w (full DP) and the first banded sizes
        for m in range(0, band + 3):
            for left in (0, 1):
                t = rnd(m, ACGT[:2])
                s = np.concatenate([t, rnd(n, ACGT[:2])])[:n]
                if n and rng.random() < 0.6:
                    s[int(rng.integers(0, n))] = ACGT[rng.integers(0, 4)]
                vc = int(rng.integers(0, 4))
                out.append(LR(1, s, t, 0, left, vc, tag=f"e edit n {n} m {m}"))
                out.append(LR(2, s, t, 0, left, vc, tag=f"e x-drop n {n} m {m}"))
    for m in (1, 5, 40, 100):                              # mode 2: the all-NUL window of pac2char(start == 0)
        for left in (0, 1):
            t = rnd(m)
            s = rnd(m + band)
            out.append(LR(2, s, t, 0, left, int(rng.integers(0, 4)), nul_s=True, tag=f"e all-NUL s m {m}"))
            out.append(LR(1, s, t, 0, left, int(rng.integers(0, 4)), nul_s=True, tag=f"e all-NUL s m {m}"))
            out.append(LR(0, s[:m], np.concatenate([t, rnd(band)]), band, 0, 0, nul_s=True, tag=f"e all-NUL s m {m} one-sided"))
            out.append(LR(0, s[:m], t, 0, 0, 0, nul_s=True, tag=f"e all-NUL s m {m} hamming"))
    for it in range(600):                                  # one repeated base, period 2, ...: which of several equal alignments wins
        alpha = np.frombuffer(ALPHABETS[it % 5], np.uint8)
        m = int(rng.integers(4, 120))
        t = rnd(m, alpha)
        s = mutate(rng, t, (it // 5) % 8, band, alpha)
        left = it & 1
        vc = int(rng.integers(0, 4))
        sv, tv = s, t
        out.append(LR(2, sv, tv, 0, left, vc, tag=f"e alphabet {ALPHABETS[it % 5]!r}"))
        if len(s) > m:
            out.append(LR(1, sv, tv, 0, left, vc, tag=f"e alphabet {ALPHABETS[it % 5]!r}"))
    return out


def family_f(band=3, seed=61, n_waves=16):
    """waves of 64 consecutive kind-2 requests that diverge: (1) m from 1 to 140 side by side; (2) 63 lanes that take the closed
    form next to one 140-base DP (the CM_ANY_LANE loop with one live lane); (3) lanes whose X-drop ends early -- an unrelated s
    after a 10-base common prefix -- next to lanes that run the whole length"""
    rng = np.random.default_rng(seed)
    out = []

    def pair(m, case, left, early=False):
        t = ACGT[rng.integers(0, 4, m)].copy()
        if early:
            s = np.concatenate([t[:10], ACGT[rng.integers(0, 4, m + band)]])[:m + band]
        else:
            s = mutate(rng, t, case, band)
        return s, t

    for v in range(n_waves):                               # (1)
        ms = rng.permutation(np.linspace(1, 140, 64).astype(int))
        for lane in range(64):
            left = int(rng.integers(0, 2))
            sv, tv = pair(int(ms[lane]), 2 + (lane + v) % 6, left)
            out.append(LR(2, sv, tv, 0, left, int(rng.integers(0, 3)), tag=f"f1 wave {v} lane {lane}"))
    for v in range(n_waves):                               # (2)
        live = int(rng.integers(0, 64)) if v else 63
        for lane in range(64):
            left = int(rng.integers(0, 2))
            sv, tv = pair(140, 2 + v % 6, left) if lane == live else pair(int(rng.integers(1, 141)), 0, left)
            out.append(LR(2, sv, tv, 0, left, int(rng.integers(0, 3)), tag=f"f2 wave {v} lane {lane}{' (the DP)' if lane == live else ''}"))
    for v in range(n_waves):                               # (3)
        for lane in range(64):
            early = ((lane >> (v % 6)) & 1) == 0
            left = int(rng.integers(0, 2))
            sv, tv = pair(int(rng.integers(30, 141)), 2 + lane % 6, left, early)
            out.append(LR(2, sv, tv, 0, left, int(rng.integers(0, 3)), tag=f"f3 wave {v} lane {lane}{' early' if early else ''}"))
    return out


# ------------------------------------------------------------------------------------------------------------ the batches by name
def params(band, max_ed):
    return cl.default_params(band=band, max_ed=max_ed)


_cache = {}


def batch(name):
    """the batch `name` (built once per process and shared; nothing modifies it)"""
    if name in _cache:
        return _cache[name]
    fam, *rest = name.split("-")
    band = int(rest[0]) if rest else 3
    P = params(band, dict(PARAM_SETS)[band])
    cap = int(rest[1]) if len(rest) > 1 else 144
    if fam == "a":
        b = build(P, cap, family_a(band), 1)
    elif fam == "b":
        b = build(P, cap, family_b(band), 2)
    elif fam == "c":
        b = build(P, cap, family_c(band, cap, reps=1 if cap > 200 else 2), 3)
    elif fam == "d":
        b = build(P, cap, family_d(band, cap), 4)
    elif fam == "e":
        b = build(P, cap, family_e(band), 5)
    elif fam == "f":
        b = build(P, cap, family_f(band), 6)
    else:
        raise KeyError(name)
    _cache[name] = b
    return b


def dump(name, path):
    """the batch as one file for tests/diag/dp_san_main.cpp (emu_dp_batch under the host sanitizers, stand-alone): cm_params, str_cap
    (i4), n_req (u4), arena_len (u8), the arena, the requests, the expected results"""
    b = batch(name)
    with open(path, "wb") as f:
        f.write(bytes(b.P))
        f.write(np.array([b.str_cap], "<i4").tobytes() + np.array([len(b)], "<u4").tobytes() + np.array([b.arena.size], "<u8").tobytes())
        f.write(b.arena.tobytes() + b.req.tobytes() + b.exp.tobytes())


# every family x parameter set the tests run: name -> "family-band-str_cap"
A_BATCH = {3: "a-3-144", 2: "a-2-144", 5: "a-5-152"}       # family (a) by band (n reaches 140 + band: every request fits its buffers)
ALL_BATCHES = [*A_BATCH.values(), "b-3-144", "b-5-144", "c-3-144", "c-3-8", "c-3-1016", "c-5-144", "d-3-144", "d-3-8", "d-5-144", "e-3-144",
               "e-2-144", "e-5-144", "f-3-144"]
ARR1_BATCHES = ["a-3-144", "b-3-144", "c-3-144", "c-3-8", "c-3-1016", "e-3-144", "f-3-144"]      # kind 2 of these also through arrangement 1 (band 3 only)
