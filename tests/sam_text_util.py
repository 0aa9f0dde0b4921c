"""Helpers of the device-side SAM formatter's tests (test_sam_text_cpu.py, test_gpu_sam_text.py): the directed states of
pam_text_util with every combination the SAM rules branch on among the first 64, FASTQ records whose reads decide those rules
(every word edge of the cooperative copy, one byte outside ACGTNacgtn on reversed and on unreversed records, lower case), and the
project's own host writer as the checker -- cm_fastq_next on files holding the same bytes, then cm_write_sam with the same states.
Without a header it gives the rows alone."""
import numpy as np

from fastq_text_util import records, text_of
from pam_text_util import CHRS, INT_MAX, INT_MIN, HostRows, directed_states, name_records

SPAN_RECS, WINDOW = 16, 8192                                            # cmst::SPAN_RECS, cmrt::WINDOW
SPAN_PAIRS = SPAN_RECS // 2
SAM_MAPPED = (0, 1, 2, 5, 7, -1, INT_MIN, -9)                           # type <= CHIORF || CONGEN || CONGNM, as a signed compare
SAM_UNMAPPED = (3, 4, 6, 8, 13, 14, INT_MAX, 100)
SHORT_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9)
ODD_BYTES = (b".", b"R", b"U", b"\r", b"\x00")                         # outside ACGTNacgtn: no complement


def sam_mapped(types):
    t = np.asarray(types, np.int64)
    return (t <= 2) | (t == 5) | (t == 7)


def sam_states(n, n_chr=len(CHRS)):
    """pam_text_util.directed_states with tlen == INT_MIN (signed overflow in the host's negation) replaced by INT_MIN + 1, and
    states 0 .. 23 set so that every combination of (mapped by the SAM rule, r1_forward, r2_forward, spos_r1 <, ==, > spos_r2)
    occurs; the fields those states print otherwise keep cycling"""
    st = directed_states(n, n_chr)
    st["tlen"][st["tlen"] == INT_MIN] = INT_MIN + 1
    for k in range(min(n, 24)):
        st["type"][k] = (SAM_MAPPED if k & 1 else SAM_UNMAPPED)[(k // 2) % 8]
        st["r1_forward"][k] = (k >> 1) & 1
        st["r2_forward"][k] = (k >> 2) & 1
        a = (5, 1_000_000_000, 4_294_967_295)[k // 8]                   # spos_r1, and spos_r2 larger, equal, smaller
        st["spos_r1"][k], st["spos_r2"][k] = a, (a + 94, a, a - 5)[k // 8]
    if n >= 64:
        seen = set(zip(sam_mapped(st["type"][:64]).tolist(), st["r1_forward"][:64].tolist(), st["r2_forward"][:64].tolist(),
                       np.sign(st["spos_r1"][:64].astype(np.int64) - st["spos_r2"][:64].astype(np.int64)).tolist()))
        assert len(seen) == 24, seen
    return st


def reversed_records(st):
    """(mate 1 reversed, mate 2 reversed) per pair, by the rule of sam_flag"""
    m = sam_mapped(st["type"])
    return m & (st["r1_forward"] == 0), m & (st["r2_forward"] == 0)


def _set_read(rec, seq: bytes, rng):
    rec[1] = seq
    rec[3] = bytes(rng.integers(33, 74, len(seq)).astype(np.uint8))


def sam_pair_records(rng, n, st, long_run=None, hi=150):
    """(records of R1, records of R2, what was placed): name_records / records with reads added that decide the rules -- every
    length of SHORT_LENGTHS in both files, all-lower-case reads, and per odd byte and per place (last base, first base, middle) a
    read on a record the states reverse and one on a record they do not, as far as n pairs have room for them"""
    recs = [name_records(rng, n, long_run, 1), records(rng, n, mate=2)]
    bases9 = np.frombuffer(b"ACGTNacgt", np.uint8)
    for mate in (0, 1):                                                  # hi > 150 (the 24-seed build): every other read is 151 .. hi bases
        for i in range(mate, n if hi > 150 else 0, 2):
            _set_read(recs[mate][i], bases9[rng.integers(0, 9, int(rng.integers(151, hi + 1)))].tobytes(), rng)
    rev = reversed_records(st)
    placed = {"short": 0, "odd_rev": 0, "odd_fwd": 0, "lower": 0}
    free = [list(range(n)), list(range(n))]

    def take(mate, want_rev=None):
        for i in free[mate]:
            if want_rev is None or bool(rev[mate][i]) == want_rev:
                free[mate].remove(i)
                return i
        return None
    bases = np.frombuffer(b"ACGTNacgtn", np.uint8)
    k = 0
    for b in ODD_BYTES:                                                  # (first: they need records of a kind)
        for place in ("last", "first", "middle"):
            for want_rev in (True, False):
                mate = k & 1
                k += 1
                i = take(mate, want_rev)
                if i is None and (i := take(1 - mate, want_rev)) is not None:
                    mate = 1 - mate
                if i is None:
                    continue
                ln = int(rng.integers(20, 151))
                s = bytearray(bases[rng.integers(0, 10, ln)].tobytes())
                s[{"last": ln - 1, "first": 0, "middle": ln // 2}[place]] = b[0]
                _set_read(recs[mate][i], bytes(s), rng)
                placed["odd_rev" if want_rev else "odd_fwd"] += 1
    for mate in (0, 1):
        for j, ln in enumerate(SHORT_LENGTHS):
            i = take(mate, want_rev=bool((j + mate) & 1)) if n >= 64 else take(mate)
            if i is None:
                continue
            _set_read(recs[mate][i], bases[rng.integers(0, 10, ln)].tobytes(), rng)
            placed["short"] += 1
        i = take(mate)
        if i is not None:
            _set_read(recs[mate][i], bytes(np.frombuffer(b"acgtn", np.uint8)[rng.integers(0, 5, 150)]), rng)
            placed["lower"] += 1
    return recs[0], recs[1], placed


def sam_pair_text(rng, n, st, long_run=None, hi=150):
    r1, r2, placed = sam_pair_records(rng, n, st, long_run, hi)
    return text_of(r1), text_of(r2), placed


def HostSam(tmpdir, t1: bytes, t2: bytes, n, tag="sam", chrs=CHRS):
    """the checker: pam_text_util.HostRows with cm_write_sam (without a header) as the writer"""
    return HostRows(tmpdir, t1, t2, n, tag=tag, chrs=chrs, write="write_sam")
