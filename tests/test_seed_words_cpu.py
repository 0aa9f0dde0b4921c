"""The k-mer word path of cmc::seed_probe without a device: cmc::kmer_from_span (circminer_amd/csrc/cm_core.h) against the per-byte
loop it replaced, kept in tests/hostemu_seed.cpp as the reference form, and emu-style seeding of a batch through cmc::seed_probe
against the oracle's seed batch."""
import ctypes as C

import numpy as np
import pytest

from circminer_amd import lib as cl
from oracle import oracle_py as op
from seed_words_util import load_emu_seed


@pytest.fixture(scope="module")
def emu_seed(built):
    return load_emu_seed()


def _report(out):
    return (f"checked {out[0]}, k-mers with a bad base {out[1]}, clean {out[2]}, mismatches {out[3]}; first: k {out[4]} mode {out[5]} qpos {out[6]} "
            f"form {out[7]} hv {out[8]} / {out[9]} cv {out[10]} / {out[11]}")


# 0 clean ACGT, 1 sprinkled with lower case / N / @ / B D U / bytes >= 0x80 / anything, 2 every byte value in turn, 3 all lower case
@pytest.mark.parametrize("flavour", [0, 1, 2, 3])
def test_words_equal_byte_loop_on_random_reads(emu_seed, flavour):
    """k = 14, 17, 20, 22; both strands; start alignments 0 - 7; every qpos of a read of 150: (hv, cv, bad) of the word path, from
    loaded words and from words filled byte by byte, equal the byte loop's -- also where a base is bad."""
    bad_total = clean_total = 0
    for seed in range(6):
        out = np.zeros(12, np.int64)
        assert emu_seed.seedw_sweep(seed, flavour, out.ctypes.data) == 0, _report(out)
        # 8 alignments x sum over k of (150 - k + 1) positions x 2 strands x 2 forms
        assert out[0] == 8 * sum(151 - k for k in (14, 17, 20, 22)) * 4
        bad_total += int(out[1]); clean_total += int(out[2])
    if flavour == 0:
        assert bad_total == 0
    elif flavour == 1:
        assert bad_total > 1000 and clean_total > 1000           # both outcomes are exercised
    elif flavour == 2:
        assert clean_total == 0
    else:
        assert bad_total == clean_total                          # lower case: bad on the forward strand, fine on the reverse


def test_every_byte_value_at_every_position(emu_seed):
    """a clean k-mer with each of the 256 byte values at each of its k positions in turn, in a read of exactly k bytes (both word
    loads reach into the slack on either side)"""
    out = np.zeros(12, np.int64)
    assert emu_seed.seedw_each_position(1, out.ctypes.data) == 0, _report(out)
    assert out[0] == 8 * sum(k * 256 for k in (14, 17, 20, 22)) * 4
    # per (position, value): 4 values leave the forward k-mer clean, 8 (either case) the reverse one
    assert out[2] == 8 * sum(k for k in (14, 17, 20, 22)) * (4 + 8)


def test_known_kmers(emu_seed):
    """spot values worked out by hand: ACGT = 0 1 2 3, the first 14 bases are the hash, the rest the checksum"""
    def run(span, k, rc):
        buf = np.zeros(24, np.uint8)
        buf[:len(span)] = np.frombuffer(span, np.uint8)
        if rc:
            buf = np.roll(buf, 24 - len(span))                   # the reverse span ends with the k-mer
        out = np.zeros(3, np.int32)
        emu_seed.seedw_kmer(buf.ctypes.data, k, rc, out.ctypes.data)
        return tuple(int(x) for x in out)
    assert run(b"A" * 20, 20, 0) == (0, 0, 0)
    assert run(b"T" * 20, 20, 0) == ((1 << 28) - 1, (1 << 12) - 1, 0)
    assert run(b"A" * 13 + b"C" + b"G" + b"A" * 5, 20, 0) == (1, 2 << 10, 0)
    assert run(b"A" * 20, 20, 1) == ((1 << 28) - 1, (1 << 12) - 1, 0)             # reverse complement of A^20 is T^20
    assert run(b"a" * 20, 20, 1) == ((1 << 28) - 1, (1 << 12) - 1, 0)             # upper-cased on the reverse strand only
    assert run(b"a" * 20, 20, 0)[2] == 1
    assert run(b"C" + b"A" * 19, 20, 1) == ((1 << 28) - 1, (1 << 12) - 2, 0)      # the lowest address is the last base: G = 2
    assert run(b"A" * 19 + b"N", 20, 0)[2] == 1
    assert run(b"ACGTACGTACGTAC", 14, 0) == (int("".join("0123"[i % 4] for i in range(14)), 4), 0, 0)


@pytest.mark.parametrize("with_desc", [0, 1])
def test_seed_batch_equals_oracle(emu_seed, ds_tiny2r, with_desc):
    """emu-style seeding of a small data set through cmc::seed_probe (index arrays / bucket descriptors) against oracle_seed_batch"""
    P = cl.default_params()
    iv, b = ds_tiny2r.hi.views[0], ds_tiny2r.batch
    S = b.max_len() // P.kmer
    a0, b0, c0 = op.seeds(P, ds_tiny2r.ohi.views[0], b, S)
    a1, b1, c1 = (np.zeros_like(a0) for _ in range(3))
    assert emu_seed.seedw_seed_batch(C.byref(P), C.byref(iv), C.byref(b.c), S, with_desc, None, a1.ctypes.data, b1.ctypes.data, c1.ctypes.data, None) == 0
    assert (c0 > 0).sum() > 1000
    assert (c0 == c1).all() and (b0 == b1).all() and (a0[c0 > 0] == a1[c0 > 0]).all()


def test_seed_batch_dirty_reads(emu_seed, ds_dirty):
    """ragged lengths, N runs, lower-case stretches (conftest.ds_dirty): reads shorter than k have no probe, a read that ends inside
    a seed has none for it"""
    P = cl.default_params()
    iv, b = ds_dirty.hi.views[0], ds_dirty.batch
    S = b.max_len() // P.kmer
    a0, b0, c0 = op.seeds(P, ds_dirty.ohi.views[0], b, S)
    a1, b1, c1 = (np.zeros_like(a0) for _ in range(3))
    assert emu_seed.seedw_seed_batch(C.byref(P), C.byref(iv), C.byref(b.c), S, 1, None, a1.ctypes.data, b1.ctypes.data, c1.ctypes.data, None) == 0
    assert (c0 == c1).all() and (b0 == b1).all() and (a0[c0 > 0] == a1[c0 > 0]).all()
