"""The device-side index builder without a device: the bodies of circminer_amd/csrc/cm_index_build.h run by a host emulation
(tests/hostemu_index.cpp) against cm_host_build_index, the packed FASTA as a table-less source of the index reader, and the
new names of the C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from circminer_amd import lib as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 1 << 28


@pytest.fixture(scope="module")
def emu_ib(built):
    out_dir = os.path.join(ROOT, "tests", "_hostemu")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libcmemu_index.so")
    srcs = [os.path.join(ROOT, "tests", "hostemu_index.cpp"), os.path.join(ROOT, "circminer_amd", "csrc", "cm_index_build.h"),
            os.path.join(ROOT, "include", "circminer_hot.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "circminer_amd", "csrc"), srcs[0], "-o", so])
    E = C.CDLL(so)
    vp = C.c_void_p
    E.emu_index_build.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    E.emu_index_build.restype = C.c_int
    return E


def _contig(rng, n):
    """random sequence with N runs, lower-case stretches, a homopolymer and two tandem repeats"""
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    for _ in range(6):
        a = int(rng.integers(0, n - 400))
        g[a:a + int(rng.integers(1, 300))] = ord("N")
    for _ in range(6):
        a = int(rng.integers(0, n - 400))
        g[a:a + int(rng.integers(1, 300))] |= 0x20                      # lower case: not indexed
    g[n // 5] = ord("R")                                                # an IUPAC letter
    a = n // 3
    g[a:a + 3000] = ord("A")                                            # one bucket, one checksum, 3000 - k + 1 entries
    a = n // 2
    g[a:a + 1500] = np.resize(np.frombuffer(b"ACG", np.uint8), 1500)    # period 3: three buckets of ~500 entries
    a = 2 * n // 3
    unit = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 37)]
    g[a:a + 37 * 12] = np.resize(unit, 37 * 12)                         # period 37: buckets of ~11 entries, several checksums each
    return g


def _host_arrays(L, g, k):
    iv = cl.IndexView()
    assert L.cm_host_build_index(cl.ptr(g, cl.u8p), len(g), k, 0, 4, C.byref(iv)) == 0
    n = int(iv.n_entries)
    off = np.ctypeslib.as_array(iv.bucket_off, (NB + 1,)).copy()
    cks = np.ctypeslib.as_array(iv.checksum, (max(n, 1),))[:n].copy()
    pos = np.ctypeslib.as_array(iv.pos, (max(n, 1),))[:n].copy()
    L.cm_host_free_index(C.byref(iv))
    return off, cks, pos


def _emu_arrays(E, g, k, lane_max, wg_max, seed):
    off = np.empty(NB + 1, np.uint32)
    cap = max(len(g), 1)
    cks, pos = np.zeros(cap, np.uint16), np.zeros(cap, np.uint32)
    n, paths, mx = C.c_uint64(0), (C.c_uint64 * 3)(), C.c_uint32(0)
    gg = np.ascontiguousarray(g)
    rc = E.emu_index_build(gg.ctypes.data if len(gg) else None, len(gg), k, lane_max, wg_max, seed, off.ctypes.data, cks.ctypes.data, pos.ctypes.data, cap,
                           C.byref(n), paths, C.byref(mx))
    assert rc == 0
    return off, cks[:n.value], pos[:n.value], list(paths), mx.value


@pytest.mark.parametrize("k", [14, 17, 20, 22])
def test_emulated_builder_equals_host_builder(emu_ib, k):
    """shuffled scatter order, thresholds small enough that all three ordering paths run: same arrays as cm_host_build_index"""
    L = cl.load()
    rng = np.random.default_rng(100 + k)
    for n, lane_max, wg_max in ((60_000, 4, 64), (25_000, 2, 16)):
        g = _contig(rng, n)
        want = _host_arrays(L, g, k)
        off, cks, pos, paths, mx = _emu_arrays(emu_ib, g, k, lane_max, wg_max, seed=k * 7 + n)
        assert len(cks) == len(want[1]) and off[NB] == len(cks)
        assert np.array_equal(off, want[0])
        assert np.array_equal(cks, want[1])
        assert np.array_equal(pos, want[2])
        assert paths[0] > 0 and paths[1] > 0 and paths[2] > 0, paths          # lane / workgroup / oversize all ran
        assert mx >= 3000 - k + 1 and sum(paths) == int((np.diff(want[0].astype(np.int64)) > 0).sum())


def test_emulated_builder_edges(emu_ib):
    L = cl.load()
    k = 20
    rng = np.random.default_rng(5)
    rnd = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    spiked = rnd(5000)
    spiked[k - 1::k] = ord("N")                                # an N every k - 1 bases: no k-mer survives
    cases = {"all_n": np.full(3000, ord("N"), np.uint8), "short": rnd(k - 1), "exact": rnd(k), "spiked": spiked,
             "tile_edge": rnd(2048 + k - 1), "tile_edge_plus": rnd(2048 + k), "lower": np.concatenate([rnd(500), rnd(500) | 0x20, rnd(500)])}
    for name, g in cases.items():
        want = _host_arrays(L, g, k)
        off, cks, pos, paths, mx = _emu_arrays(emu_ib, g, k, 16, 4096, seed=1)
        assert np.array_equal(off, want[0]) and np.array_equal(cks, want[1]) and np.array_equal(pos, want[2]), name
        if name in ("all_n", "short", "spiked"):
            assert len(cks) == 0 and paths == [0, 0, 0], name
        if name == "exact":
            assert len(cks) == 1 and pos[0] == 1 and paths == [1, 0, 0]


def test_device_allocation_list_over_malloc(tmp_path):
    """DevList (cm_index_dev.h), the owner of a slot's device arrays, with malloc / free in place of the device allocator: hand-over,
    scope exit on a failure at every allocation, double release, empty lists -- the program counts its live blocks itself"""
    exe = str(tmp_path / "devlist")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "circminer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "diag", "devlist_san_main.cpp"), "-o", exe])
    assert subprocess.check_output([exe], text=True).strip() == "devlist: 0 mismatches, 0 blocks live"


def test_pinned_ranges_over_a_fake_runtime(tmp_path):
    """PinnedRanges (cm_pinned_ranges.h), the owner of cm_mapping_run's page-locked ranges, over a fake register / unregister that
    keeps its own set of live ranges: growing batch arrays, widened text blocks, a block with two registrations, the cap of 64, a
    refused registration, a failed unregistration, release from a second thread -- the program checks the invariants after every call"""
    exe = str(tmp_path / "pinned")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "circminer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "diag", "pinned_san_main.cpp"), "-o", exe])
    assert subprocess.check_output([exe], text=True).strip() == "0 mismatches"


def _write_packed(tmp_path):
    """a FASTA of two chromosomes with lower-case and IUPAC letters, packed into two contigs"""
    rng = np.random.default_rng(3)
    recs = []
    for name, n in (("chrA", 5000), ("chrB", 3100)):
        s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes())
        s[100:180] = bytes(s[100:180]).lower()
        for i, ch in zip(range(300, 312), b"RYKMSWBDHVNn"):
            s[i] = ch
        recs.append((name, bytes(s)))
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, s in recs:
            f.write(f">{name} descr\n")
            f.writelines(s[i:i + 60].decode() + "\n" for i in range(0, len(s), 60))
    packed, info = cl.pack_genome(fa, 6000)                    # chrB does not fit behind chrA: two packed contigs
    return packed, info


def _genomes(path):
    f = cl.IndexFile(path, genome_only=True)
    out = [(iv.contig_num, iv.ref_len, bytes(np.ctypeslib.as_array(iv.genome, (iv.ref_len,)))) for iv in f]
    f.close()
    return f, out


def test_packed_fasta_is_a_table_less_source(built, tmp_path):
    L = cl.load()
    packed, info = _write_packed(tmp_path)
    idx = cl.write_index(packed, kmer=17, n_threads=2)
    fi, from_index = _genomes(idx)
    ff, from_fasta = _genomes(packed)
    assert len(from_index) == 2 and from_fasta == from_index
    assert ff.table_less and ff.kmer == 0 and ff.n_records == 2 and not fi.table_less and fi.kmer == 17
    assert all(set(g) <= set(b"ACGTN") for _, _, g in from_fasta) and any(b"N" in g for _, _, g in from_fasta)
    # no table to serve
    h, kmer, full, nrec = C.c_void_p(), C.c_int32(7), C.c_int32(7), C.c_uint32(0)
    assert L.cm_host_open_index(packed.encode(), C.byref(h), C.byref(kmer), C.byref(full), C.byref(nrec)) == 0
    assert (kmer.value, full.value, nrec.value) == (0, -1, 2)
    iv, raw, loaded = cl.IndexView(), cl.IndexRaw(), C.c_int(1)
    assert L.cm_host_next_contig(h, 2, C.byref(iv), C.byref(loaded)) == -1           # CM_EINVAL
    assert L.cm_host_next_contig_raw(h, 2, C.byref(raw), C.byref(loaded)) == -1
    assert L.cm_host_next_contig_genome(h, C.byref(iv), C.byref(loaded)) == 0 and loaded.value == 1 and iv.contig_num == 0     # ... and the handle still works
    L.cm_host_free_loaded_contig(C.byref(iv))
    L.cm_host_close_index(h)
    with pytest.raises(RuntimeError, match="packed FASTA"):
        cl.IndexFile(packed)


def test_mapping_run_on_a_packed_fasta_needs_k(built, tmp_path):
    """no index file, no k to read: CM_EINVAL with a message, before any device is touched (this suite runs without one)"""
    L = cl.load()
    packed, info = _write_packed(tmp_path)
    gtf = str(tmp_path / "a.gtf")
    open(gtf, "w").write("")
    a = cl.MappingArgs(packed.encode(), info.encode(), gtf.encode(), b"/nonexistent_1.fq", b"/nonexistent_2.fq", str(tmp_path / "out").encode(),
                       cl.default_params(kmer=0), 1, 2, 0, 0, 1)
    st, err = cl.MappingStats(), C.create_string_buffer(512)
    assert L.cm_mapping_run(C.byref(a), C.byref(st), err, len(err)) == -1
    assert b"packed FASTA" in err.value and b"kmer" in err.value


def test_mapping_run_refusals_before_any_device(built, tmp_path):
    """what cm_mapping_run refuses before it creates a context, each with its code and message, each followed by another refusal
    in the same process (a clean-up that frees twice would show): null path, report 3, rank 2 of 2, k of the index file against
    params.kmer, a missing index file, a missing .index.info"""
    L = cl.load()
    packed, info = _write_packed(tmp_path)
    idx = cl.write_index(packed, kmer=20, n_threads=2)
    gtf = str(tmp_path / "a.gtf")
    open(gtf, "w").write("")
    out = str(tmp_path / "out").encode()

    def run(index=idx.encode(), index_info=None, gtf_path=gtf.encode(), kmer=0, report=1, rank=0, world=1):
        a = cl.MappingArgs(index, index_info or (index or b"") + b".info", gtf_path, b"/nonexistent_1.fq", b"/nonexistent_2.fq", out,
                           cl.default_params(kmer=kmer), report, 2, 0, rank, world)
        st, err = cl.MappingStats(), C.create_string_buffer(512)
        rc = L.cm_mapping_run(C.byref(a), C.byref(st), err, len(err))
        return rc, err.value

    k_mismatch = (-1, b"index was built for k = 20, params ask for k = 18")
    cases = [
        (dict(gtf_path=None), (-1, b"cm_mapping_run: null argument")),
        (dict(kmer=18), k_mismatch),
        (dict(report=3), (-1, b"report must be 0 (none), 1 (PAM) or 2 (SAM)")),
        (dict(index=(idx + ".nope").encode(), index_info=(idx + ".info").encode()), (-1, b"cm_host_open_index failed (-1)")),
        (dict(rank=2, world=2), (-1, b"rank 2 of 2")),
        (dict(index_info=(idx + ".nope.info").encode()), (-1, b"cm_host_read_index_info failed (-1)")),
        (dict(kmer=18), k_mismatch),
        (dict(index=packed.encode(), index_info=info.encode()), (-1, b"is a packed FASTA, not an index file")),
    ]
    for kw, (rc, msg) in cases:
        got = run(**kw)
        assert got[0] == rc and msg in got[1], (kw, got)
    assert L.cm_mapping_run(None, None, None, 0) == -1                  # no arguments, no room for a message
    assert run(kmer=18) == k_mismatch


def test_new_names_agree_between_header_library_and_binding(built):
    L = cl.load()
    hdr = open(os.path.join(ROOT, "include", "circminer_hot.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("cm_build_contig", "cm_index_download", "cm_dp_batch", "cm_annot_batch"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in cl.EXPORTED_SYMBOLS
    assert "typedef struct cm_build_stats" in hdr and "typedef struct cm_dp_req" in hdr and "typedef struct cm_dp_res" in hdr
    assert "typedef struct cm_annot_req" in hdr and "typedef struct cm_annot_res" in hdr
    got = (C.c_uint32 * 32)()
    n = L.cm_abi_sizes(got, 32)
    assert n == 19 and got[14] == C.sizeof(cl.BuildStats) == 48
    assert got[15] == C.sizeof(cl.DpReq) == 40 and got[16] == C.sizeof(cl.DpRes) == 20
    assert got[17] == C.sizeof(cl.AnnotReq) == 32 and got[18] == C.sizeof(cl.AnnotRes) == 16
    assert L.cm_abi_sizes(got, 16) == -1 and L.cm_abi_sizes(got, 18) == -1                # (a caller with room for fewer entries is told so)
    # without a context both refuse, they do not crash
    assert L.cm_build_contig(None, 0, 0, None, 0, None) == -1
    assert L.cm_index_download(None, 0, None, None, None, 0, None) == -1
    assert L.cm_dp_batch(None, None, None, 0, None, 0, 144, 0, 0, 0, None) == -1
    assert L.cm_annot_batch(None, 0, None, None, 0, None, None) == -1
