"""cm_build_contig on the device: the k-mer table built from the sequence alone must be the arrays the host builder makes,
byte for byte, on every ordering path; mapping on such contigs must give what mapping on uploaded ones gives; and the file
entry points must run from the packed FASTA with no index file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from circminer_amd import lib as cl, synth
from oracle import oracle_py as op
from conftest import first_diff
from test_index_build_cpu import NB, _host_arrays

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    torch.cuda.init()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _view_arrays(iv):
    n = int(iv.n_entries)
    return (np.ctypeslib.as_array(iv.bucket_off, (NB + 1,)), np.ctypeslib.as_array(iv.checksum, (max(n, 1),))[:n],
            np.ctypeslib.as_array(iv.pos, (max(n, 1),))[:n])


def _assert_slot_is(hp, slot, want, what=""):
    off, cks, pos = hp.index_arrays(slot)
    assert len(cks) == len(want[1]) == int(off[NB]), (what, len(cks), len(want[1]))
    assert np.array_equal(off, want[0]), what
    assert np.array_equal(cks, want[1]), (what, np.nonzero(cks != want[1])[0][:5])
    assert np.array_equal(pos, want[2]), (what, np.nonzero(pos != want[2])[0][:5])


def _print_stats(what, g, st):
    print(f"[index build] {what}: {len(g)} bp, {st.n_entries} entries, fullest bucket {st.max_bucket}, buckets by path "
          f"{list(st.buckets_by_path)}, {st.ms_device:.2f} ms on the device, {st.reserved} MiB of temporaries", flush=True)


@pytest.mark.parametrize("name,kmer", [("ds_tiny", None), ("ds_tiny2r", None), ("ds_long", None), ("ds_small", None), ("ds_tiny", 22)])
def test_built_arrays_equal_the_host_builders(name, kmer, request):
    ds = request.getfixturevalue(name)
    L = cl.load()
    k = kmer or ds.kmer
    hp = cl.HotPath(cl.default_params(kmer=k))
    for ci, g in enumerate(ds.hi.contigs):
        want = _view_arrays(ds.hi.views[ci]) if kmer is None else _host_arrays(L, g, k)
        st = hp.build_contig(0, ci, g)
        _print_stats(f"{name} contig {ci} k {k}", g, st)
        assert st.n_entries == len(want[1]) and sum(st.buckets_by_path) == int((np.diff(want[0].astype(np.int64)) > 0).sum())
        assert st.max_bucket == int(np.diff(want[0].astype(np.int64)).max())
        _assert_slot_is(hp, 0, want, f"{name}[{ci}]")
    hp.close()


def test_built_arrays_of_a_chr21_size_contig():
    """46.7 Mbp: the count / scatter grids, the scans and the per-bucket pass span many workgroups"""
    L = cl.load()
    d = synth.generate("chr21", n_pairs=64, seed=21)
    g = d.contigs[0]
    assert len(g) >= 40_000_000
    want = _host_arrays(L, g, 20)
    hp = cl.HotPath(cl.default_params())
    st = hp.build_contig(3, 0, g)
    _print_stats("chr21 preset", g, st)
    assert st.n_entries == len(want[1])
    _assert_slot_is(hp, 3, want, "chr21")
    hp.close()


def _rnd(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()


def _tandem(rng, unit, total, sub_every):
    """`total` bases of a tandem repeat of `unit` with one substitution about every `sub_every` bases: the same 14-mer is followed
    by different bases here and there, so its bucket holds several checksums, met in position order -- not in checksum order"""
    g = np.resize(unit, total).copy()
    at = rng.choice(total, total // sub_every, replace=False)
    g[at] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), g[at]) + rng.integers(1, 4, len(at))) % 4]
    return g


def _edge_cases(k):
    rng = np.random.default_rng(11)
    spiked = _rnd(rng, 50_000)
    spiked[k - 1::k] = ord("N")
    lower = np.concatenate([_rnd(rng, 3000), _rnd(rng, 3000) | 0x20, _rnd(rng, 3000)])
    homo = np.concatenate([np.full(1 << 20, ord("A"), np.uint8), _rnd(rng, 300_000)])
    tandem = np.concatenate([_rnd(rng, 1000), _tandem(rng, np.frombuffer(b"ACG", np.uint8), 200_000, 997), np.full(30, ord("N"), np.uint8),
                             _tandem(rng, _rnd(rng, 50), 200_000, 211), _rnd(rng, 1000)])
    return [("all_n", np.full(5000, ord("N"), np.uint8)), ("shorter_than_k", _rnd(rng, k - 1)), ("exactly_k", _rnd(rng, k)), ("n_every_k_minus_1", spiked),
             ("lower_case", lower), ("homopolymer", homo), ("tandem", tandem), ("empty", np.zeros(0, np.uint8))]


def test_edges_and_every_ordering_path():
    L = cl.load()
    k = 20
    hp = cl.HotPath(cl.default_params(kmer=k))
    for name, g in _edge_cases(k):
        want = _host_arrays(L, g, k) if len(g) else (np.zeros(NB + 1, np.uint32), np.zeros(0, np.uint16), np.zeros(0, np.uint32))
        st = hp.build_contig(1, 0, g)
        _print_stats(name, g, st)
        paths = list(st.buckets_by_path)
        sizes = np.diff(want[0].astype(np.int64))
        _assert_slot_is(hp, 1, want, name)
        assert st.n_entries == len(want[1]) and st.max_bucket == int(sizes.max()), name
        # the thresholds of cm_index_build.h decide the path of a bucket
        assert paths == [int(((sizes > 0) & (sizes <= 16)).sum()), int(((sizes > 16) & (sizes <= 4096)).sum()), int((sizes > 4096).sum())], name
        if name in ("all_n", "shorter_than_k", "n_every_k_minus_1", "empty"):
            assert st.n_entries == 0 and paths == [0, 0, 0], name
        elif name == "exactly_k":
            assert st.n_entries == 1 and paths == [1, 0, 0]
        elif name == "lower_case":
            assert st.n_entries == 2 * (3000 - k + 1) and paths[0] > 0 and paths[1] == paths[2] == 0
        elif name == "homopolymer":
            assert st.max_bucket >= (1 << 20) - k and paths[2] >= 1
        elif name == "tandem":
            assert paths[1] >= 40 and paths[2] >= 3, paths
            # ... and both kinds of bucket held several checksums that did not arrive in order
            for lo, hi in ((17, 4096), (4097, 1 << 30)):
                mixed = 0
                for h in np.nonzero((sizes >= lo) & (sizes <= hi))[0]:
                    a, b = int(want[0][h]), int(want[0][h + 1])
                    by_pos = want[1][a:b][np.argsort(want[2][a:b], kind="stable")]
                    mixed += int(len(np.unique(by_pos)) > 1 and (np.diff(by_pos.astype(np.int64)) < 0).any())
                assert mixed > 0, (lo, hi)
    hp.close()


def _map_all(ds, P, loader):
    """all rounds, contig ci made resident in slot ci by loader(hp, ci); seeds of every round, final (state, category, active)"""
    hp = cl.HotPath(P)
    hp.upload(ds.batch)
    seeds = []
    for ci in range(ds.hi.n_contigs):
        loader(hp, ci)
        seeds.append(tuple(x.copy() if isinstance(x, np.ndarray) else x for x in hp.seeds(ci)))
        hp.map_round(ci, ci == ds.hi.n_contigs - 1)
    res = hp.download()
    hp.close()
    return seeds, res


def test_mapping_on_device_built_contigs(ds_variety):
    ds, P = ds_variety, cl.default_params(kmer=ds_variety.kmer)
    s_up, r_up = _map_all(ds, P, lambda hp, ci: hp.load_contig(ci, ds.hi.views[ci], ds.hi.annots[ci]))
    s_bd, r_bd = _map_all(ds, P, lambda hp, ci: hp.build_contig(ci, ci, ds.hi.contigs[ci], ds.hi.annots[ci]))
    for ci, (a, b) in enumerate(zip(s_up, s_bd)):
        hit = a[2] > 0                                # (a probe's start index means something only when it has hits)
        assert a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[0][hit], b[0][hit]), ci
    # against the oracle, round by round on ITS index, as test_map_parity_all_rounds compares
    st0, act0 = op.default_state(P, ds.batch.n)
    for ci in range(ds.hi.n_contigs):
        cat0 = op.map_round(P, ds.ohi.views[ci], ds.ohi.annots[ci], ds.batch, ci == ds.hi.n_contigs - 1, st0, act0)
    st1, cat1, act1 = r_bd
    assert (cat0 == cat1).all(), np.nonzero(cat0 != cat1)[0][:10]
    assert (act0 == act1).all()
    assert st0.tobytes() == st1.tobytes(), first_diff(st0, st1)
    assert r_up[0].tobytes() == st1.tobytes() and (r_up[1] == cat1).all() and (r_up[2] == act1).all()


def test_a_slot_is_reused_across_loaders(ds_tiny2r):
    ds, P = ds_tiny2r, cl.default_params()
    want_st, _, _ = op.map_all_rounds(P, ds.ohi, ds.batch)
    hp = cl.HotPath(P)
    for order in (("load", "build"), ("build", "load")):        # contig 0 one way, contig 1 the other, all through slot 0
        hp.upload(ds.batch)
        for ci, how in enumerate(order):
            for first in (("build", "load") if how == "load" else ("load", "build")):     # fill the slot the OTHER way first, with the other contig
                cj = ci if first == how else 1 - ci
                if first == "load":
                    hp.load_contig(0, ds.hi.views[cj], ds.hi.annots[cj])
                else:
                    hp.build_contig(0, cj, ds.hi.contigs[cj], ds.hi.annots[cj])
                _assert_slot_is(hp, 0, _view_arrays(ds.hi.views[cj]), (order, ci, first))
            hp.map_round(0, ci == ds.hi.n_contigs - 1)
        st, _, _ = hp.download()
        assert st.tobytes() == want_st.tobytes(), (order, first_diff(want_st, st))
    # the capacity rule of the download
    n = C.c_uint64(0)
    cks = np.zeros(4, np.uint16)
    assert hp.L.cm_index_download(hp.h, 0, None, cks.ctypes.data, None, 4, C.byref(n)) == -6 and n.value == ds.hi.views[1].n_entries     # CM_ELIMIT
    assert hp.L.cm_index_download(hp.h, 5, None, None, None, 0, C.byref(n)) == -5                                                           # CM_ESTATE: nothing loaded there
    hp.close()


def _tiny2r_index_file(ds, tmp_path, kmer):
    packed = str(tmp_path / f"ref_k{kmer}.fa.packed.fa")
    with open(packed, "w") as f:
        for i, c in enumerate(ds.d.contigs):
            f.write(f">{i + 1}\n{c.tobytes().decode()}\n")
    return cl.write_index(packed, kmer=kmer, n_threads=4)


def _wide_params():
    """18 seeds per read: cm_create takes the build for reads of up to 24 seeds (cm_dispatch.cpp)"""
    return cl.default_params(max_read_len=300, kmer=16)


def _one_round_on_slot_0(hp, ds, rec):
    hp.upload(ds.batch)
    hp.load_contig_raw(0, rec, ds.hi.annots[0])
    seeds = [x.copy() if isinstance(x, np.ndarray) else x for x in hp.seeds(0)]
    hp.map_round(0, False)
    return seeds, hp.download()


@pytest.mark.parametrize("wide", [False, True], ids=["k16", "k24"])
def test_a_failed_raw_load_leaves_a_clean_slot(wide, ds_tiny2r, tmp_path):
    """A record whose first bucket header claims 2^20 entries is refused after the slot gave up its contig: the slot is then
    unloaded (the old contig does not come back), and loading the good record again maps as in a context that never failed."""
    ds, P = ds_tiny2r, _wide_params() if wide else cl.default_params()
    f = cl.IndexFile(_tiny2r_index_file(ds, tmp_path, P.kmer), n_threads=2, raw=True)
    good = next(f)
    tab = np.ctypeslib.as_array(C.cast(good.table, C.POINTER(C.c_int32)), (int(good.table_slots) * 2,)).copy()
    tab[1] = 1 << 20                                   # info of the first bucket's header (only in-range reads follow from it)
    bad = cl.IndexRaw(good.contig_num, good.ref_len, good.genome, good.n_buckets, good.hv, good.count14, tab.ctypes.data, good.table_slots)
    fresh = cl.HotPath(P)
    want_seeds, want_res = _one_round_on_slot_0(fresh, ds, good)
    fresh.close()
    hp = cl.HotPath(P)
    hp.upload(ds.batch)
    hp.load_contig_raw(0, good, ds.hi.annots[0])
    with pytest.raises(RuntimeError, match="malformed"):
        hp.load_contig_raw(0, bad)
    n = C.c_uint64(0)
    assert hp.L.cm_index_download(hp.h, 0, None, None, None, 0, C.byref(n)) == -5          # CM_ESTATE
    assert hp.L.cm_map_round(hp.h, 0, 0) == -5
    seeds, res = _one_round_on_slot_0(hp, ds, good)
    hp.close()
    f.close()
    assert seeds[3] == want_seeds[3] and all(a.tobytes() == b.tobytes() for a, b in zip(seeds[:3], want_seeds[:3]))
    assert res[0].tobytes() == want_res[0].tobytes() and (res[1] == want_res[1]).all() and (res[2] == want_res[2]).all()
    assert (want_seeds[2] > 0).any()                   # (probes with hits: the comparison is not one of empty rounds)


def test_build_contig_from_the_build_for_long_reads(ds_tiny2r):
    """cm_build_contig from the build for long reads: the host builder's arrays, and the statistics the other build reports"""
    g = ds_tiny2r.hi.contigs[0]
    want = _host_arrays(cl.load(), g, 16)
    seen = []
    for what, P in (("k16", cl.default_params(max_read_len=150, kmer=16)), ("k24", _wide_params())):
        hp = cl.HotPath(P)
        st = hp.build_contig(0, 0, g)
        _print_stats(f"tiny2r contig 0 k 16, {what} build", g, st)
        if what == "k24":
            _assert_slot_is(hp, 0, want, what)
        seen.append((st.n_entries, st.max_bucket, st.reserved, list(st.buckets_by_path)))
        hp.close()
    assert seen[0] == seen[1] and seen[0][0] == len(want[1])


def test_files_to_files_without_an_index_file(tmp_path):
    """FASTA + GTF + FASTQ -> circ_report with index_path = the packed FASTA: every output byte-equal to the run through the index file;
    then the same from plain C++ (examples/cm_map.cpp) in a directory that never held an index file."""
    n = 3000
    d = synth.generate("tiny2r", n_pairs=n, seed=33)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            seq = d.contigs[con - 1][start:start + ln].tobytes().decode()
            f.write(f">{name} some description\n")
            f.writelines(seq[i:i + 70] + "\n" for i in range(0, ln, 70))
    packed, info = cl.pack_genome(fa, 150_000)
    gtf = str(tmp_path / "ref.gtf")
    open(gtf, "w").write(d.gtf_text)
    fq = []
    for mate, arr in ((1, d.seq1), (2, d.seq2)):
        p = str(tmp_path / f"reads_{mate}.fq")
        with open(p, "w") as f:
            for i in range(n):
                f.write(f"@frag.{i}/{mate}\n{arr[i].tobytes().decode()}\n+\n{'I' * arr.shape[1]}\n")
        fq.append(p)
    # the run without an index file goes first: nothing but the packed FASTA and its .index.info exists yet
    out_b = str(tmp_path / "built")
    assert not os.path.exists(packed + ".index")
    st_b = cl.run_mapping(packed, gtf, fq[0], fq[1], out_b, cl.default_params(kmer=20), n_threads=4, batch_pairs=1024, index_info=info)
    cs_b = cl.run_circ(packed, gtf, out_b, st_b.rounds, cl.default_params(kmer=20), index_info=info)
    with pytest.raises(RuntimeError, match="packed FASTA"):
        cl.run_mapping(packed, gtf, fq[0], fq[1], out_b + "_k0", cl.default_params(kmer=0), index_info=info)
    # plain C++, still no index file
    exe = str(tmp_path / "cm_map")
    libdir = os.path.join(ROOT, "circminer_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cm_map.cpp"), "-L", libdir,
                           "-lcmhot", f"-Wl,-rpath,{libdir}", "-o", exe])
    out_c = str(tmp_path / "cpp")
    msg = subprocess.check_output([exe, packed, gtf, fq[0], fq[1], out_c, "pam", "20"], text=True)
    assert msg.startswith(f"{n} pairs, {st_b.rounds} round(s), {st_b.bsj_pairs} BSJ") and "stage 2:" in msg
    assert not os.path.exists(packed + ".index")
    # the same through the index file
    idx = cl.write_index(packed, kmer=20, n_threads=4)
    out_i = str(tmp_path / "indexed")
    st_i = cl.run_mapping(idx, gtf, fq[0], fq[1], out_i, cl.default_params(kmer=0), n_threads=4, batch_pairs=1024)
    cs_i = cl.run_circ(idx, gtf, out_i, st_i.rounds, cl.default_params(kmer=0))
    assert st_i.rounds == st_b.rounds == 2 and st_i.pairs == st_b.pairs == n and st_i.bsj_pairs == st_b.bsj_pairs > 0
    assert list(st_i.by_type) == list(st_b.by_type)
    assert (cs_i.pairs, cs_i.candidate_rows, cs_i.calls) == (cs_b.pairs, cs_b.candidate_rows, cs_b.calls) and cs_b.calls > 0
    for suffix in [".mapping.pam", "_2_remain_R1.fastq", "_2_remain_R2.fastq", ".candidates.pam", ".circ_report"]:
        want = open(out_i + suffix, "rb").read()
        assert len(want) > 0, suffix
        assert open(out_b + suffix, "rb").read() == want, suffix
        assert open(out_c + suffix, "rb").read() == want, suffix
