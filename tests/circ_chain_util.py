"""Shared by tests/test_circ_chain_cpu.py and tests/test_gpu_circ_chain.py: the host emulation of cm_circ_chain.hip
(tests/hostemu_circ_chain.cpp), the sets of sorted remain pairs with their problems (computed once per process), a request lister
written from the rule of include/circminer_hot.h alone, and the directed problems."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from circminer_amd import lib as cl, synth
from oracle import oracle_py as op
from stage2_util import remain_files_from_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CM_CHIBSJ, CM_CHI2BSJ = 3, 4

# (preset, pairs, seed, parameters, generator arguments): the sets the issue names
SETS = {
    "tiny": ("tiny", 3000, 5, {}, {}),
    "tiny2r": ("tiny2r", 3000, 13, dict(scan_level=2, max_ed=8, seed_lim=1000), {}),
    "variety": ("variety", 4000, 31, {}, {}),
    "long300": ("tiny2r", 1500, 41, {}, dict(read_len=300)),
}


@functools.lru_cache(maxsize=None)
def emu():
    """the emulation, built on first use into tests/_hostemu/ (not tracked)"""
    out_dir = os.path.join(ROOT, "tests", "_hostemu")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libccemu.so")
    csrc = os.path.join(ROOT, "circminer_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "hostemu_circ_chain.cpp"), os.path.join(ROOT, "include", "circminer_hot.h")] + \
           [os.path.join(csrc, h) for h in ("cm_core.h", "cm_aos.h", "cm_circ_chain.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                               srcs[0], "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    vp = C.c_void_p
    L.cm_cc_emu_table.restype = C.c_int
    L.cm_cc_emu_table.argtypes = [vp, C.c_uint32, C.c_int32, C.c_uint64, vp, vp]
    L.cm_cc_emu.restype = C.c_int
    L.cm_cc_emu.argtypes = [C.POINTER(cl.Params), C.POINTER(cl.AnnotView), C.c_int32, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint32, vp, vp, vp, vp,
                            C.c_uint64, vp, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32,
                            C.c_uint64, vp]
    return L


def emu_table(gene: bytes, ws: int, seed: int = 1):
    g = np.frombuffer(gene, np.uint8)
    off = np.zeros((1 << (2 * ws)) + 1, np.uint32)
    loc = np.zeros(max(len(g) - ws + 1, 1), np.uint32)
    assert emu().cm_cc_emu_table(g.ctypes.data if len(g) else None, len(g), ws, seed, off.ctypes.data, loc.ctypes.data) == 0
    return off, loc[:int(off[-1])]


def host_table(gene: bytes, ws: int):
    """cm_regional_table_build on the gene's bytes (start 0)"""
    L = cl.load()
    g = np.frombuffer(gene, np.uint8)
    off, loc = cl.u32p(), cl.u32p()
    assert L.cm_regional_table_build(g.ctypes.data if len(g) else None, 0, len(g), ws, C.byref(off), C.byref(loc)) == 0
    o = np.ctypeslib.as_array(off, ((1 << (2 * ws)) + 1,)).copy()
    l = np.ctypeslib.as_array(loc, (max(int(o[-1]), 1),)).copy()[:int(o[-1])]
    L.cm_regional_table_free(off, loc)
    return o, l


def emu_chains(P, av, genome, seqs, req, window=0, log_cap=0, cell_cap=0, seed=1):
    """the emulation's answers in cm_circ_chain_host's layout -> (CircChains, log length per problem)"""
    req = np.ascontiguousarray(req, dtype=cl.CIRC_CHAIN_REQ_DTYPE)
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    g = np.ascontiguousarray(genome, dtype=np.uint8)
    n = len(req)
    span = np.maximum(req["qe"].astype(np.int64) - req["qs"].astype(np.int64) + 1, 0)
    cap_c, cap_f = 10 * n, int((10 * (span // 3 + 1)).sum())
    res = np.zeros(n, cl.CIRC_CHAIN_RES_DTYPE)
    score, length, frag_off = np.zeros(max(cap_c, 1), np.float32), np.zeros(max(cap_c, 1), np.uint32), np.zeros(max(cap_c, 1), np.uint64)
    rpos, qpos = np.zeros(max(cap_f, 1), np.uint32), np.zeros(max(cap_f, 1), np.int32)
    log_len = np.zeros(max(n, 1), np.uint32)
    nc, nf = C.c_uint64(0), C.c_uint64(0)
    stats = (C.c_uint64 * 8)()
    rc = emu().cm_cc_emu(C.byref(P), C.byref(av), window, g.ctypes.data, len(g), seqs.ctypes.data if seqs.size else None, seqs.size,
                         req.ctypes.data if n else None, n, res.ctypes.data if n else None, score.ctypes.data, length.ctypes.data, frag_off.ctypes.data,
                         cap_c, rpos.ctypes.data, qpos.ctypes.data, cap_f, C.byref(nc), C.byref(nf), stats, log_cap, cell_cap, seed, log_len.ctypes.data)
    assert rc == 0, rc
    return cl.CircChains(res, score[:nc.value].copy(), length[:nc.value].copy(), frag_off[:nc.value].copy(), rpos[:nf.value].copy(),
                         qpos[:nf.value].copy(), [int(x) for x in stats]), log_len[:n]


class RemainSet:
    """The sorted remain pairs of one synthetic run (stage-1 states from the oracle), parsed back, and their problems per contig."""

    def __init__(self, preset, n, seed, kw, gen):
        self.tmp = tempfile.mkdtemp(prefix="cm_cc_")
        self.d = d = synth.generate(preset, n_pairs=n, seed=seed, mix=(0.3, 0.1, 0.6), **gen)
        self.gtf = os.path.join(self.tmp, "a.gtf")
        open(self.gtf, "w").write(d.gtf_text)
        self.hi = cl.HostIndex(d.contigs, d.chr_table, self.gtf, max_read_len=kw.get("max_read_len", 300))
        self.ohi = op.OracleIndex(d.contigs, d.chr_table, self.gtf)
        self.P = cl.default_params(**kw)
        st, act, _ = op.map_all_rounds(self.P, self.ohi, cl.ReadBatch(d.seq1, d.seq2))
        self.prefix, self.r1, self.r2 = remain_files_from_states(self.tmp, d, self.P, st, act, self.hi.n_contigs)
        self.s1, self.s2 = cl.sort_remain(self.r1), cl.sort_remain(self.r2)
        self._rd = cl.FastqReader(self.s1, self.s2, d.chr_table, self.P.max_ed)      # (owns the batch's memory)
        self.b = self._rd.next_batch(1 << 30)
        self.problems = [cl.circ_chain_list(self.P, self.hi.annots[c], d.chr_table, self.b, c) for c in range(self.hi.n_contigs)]
        self._host = {}

    def host(self, con, window=0, P=None):
        """cm_circ_chain_host's answers for the contig's problems (computed once per window with the set's own parameters)"""
        req, _, seqs = self.problems[con]
        if P is not None:
            return cl.circ_chain_host(P, self.hi.annots[con], self.hi.contigs[con], seqs, req, window)
        if (con, window) not in self._host:
            self._host[con, window] = cl.circ_chain_host(self.P, self.hi.annots[con], self.hi.contigs[con], seqs, req, window)
        return self._host[con, window]


@functools.lru_cache(maxsize=None)
def remain_set(name) -> RemainSet:
    return RemainSet(*SETS[name])


# ---- the listing, from the rule alone ----------------------------------------------------------------------------------
_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A"), ord("N"): ord("N"),
         ord("a"): ord("T"), ord("c"): ord("G"), ord("g"): ord("C"), ord("t"): ord("A"), ord("n"): ord("N")}


def oriented(seq: bytes, forward: bool) -> bytes:
    return seq if forward else bytes(_COMP.get(ch, 0) for ch in reversed(seq))


def _unmapped_side(qspos, qepos, rlen):
    return (1, qspos - 1) if (qspos - 1) > (rlen - qepos) else (qepos + 1, rlen)


def py_list_requests(av, chr_table, b, contig, ws=8):
    """pair-major, genes in the interval's order, piece 0 then 1; CHIBSJ: the split mate's unmapped side, CHI2BSJ: both"""
    giv_s = np.ctypeslib.as_array(av.giv_spos, (av.n_giv,)) if av.n_giv else np.zeros(0, np.uint32)
    giv_e = np.ctypeslib.as_array(av.giv_epos, (av.n_giv,)) if av.n_giv else np.zeros(0, np.uint32)
    goff = np.ctypeslib.as_array(av.giv_gene_off, (av.n_giv + 1,))
    gene = np.ctypeslib.as_array(av.giv_gene, (max(int(goff[-1]), 1),))
    gs, ge = np.ctypeslib.as_array(av.gene_start, (av.n_gene,)), np.ctypeslib.as_array(av.gene_end, (av.n_gene,))
    chr_start = [row[2] for row in chr_table]                # (name, contig, start, len)
    req, pair_of, seqs = [], [], bytearray()
    for i in range(b.n):
        st = b.prior[i]
        if st["type"] not in (CM_CHIBSJ, CM_CHI2BSJ) or st["contig_num"] != contig or not (0 <= st["chr_id"] < len(chr_table)):
            continue
        mates = [b.seq(i, 1), b.seq(i, 2)]
        fw = [bool(st["r1_forward"]), bool(st["r2_forward"])]
        sides = [_unmapped_side(int(st["qspos_r1"]), int(st["qepos_r1"]), len(mates[0])), _unmapped_side(int(st["qspos_r2"]), int(st["qepos_r2"]), len(mates[1]))]
        long_enough = [qe - qs + 1 >= ws for qs, qe in sides]
        if st["type"] == CM_CHIBSJ:
            k = 0 if st["mlen_r1"] < st["mlen_r2"] else 1
            if not long_enough[k]:
                continue
            use = [k]
        else:
            if not any(long_enough):
                continue
            use = [0, 1]
        pos = int(st["spos_r1"]) + chr_start[int(st["chr_id"])]
        g = int(np.searchsorted(giv_s, pos, side="right")) - 1
        if g < 0 or giv_e[g] < pos or goff[g + 1] == goff[g]:
            continue
        offs = {}
        for k in use:
            offs[k] = len(seqs)
            seqs += oriented(mates[k], fw[k])
        for x in range(int(goff[g]), int(goff[g + 1])):
            for k in use:
                req.append((int(gs[gene[x]]), int(ge[gene[x]]), offs[k], len(mates[k]), sides[k][0], sides[k][1], k))
                pair_of.append(i)
    return np.array(req, dtype=cl.CIRC_CHAIN_REQ_DTYPE), np.array(pair_of, np.uint64), np.frombuffer(bytes(seqs), np.uint8)


# ---- directed problems -------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


class Directed:
    """A fabricated contig with fabricated genes (the annotation is the tiny set's: its look-ups run on bare gene offsets) and the
    problems the issue lists.  groups: name -> request indices."""

    def __init__(self, ws=8):
        rng = np.random.default_rng(77)
        contig = bytearray(_rand(rng, 300))
        genes, reqs, seqs, self.groups = {}, [], bytearray(), {}

        def gene(name, body):
            contig.extend(_rand(rng, 50))
            genes[name] = (len(contig) + 1, len(contig) + len(body))          # 1-based inclusive
            contig.extend(body)

        def ask(group, gname, mate, qs, qe):
            self.groups.setdefault(group, []).append(len(reqs))
            reqs.append((genes[gname][0], genes[gname][1], len(seqs), len(mate), qs, qe, 0))
            seqs.extend(mate)

        plain = _rand(rng, 4000)
        gene("plain", plain)
        mate = plain[1000:1150]
        for span in (ws - 1, ws, ws + 2, ws + 3):
            ask("spans", "plain", mate, 5, 5 + span - 1)
        ask("spans", "plain", mate, 1, 150)
        ask("invalid", "plain", b"N" * 150, 1, 150)
        ask("invalid", "plain", b"ACGT\0ACGTN" * 15, 1, 150)
        no_t = bytes(rng.choice(np.frombuffer(b"ACG", np.uint8), 1500).tobytes())          # a gene without T: no seed of a poly-T tail hits it
        gene("no_t", no_t)
        ask("trailing", "no_t", no_t[700:760] + b"T" * 80, 1, 140)
        ask("lowercase", "plain", mate.lower(), 1, 150)
        # a unit repeated 63 / 64 / 65 times with spacers: lists of that many hits, many chains of one score
        for copies in (63, 64, 65):
            unit = _rand(rng, 48)
            gene(f"rep{copies}", b"".join(unit + _rand(rng, 30 + 3 * (c % 5)) for c in range(copies)))
            ask("family", f"rep{copies}", unit + _rand(rng, 20), 1, 60)
            ask("family", f"rep{copies}", unit, 1, 48)
        # tandem copies: every seed of the mate has 500 / 501 hits (seed_lim 500: listed, or listed with n = 0)
        for copies in (500, 501):
            unit = _rand(rng, 21)
            gene(f"tandem{copies}", unit * copies)
            ask("seed_lim", f"tandem{copies}", unit * 3, 1, 63)
        # the two halves of the mate lie in the gene in the opposite order, and only one seed of each half is listed: no improvement
        gene("swapped", plain[3000:3008] + _rand(rng, 200) + plain[500:508])
        ask("no_improvement", "swapped", plain[500:508] + b"N" + plain[3000:3008], 1, 17)
        ask("no_improvement", "swapped", plain[500:508], 1, 8)
        # genes genome_at refuses: one that ends beyond the contig (added last), one that "starts at 0"
        contig.extend(_rand(rng, 50))
        genes["beyond"] = (len(contig) - 100, len(contig) + 40)
        ask("refused_genes", "beyond", bytes(contig[-100:-20]), 1, 80)
        genes["zero"] = (0, 500)
        ask("refused_genes", "zero", bytes(contig[0:100]), 1, 100)
        genes["first"] = (1, 280)
        ask("first_gene", "first", bytes(contig[10:130]), 1, 120)
        genes["short"] = (400, 400 + ws - 2)
        ask("short_gene", "short", bytes(contig[399:399 + 60]), 1, 60)
        self.contig = np.frombuffer(bytes(contig), np.uint8)
        self.genes = genes
        self.req = np.array(reqs, dtype=cl.CIRC_CHAIN_REQ_DTYPE)
        self.seqs = np.frombuffer(bytes(seqs), np.uint8)


@functools.lru_cache(maxsize=None)
def directed(ws=8) -> Directed:
    return Directed(ws)


def junction_problems(s: RemainSet, con=0, min_intron=1000, most=12):
    """Mates that run over an annotated junction with an intron longer than min_intron, asked against a "gene" that starts at
    position 1 of the contig: the reference runs its annotation look-ups on bare gene offsets, so only there (offset = position - 1,
    and a junction's two distances shift against each other) does a chain cross an intron -- and only there can max_intron bind."""
    av, g = s.hi.annots[con], s.hi.contigs[con]
    se = np.ctypeslib.as_array(av.seg_end, (av.n_seg,)).astype(np.int64)
    ss = np.ctypeslib.as_array(av.seg_start, (av.n_seg,)).astype(np.int64)
    nx = np.ctypeslib.as_array(av.seg_next_exon_beg, (av.n_seg,)).astype(np.int64)
    req, seqs = [], bytearray()
    for k in np.nonzero((nx > 0) & (nx - se > min_intron) & (se - ss >= 60) & (nx + 400 < len(g)))[0][:most]:
        mate = bytes(g[se[k] - 50:se[k]]) + bytes(g[nx[k] - 1:nx[k] + 49])
        req.append((1, int(nx[k]) + 300, len(seqs), len(mate), 1, len(mate), 0))
        seqs += mate
    return np.array(req, dtype=cl.CIRC_CHAIN_REQ_DTYPE), np.frombuffer(bytes(seqs), np.uint8)
