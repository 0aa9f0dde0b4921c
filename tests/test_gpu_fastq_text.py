"""cm_reads_stage_text on the device: FASTQ text tokenised by the kernels k_ft_* against the project's host parser cm_fastq_next on
files holding the same bytes -- arrays, verdicts, mapping results, and cm_mapping_run from files to files with CM_FASTQ_DEVICE=1.

The kernels chunk by: 1 KB of text per newline count (cmft::NL_CHUNK), 8192 items per block of both scans (S32_B: 8 MB of text,
8192 records), 256 records per workgroup of the record kernel.  The sizes below cross all of them at least four times."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from circminer_amd import lib as cl
from fastq_text_util import (CARRIED_HEADER, MALFORMED, HostParse, check_against_host, fast_text, malformed, records, text_of, whole_records)

pytestmark = pytest.mark.gpu


class Dev:
    """stage_text -> swap -> peek_reads, in the shape check_against_host compares"""

    def __init__(self, hp, t1: bytes, t2: bytes, max_pairs, flags=3):
        self.rc, self.n, self.err = 0, 0, ""
        try:
            self.tb, self.rec1, self.rec2 = hp.stage_text(t1, t2, max_pairs, eof1=bool(flags & 1), eof2=bool(flags & 2))
        except RuntimeError as e:
            self.err = str(e)
            self.rc = int(self.err.split("(")[1].split(")")[0])
            return
        self.n = int(self.tb.n_pairs)
        if self.n:
            hp.swap()
            self.seq1, self.off1, self.seq2, self.off2 = hp.peek_reads()
        else:
            self.seq1 = self.seq2 = np.zeros(0, np.uint8)
            self.off1 = self.off2 = self.rec1 = self.rec2 = np.zeros(1, np.uint64)


@pytest.fixture(scope="module")
def hp_plain(built):
    hp = cl.HotPath(cl.default_params())
    yield hp
    hp.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4100])
def test_staged_text_equals_host_parser(hp_plain, tmp_path, n):
    """whole files with and without the final line feed, max_pairs below what the block holds, blocks cut inside a header, a line
    and a record (flags 0: the tail is not consumed, used* is the host's record boundary)"""
    hp = hp_plain
    rng = np.random.default_rng(n)
    r1 = records(rng, n, zero_at=(0, n // 2) if n > 1 else (), mate=1)
    r2 = records(rng, n, zero_at=(n - 2,) if n > 1 else (), mate=2)
    for last_nl in (True, False):
        t1, t2 = text_of(r1, last_nl), text_of(r2, last_nl)
        h = HostParse(tmp_path, t1, t2, n + 5, tag=f"w{n}")
        for mp in sorted({n + 5, n, max(1, n // 2)}):
            e = Dev(hp, t1, t2, mp)
            check_against_host(e, h, min(n, mp), t1, t2)
    rec1 = whole_records(t1, True)[0]
    m = n * 2 // 3
    for k, cut in enumerate([int(rec1[m]), int(rec1[m]) + 3, int(rec1[m]) + len(r1[m][0]) + 10, int(rec1[m]) + len(t1[int(rec1[m]):].split(b"\n+")[0]) + 2,
                             len(t1) - 1]):
        b1, b2 = t1[:cut], t2[:cut]
        a1, a2 = whole_records(b1, False)[1], whole_records(b2, False)[1]
        assert a2 <= a1 and (k > 0 or n < 63 or a2 < a1)        # R2's names are longer: a byte cut holds fewer of its records
        e = Dev(hp, b1, b2, n, flags=0)
        check_against_host(e, h, min(a1, a2), b1, b2, eof=False)
        if min(a1, a2) > 2:
            e = Dev(hp, b1, b2, min(a1, a2) - 2, flags=0)
            check_against_host(e, h, min(a1, a2) - 2, b1, b2, eof=False)


def test_staged_text_across_scan_blocks(hp_plain, tmp_path):
    """files of more than four blocks of both scans (> 32 MB of text, > 32768 records), ragged records in front"""
    hp = hp_plain
    rng = np.random.default_rng(77)
    n_big = 135_000
    r1, r2 = records(rng, 500, mate=1, zero_at=(5,)), records(rng, 500, mate=2)
    t1 = text_of(r1) + fast_text(rng, n_big, 70)
    t2 = text_of(r2) + fast_text(rng, n_big, 90)
    assert min(len(t1), len(t2)) > 4 * 8192 * 1024
    n = 500 + n_big
    h = HostParse(tmp_path, t1, t2, n, tag="big")
    e = Dev(hp, t1, t2, n + 1)
    check_against_host(e, h, n, t1, t2)
    cut = len(t1) - 12345
    b1, b2 = t1[:cut], t2[:cut]
    want = min(whole_records(b1, False)[1], whole_records(b2, False)[1])
    check_against_host(Dev(hp, b1, b2, n, flags=0), h, want, b1, b2, eof=False)


def test_blocks_of_a_file_pair_continue(hp_plain, tmp_path):
    """next_text / stage_text / consumed with 64-KB blocks: the concatenated batches are one host-parsed batch, every tail is
    the front of the next block"""
    hp = hp_plain
    rng = np.random.default_rng(21)
    n = 3000
    t1, t2 = text_of(records(rng, n, mate=1, zero_at=(100, 2999))), text_of(records(rng, n, mate=2, zero_at=(0,), name_pad=9), last_newline=False)
    h = HostParse(tmp_path, t1, t2, n, tag="cont")
    rd = cl.FastqReader(*h.paths)
    seqs, lens, pos, tails = ([], []), ([], []), [0, 0], 0
    for it in range(200):
        b1, e1, b2, e2 = rd.next_text(64 << 10)
        assert bytes(b1) == t1[pos[0]:pos[0] + len(b1)] and bytes(b2) == t2[pos[1]:pos[1] + len(b2)]          # the tail was carried
        if len(b1) == 0 and e1:
            break
        tb, rec1, rec2 = hp.stage_text(b1, b2, 150 if it % 4 == 3 else 1 << 20, eof1=e1, eof2=e2)
        assert tb.n_pairs > 0
        hp.swap()
        s1, o1, s2, o2 = hp.peek_reads()
        for x, (s, o) in enumerate(((s1, o1), (s2, o2))):
            seqs[x].append(s)
            lens[x].append(np.diff(o))
        tails += (tb.used1 < len(b1)) + (tb.used2 < len(b2))
        rd.consumed(tb.used1, tb.used2)
        pos[0] += tb.used1
        pos[1] += tb.used2
    rd.close()
    assert pos[0] == len(t1) and it > 10 and tails > it
    for x, (hs, ho) in enumerate(((h.seq1, h.off1), (h.seq2, h.off2))):
        assert np.array_equal(np.concatenate(lens[x]), np.diff(ho)) and np.array_equal(np.concatenate(seqs[x]), hs)


@pytest.fixture(scope="module")
def mapped(ds_tiny2r, tmp_path_factory):
    """a context with the two contigs of ds_tiny2r, its reads as FASTQ text, and what stage(host-parsed) + map_rounds gives"""
    from stage2_util import write_fastq_pair
    ds = ds_tiny2r
    hp = cl.HotPath(cl.default_params(kmer=ds.kmer))
    for ci in range(ds.hi.n_contigs):
        hp.load_contig(ci, ds.hi.views[ci], ds.hi.annots[ci])
    slots = list(range(ds.hi.n_contigs))
    tmp = tmp_path_factory.mktemp("ft_map")
    p1, p2 = write_fastq_pair(tmp, ds.d, ds.batch.n)
    t1, t2 = open(p1, "rb").read(), open(p2, "rb").read()
    rd = cl.FastqReader(p1, p2)
    b = rd.next_batch(ds.batch.n)
    hp.stage(b)
    hp.swap()
    hp.map_rounds(slots)
    want = hp.download()
    rd.close()
    yield hp, slots, t1, t2, want
    hp.close()


def _maps_like(hp, slots, t1, t2, want, lo, hi):
    """pairs [lo, hi) of the text staged, mapped: the states, categories and flags of the host-staged run"""
    r1, r2 = whole_records(t1, True)[0], whole_records(t2, True)[0]
    tb, _, _ = hp.stage_text(t1[int(r1[lo]):int(r1[hi])], t2[int(r2[lo]):int(r2[hi])], hi - lo)
    assert tb.n_pairs == hi - lo
    hp.swap()
    hp.map_rounds(slots)
    got = hp.download()
    for g, w in zip(got, want):
        assert g.tobytes() == w[lo:hi].tobytes()


def test_refusals_and_the_batch_after_them(mapped, tmp_path):
    """every malformed case of either file in the first, a middle and the last record is CM_EINVAL with the file and the record
    in the message; the legal look-alikes pass; after every refusal the context maps the next good batch correctly"""
    hp, slots, g1, g2, want = mapped
    rng = np.random.default_rng(11)
    n = 40                                       # ~ 9 KB per file: records straddle the 1-KB newline chunks
    r1, r2 = records(rng, n, mate=1), records(rng, n, mate=2)
    good = 0
    for f in (0, 1):
        for i in (0, n // 2, n - 1):
            for how in MALFORMED:
                b = [r1, r2]
                b[f] = malformed(b[f], i, how)
                t1, t2 = text_of(b[0]), text_of(b[1])
                assert HostParse(tmp_path, t1, t2, n, tag="bad").rc == -1
                e = Dev(hp, t1, t2, n)
                assert e.rc == -1 and f"file {f + 1}, record {i} " in e.err, (f, i, how, e.err)
                with pytest.raises(RuntimeError, match="no staged batch"):
                    hp.swap()                                                  # nothing was staged
                _maps_like(hp, slots, g1, g2, want, good, good + 50)          # ... and the context is as good as before
                good = (good + 50) % 1000
    q = [list(x) for x in r1]                    # '@' in front of a quality line, '+' in front of a sequence: records are counted by line
    q[3][3] = b"@" + q[3][3][1:]
    q[4][1] = b"+" + q[4][1][1:]
    t1, t2 = text_of(q), text_of(r2)
    check_against_host(Dev(hp, t1, t2, n), HostParse(tmp_path, t1, t2, n, tag="at"), n, t1, t2)
    for tail in (b"\n", b"@x\nACGT\n+"):         # lines behind the last whole record at the end of the input
        for f in (0, 1):
            t = [text_of(r1), text_of(r2)]
            t[f] += tail
            assert HostParse(tmp_path, t[0], t[1], n + 1, tag="tail").rc == Dev(hp, t[0], t[1], n + 1).rc == -1
            assert Dev(hp, t[0], t[1], n).n == n and Dev(hp, t[0], t[1], n + 1, flags=3 ^ (1 << f)).n == n
    t1, t2 = text_of(r1), text_of(r2[:n - 3])    # R2 ends before R1
    assert HostParse(tmp_path, t1, t2, n, tag="short").rc == Dev(hp, t1, t2, n).rc == -1
    assert Dev(hp, t1, t2, n - 3).n == n - 3 and Dev(hp, t1, t2, n, flags=1).n == n - 3
    t1, t2 = text_of(r1[:n - 3]), text_of(r2)    # surplus R2 records are ignored
    check_against_host(Dev(hp, t1, t2, n), HostParse(tmp_path, t1, t2, n, tag="short"), n - 3, t1, t2)
    c = [list(x) for x in r1]                    # the carried header: refused in R1, nobody's business in R2
    c[n // 2][0] = CARRIED_HEADER
    e = Dev(hp, text_of(c), text_of(r2), n)
    assert e.rc == -1 and "carried state" in e.err and f"record {n // 2} " in e.err
    _maps_like(hp, slots, g1, g2, want, 1000, 1200)
    c2 = [list(x) for x in r2]
    c2[n // 2][0] = CARRIED_HEADER
    t1, t2 = text_of(r1), text_of(c2)
    check_against_host(Dev(hp, t1, t2, n), HostParse(tmp_path, t1, t2, n, tag="car"), n, t1, t2)
    lg = [list(x) for x in r2]                   # a read of max_read_len + 1
    lg[5][1], lg[5][3] = b"A" * 301, b"I" * 301
    e = Dev(hp, text_of(r1), text_of(lg), n)
    assert e.rc == -1 and "max_read_len" in e.err
    lg[5][1], lg[5][3] = b"A" * 300, b"I" * 300
    assert Dev(hp, text_of(r1), text_of(lg), n).tb.max_len == 300
    e = Dev(hp, b"", b"", 10)
    assert e.rc == 0 and e.n == 0
    _maps_like(hp, slots, g1, g2, want, 0, 1200)


def test_staged_text_maps_like_staged_reads(mapped):
    """stage_text + map_rounds == stage(host-parsed) + map_rounds, also when the staged text batch's first round is taken over
    from the cross-batch prefetch (launches[7])"""
    hp, slots, t1, t2, want = mapped
    n = len(want[0])
    h = n // 2
    r1, r2 = whole_records(t1, True)[0], whole_records(t2, True)[0]
    a = (t1[:int(r1[h])], t2[:int(r2[h])])
    b = (t1[int(r1[h]):], t2[int(r2[h]):])
    _maps_like(hp, slots, t1, t2, want, 0, n)
    hp.prof(True)
    hp.prof_reset()

    def taken():
        return hp.prof_get()[1][7]

    assert hp.stage_text(*a, h)[0].n_pairs == h
    hp.swap()
    assert hp.stage_text(*b, n)[0].n_pairs == n - h
    hp.map_rounds(slots)                                   # prefetches B's first round out of the tokeniser's buffers
    assert all(g.tobytes() == w[:h].tobytes() for g, w in zip(hp.download(), want)) and taken() == 0
    hp.swap()
    assert hp.stage_text(*a, h)[0].n_pairs == h
    hp.map_rounds(slots)                                   # takes it over; prefetches A's
    assert all(g.tobytes() == w[h:].tobytes() for g, w in zip(hp.download(), want)) and taken() == 1
    hp.swap()
    hp.map_rounds(slots)
    assert all(g.tobytes() == w[:h].tobytes() for g, w in zip(hp.download(), want)) and taken() == 2
    hp.prof(False)


@pytest.fixture(scope="module")
def run_files(tmp_path_factory):
    from circminer_amd import synth
    from stage2_util import write_fastq_pair
    tmp = tmp_path_factory.mktemp("ft_run")
    n = 2400
    d = synth.generate("tiny2r", n_pairs=n, seed=45, mix=(0.5, 0.2, 0.3))
    fa = str(tmp / "ref.fa")
    with open(fa, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f">{name}\n{d.contigs[con - 1][start:start + ln].tobytes().decode()}\n")
    packed, info = cl.pack_genome(fa, 150_000)
    idx = cl.write_index(packed, kmer=20, n_threads=4)
    gtf = str(tmp / "ref.gtf")
    open(gtf, "w").write(d.gtf_text)
    fq1, fq2 = write_fastq_pair(tmp, d, n, name=lambda i: f"pair{i}" + "y" * (i % 5))
    return tmp, n, idx, gtf, fq1, fq2


def _run(run_files, out, device, monkeypatch, report=0, world=1, fq=None):
    tmp, n, idx, gtf, fq1, fq2 = run_files
    if fq:
        fq1, fq2 = fq
    if device:
        monkeypatch.setenv("CM_FASTQ_DEVICE", "1")
        monkeypatch.setenv("CM_FASTQ_DEVICE_BLOCK", "65536")
    else:
        monkeypatch.delenv("CM_FASTQ_DEVICE", raising=False)
        monkeypatch.delenv("CM_FASTQ_DEVICE_BLOCK", raising=False)
    out = str(tmp / out)
    sts = [cl.run_mapping(idx, gtf, fq1, fq2, out, cl.default_params(kmer=0), report=report, n_threads=4, batch_pairs=512, rank=r, world=world)
           for r in range(world)]
    cl.merge_parts(out, 2, world, report)
    files = tuple(open(f"{out}_2_remain_R{m}.fastq", "rb").read() for m in (1, 2))
    return (sum(s.pairs for s in sts), sum(s.bsj_pairs for s in sts), [sum(s.by_type[t] for s in sts) for t in range(14)],
            [s.device_parsed_batches for s in sts], files, out)


def test_files_to_files_with_the_device_tokeniser(run_files, monkeypatch):
    """cm_mapping_run with CM_FASTQ_DEVICE=1 and 64-KB blocks: the remain files and the counts of the host parser's run, for one
    process and for two ranks on one card"""
    n = run_files[1]
    host = _run(run_files, "host", False, monkeypatch)
    dev = _run(run_files, "dev", True, monkeypatch)
    assert host[0] == dev[0] == n and host[1] == dev[1] > 50 and host[2] == dev[2]
    assert dev[3][0] >= 3 and host[3] == [0]
    assert dev[4] == host[4] and len(host[4][0]) > 10_000
    dev2 = _run(run_files, "dev2", True, monkeypatch, world=2)
    assert dev2[:3] == host[:3] and min(dev2[3]) >= 3 and dev2[4] == host[4]
    assert not [f for f in os.listdir(str(run_files[0])) if ".part" in f]


def test_the_variable_is_ignored_where_the_host_parser_is_needed(run_files, monkeypatch):
    """report = 1 (every pair's name goes to the PAM rows) and gzip input stay on cm_fastq_next: no batch is parsed on the device,
    the files are those of the run without the variable"""
    tmp, n = run_files[0], run_files[1]
    host = _run(run_files, "h1", False, monkeypatch, report=1)
    dev = _run(run_files, "d1", True, monkeypatch, report=1)
    assert dev[3] == [0] and dev[:3] == host[:3] and dev[4] == host[4]
    assert open(dev[5] + ".mapping.pam", "rb").read() == open(host[5] + ".mapping.pam", "rb").read()
    gz = []
    for p in run_files[4:6]:
        gz.append(p + ".gz")
        with gzip.open(gz[-1], "wb", compresslevel=1) as f:
            f.write(open(p, "rb").read())
    dev = _run(run_files, "dz", True, monkeypatch, fq=gz)
    assert dev[3] == [0] and dev[0] == n and dev[4] == host[4]
    # a carried state in the first R1 header: the host parser's for the whole run (the remain files are such input)
    rem = (host[5] + "_2_remain_R1.fastq", host[5] + "_2_remain_R2.fastq")
    h2 = _run(run_files, "hc", False, monkeypatch, fq=rem)
    d2 = _run(run_files, "dc", True, monkeypatch, fq=rem)
    assert d2[3] == [0] and d2[:3] == h2[:3] and d2[4] == h2[4] and d2[0] == host[1]
