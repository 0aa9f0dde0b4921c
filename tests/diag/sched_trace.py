"""The schedule of cm_map_rounds as text, one file per scenario: every wait, record, host wait, memset, copy and kernel launch the
library issues, in issue order (tests/diag/sched_trace.h, force-included into a build of the library).  Two builds that write the
same files queue the same work on the same streams behind the same events, in the same allocations, with the same kernel
arguments (NOTES 58: made to compare a rewrite of the round scheduler with its parent; NOTES 71: the producer side of a batch --
cm_reads_stage_text with every kept array, cm_reads_upload / cm_reads_stage with carried states, the readers of kept data).
    python tests/diag/sched_trace.py OUT_DIR             one trace file per scenario into OUT_DIR (+ line count and digest of each)
    python tests/diag/sched_trace.py --compare DIR DIR   file by file: identical or not
env CM_LIB: the trace build of another tree (default: this tree's, built here: CM_EXTRA_FLAGS="-include .../sched_trace.h",
_build.build(tag="trace")).  Every scenario runs in a child process of its own (one context, its own time limit; the knobs are
read once per process), one after the other; the first that fails ends the run."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

TWO, THREE, PRE2 = {"CM_TILE_PAIRS": "600"}, {"CM_TILE_PAIRS": "400"}, {"CM_TILE_PAIRS": "300"}
# name: (what the child runs, environment).  Data: the tiny2r set of the test fixtures (1 200 pairs, two contigs).
SCENARIOS = {
    "a_one_tile": ("rounds", {}),
    "b_two_tiles": ("rounds", TWO),
    "c_three_tiles": ("rounds", THREE),
    "d_prefetch": ("prefetch", {}),                       # the calls of test_cross_batch_prefetch_is_used_and_discarded_correctly
    "e_prefetch_two_tiles": ("prefetch", PRE2),
    "f_late_launches": ("rounds", dict(TWO, CM_HEAVY_COST="2", CM_HP_TASKS_CAP="40", CM_HP_UNP_CAP="24")),   # late fall-back + re-run
    "g_pool_retries": ("rounds", {"CM_POOL_BYTES": "65536"}),
    "g2_pool_4k": ("rounds", {"CM_POOL_BYTES": "4096"}),                # (64 KB are enough for this data set: no retry there)
    "h_no_pipeline": ("rounds", dict(TWO, CM_HEAVY_PIPELINE="0")),
    "i_one_attempt": ("rounds", dict(TWO, CM_HP_ATTEMPTS="1")),
    "j_mapping_run": ("run", {}),                         # cm_mapping_run's calls for 3 000 pairs in batches of 1 024 (1 024, 1 024, 952)
    "k_stage_text": ("text", {}),                         # the calls of test_staged_text_maps_like_staged_reads with bits 2 | 3 | 4, the readers of kept data
    "l_prior": ("prior", {}),                             # the tail of test_staged_batches_overlap_and_match: upload / stage + swap with carried states
}
KNOBS = ["CM_TILE_PAIRS", "CM_HEAVY_COST", "CM_HP_TASKS_CAP", "CM_HP_UNP_CAP", "CM_POOL_BYTES", "CM_POOL_MAX", "CM_HEAVY_PIPELINE", "CM_HP_ATTEMPTS",
         "CM_HP_TASK_ORDER", "CM_LANE_CLK", "CM_CHAIN_LIGHT_W", "CM_CHAIN_LIGHT_CELLS"]
LIMIT = 120          # seconds per child


def child(what):
    from circminer_amd import lib as cl, synth
    d = synth.generate("tiny2r", n_pairs=1200, seed=22)
    with tempfile.TemporaryDirectory() as td:
        gtf = os.path.join(td, "ref.gtf")
        open(gtf, "w").write(d.gtf_text)
        hi = cl.HostIndex(d.contigs, d.chr_table, gtf, kmer=20)
    hp = cl.HotPath(cl.default_params(kmer=20))
    for ci in range(hi.n_contigs):
        hp.load_contig(ci, hi.views[ci], hi.annots[ci])
    slots = list(range(hi.n_contigs))
    digests = []

    def done():
        digests.append(hashlib.sha1(hp.download()[0].tobytes()).hexdigest()[:12])

    if what == "run":                                     # stage the next batch, map, download, swap: as host_mapping.cpp does
        d = synth.generate("tiny2r", n_pairs=3000, seed=33)
        bs = [hp.pinned_batch(d.seq1[a:a + 1024], d.seq2[a:a + 1024]) for a in range(0, 3000, 1024)]
        hp.stage(bs[0]); hp.swap()
        for k in range(len(bs)):
            if k + 1 < len(bs):
                hp.stage(bs[k + 1])
            hp.map_rounds(slots); done()
            if k + 1 < len(bs):
                hp.swap()
        hp.sync()
    elif what == "text":                                  # two half batches of FASTQ text: swap, prefetch, take-over
        n = d.seq1.shape[0]
        h = n // 2

        def text(arr, mate, lo, hi):
            return b"".join(b"@pair%d%s/%d\n%s\n+\n%s\n" % (i, b"n" * (i % 9), mate, arr[i].tobytes(), b"I" * arr.shape[1]) for i in range(lo, hi))
        a, b = (text(d.seq1, 1, 0, h), text(d.seq2, 2, 0, h)), (text(d.seq1, 1, h, n), text(d.seq2, 2, h, n))
        bits = dict(keep_names=True, keep_quals=True, keep_names2=True)
        hp.stage_text(*a, h, **bits); hp.swap(); hp.stage_text(*b, n, **bits)
        hp.map_rounds(slots); done()                                     # prefetches B's first round
        hp.swap(); hp.stage_text(*a, h, **bits)
        hp.map_rounds(slots); done()                                     # takes it over; prefetches A's
        hp.swap()
        hp.map_rounds(slots); done()
        chrs = list(d.chr_table)
        for rows in (hp.format_pam(chrs)[0], hp.format_sam(chrs)[0], *hp.format_remain(chrs)[:2], *hp.peek_reads(), *hp.peek_quals()):
            digests.append(hashlib.sha1(bytes(rows)).hexdigest()[:12])
        hp.sync()
    elif what == "prior":                                 # carried states from the host (upload) and from the staged record (swap)
        import numpy as np
        batch = cl.ReadBatch(d.seq1, d.seq2)
        hp.upload(batch); hp.map_round(0, False)
        st1, _, act1 = hp.download()
        idx = np.nonzero(act1)[0]
        sub, prior = cl.ReadBatch(d.seq1[idx], d.seq2[idx]), np.ascontiguousarray(st1[idx])
        hp.upload(sub, prior); hp.map_round(1, True); done()
        hp.upload(batch); hp.map_round(0, False)
        hp.stage(sub, prior); hp.swap(); hp.map_round(1, True); done()
        hp.sync()
    elif what == "rounds":                                # both slots in one call
        hp.upload(cl.ReadBatch(d.seq1, d.seq2))
        hp.map_rounds(slots); hp.sync(); done()
    else:
        h = d.seq1.shape[0] // 2
        pa = hp.pinned_batch(d.seq1[:h], d.seq2[:h])
        pb = hp.pinned_batch(d.seq1[h:2 * h], d.seq2[h:2 * h])
        small = hp.pinned_batch(d.seq1[:h // 2], d.seq2[:h // 2])
        hp.stage(pa); hp.swap(); hp.stage(pb)
        hp.map_rounds(slots); done()                                     # prefetches B's first round
        hp.swap(); hp.stage(pa)
        hp.map_rounds(slots); done()                                     # takes it over; prefetches A's
        hp.swap(); hp.stage(pb)
        hp.load_contig(0, hi.views[0], hi.annots[0])                     # slot 0 reloaded: the prefetched chains are stale
        hp.map_rounds(slots); done()
        hp.swap(); hp.stage(pa)
        hp.map_rounds(slots[::-1], last_is_final=False)                  # another first slot: discarded; not the last call: no prefetch
        hp.reset()
        hp.map_rounds(slots); done()
        hp.swap(); hp.stage(small)
        hp.map_rounds(slots); done()                                     # taken over; prefetches the smaller batch
        hp.swap(); hp.stage(pb)                                          # larger than the resident batch: no prefetch
        hp.map_rounds(slots); done()
        hp.sync()
    hp.close()
    print("states", " ".join(digests), flush=True)


def digest(path):
    data = open(path, "rb").read()
    return data.count(b"\n"), hashlib.sha1(data).hexdigest()[:12]


def compare(a, b):
    bad = 0
    for name in SCENARIOS:
        fa, fb = (os.path.join(x, name + ".trace") for x in (a, b))
        if not (os.path.exists(fa) and os.path.exists(fb)):
            print("%-22s missing" % name)
            bad += 1
            continue
        ta, tb = open(fa).read(), open(fb).read()
        if ta == tb:
            print("%-22s identical  %d lines  %s" % ((name,) + digest(fa)))
            continue
        # by-value struct arguments: S<bytes>:<pointer words>:<all bytes> -- the last hash covers padding, which holds stack leftovers
        ma, mb = (re.sub(r"( S\d+:[0-9a-f]+):[0-9a-f]+", r"\1", t).split("\n") for t in (ta, tb))
        if ma == mb:
            n = sum(x != y for x, y in zip(ta.split("\n"), tb.split("\n")))
            print("%-22s equal but for the all-bytes hash of by-value structs in %d of %d lines" % (name, n, len(ma) - 1))
            continue
        first = next((i for i, (x, y) in enumerate(zip(ma, mb)) if x != y), min(len(ma), len(mb)))
        print("%-22s DIFFERENT from line %d:\n  %s\n  %s" % (name, first + 1, ma[first] if first < len(ma) else "", mb[first] if first < len(mb) else ""))
        bad += 1
    return 1 if bad else 0


def main(out_dir):
    if not os.environ.get("CM_LIB"):
        from circminer_amd import _build
        os.environ["CM_EXTRA_FLAGS"] = (os.environ.get("CM_EXTRA_FLAGS", "") + " -include " + os.path.join(HERE, "sched_trace.h")).strip()
        os.environ["CM_LIB"] = _build.build(tag="trace")
    os.makedirs(out_dir, exist_ok=True)
    print("library", os.environ["CM_LIB"], flush=True)
    for name, (what, knobs) in SCENARIOS.items():
        trace = os.path.join(os.path.abspath(out_dir), name + ".trace")
        if os.path.exists(trace):
            os.remove(trace)                               # (the library appends)
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(knobs, CM_SCHED_TRACE=trace)
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", what], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print("%s: exit status %d, stopping here\n%s" % (name, r.returncode, r.stdout[-3000:]), flush=True)
            return 1
        print("%-22s %6d lines  %s   %s" % ((name,) + digest(trace) + (r.stdout.strip().splitlines()[-1],)), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 2:
        sys.exit(main(sys.argv[1]))
    else:
        sys.exit(__doc__)
