"""Stage 2 with its seeds and chains on the device against the host path, alternating in ONE process on ONE box (numbers of
different boxes do not compare: NOTES 62 - 69).  Not run by the suite.
  input: the sorted remain pairs of one hg38like batch, made as tests/test_gpu_hg38like.py::_stage2 makes them (three rounds on the
         device, remain files of the active pairs, cm_sort_remain, parsed back);
  (a) cm_circ_call, the path without CM_CIRC_DEVICE, at THREADS threads;
  (b) cm_circ_call_device at THREADS threads (its counts and device times from the CM_CIRC_TRACE line);
  REPS times each, alternating; the two files of (b) must be (a)'s bytes.
  Then the problems themselves: cm_circ_chain_host over every contig's listing (cells, log events, the longest log of one problem:
  the data behind the default of CM_CIRC_LOG_CAP), and -- with PROF_LIB=<a -DCM_S2_PROF build of the library> -- the split of one
  thread's time in (a) on this input.
env: PAIRS (1000000), REPS (3), THREADS (16), OUT (profiles/circ_chain_device.json), PROF_LIB, COMMIT"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np
from circminer_amd import lib as cl, synth
from stage2_util import remain_files_of_active

n_pairs = int(os.environ.get("PAIRS", "1000000"))
reps = int(os.environ.get("REPS", "3"))
threads = os.environ.get("THREADS", "16")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "circ_chain_device.json"))


class Stderr:
    """what the library prints to fd 2 inside the block"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.keep = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.keep, 2)
        os.close(self.keep)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        sys.stderr.write(self.text)


res = {"workload": "hg38like", "pairs": n_pairs, "threads": int(threads), "reps": reps, "date": time.strftime("%Y-%m-%d")}
try:
    res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or os.environ.get("COMMIT")
except OSError:
    res["commit"] = os.environ.get("COMMIT")


def save():
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


t = time.perf_counter()
d = synth.generate("hg38like", n_pairs=n_pairs, seed=38)
tmp = tempfile.mkdtemp(prefix="cm_ccrate_")
gtf = os.path.join(tmp, "ref.gtf")
open(gtf, "w").write(d.gtf_text)
P = cl.default_params()
hi = cl.HostIndex(d.contigs, d.chr_table, gtf, kmer=P.kmer, n_threads=int(threads))
print(f"hg38like generated and indexed in {time.perf_counter() - t:.0f} s", flush=True)
hp = cl.HotPath(P)
for ci in range(hi.n_contigs):
    hp.load_contig(ci, hi.views[ci], hi.annots[ci])
hp.upload(cl.ReadBatch(d.seq1[:n_pairs], d.seq2[:n_pairs]))
hp.map_rounds(list(range(hi.n_contigs)), True)
st, cat, act = hp.download()
hp.close()
prefix, r1, r2 = remain_files_of_active(tmp, d, P, st, act, hi.n_contigs)
s1, s2 = cl.sort_remain(r1), cl.sort_remain(r2)
rd = cl.FastqReader(s1, s2, d.chr_table, P.max_ed)
b = rd.next_batch(1 << 30)
res["candidate_pairs"] = b.n
print(f"{b.n} candidate pairs", flush=True)
os.environ["CM_CIRC_THREADS"] = threads
os.environ["CM_CIRC_TRACE"] = "1"
hp = cl.HotPath(P)
legs = {"host": [], "device": []}
trace = ""
for rep in range(reps):
    t = time.perf_counter()
    cl.circ_call(P, hi, d.chr_table, b, prefix + ".a.c", prefix + ".a.r")
    legs["host"].append(time.perf_counter() - t)
    with Stderr() as err:
        t = time.perf_counter()
        cl.circ_call_device(hp, P, hi, d.chr_table, b, prefix + ".b.c", prefix + ".b.r")
        legs["device"].append(time.perf_counter() - t)
    trace = err.text
    assert open(prefix + ".a.c", "rb").read() == open(prefix + ".b.c", "rb").read() and open(prefix + ".a.r", "rb").read() == open(prefix + ".b.r", "rb").read()
    print(f"rep {rep}: host {legs['host'][-1]:.3f} s, device {legs['device'][-1]:.3f} s", flush=True)
hp.close()
res["seconds"] = legs
res["pairs_per_s"] = {k: b.n / float(np.median(v)) for k, v in legs.items()}
m = re.search(r"(\d+) problems, (\d+) genes, (\d+) table bytes, (\d+) gene groups, (\d+) cells, (\d+) log events, (\d+) refused, tables ([\d.]+) ms, chaining ([\d.]+) ms", trace)
if m:
    keys = ("problems", "distinct_genes_summed_over_calls", "table_bytes_largest_group", "gene_groups", "cells", "log_events", "refused")
    res["device_run"] = dict(zip(keys, map(int, m.groups()[:7])), tables_ms=float(m.group(8)), chaining_ms=float(m.group(9)))
m = re.search(r"(\d+) answers taken, (\d+) problems recomputed", trace)
if m:
    res["answers_taken"], res["recomputed_on_host"] = int(m.group(1)), int(m.group(2))
save()

# the problems themselves: sizes, and what the host twin needs for them on one thread
prob = {"problems": 0, "seq_bytes": 0, "cells": 0, "log_events": 0, "longest_log": 0, "distinct_genes": 0, "gene_bytes": 0, "host_twin_s": 0.0, "max_listed": 0}
for con in range(hi.n_contigs):
    req, pair_of, seqs = cl.circ_chain_list(P, hi.annots[con], d.chr_table, b, con)
    if len(req) == 0:
        continue
    t = time.perf_counter()
    h = cl.circ_chain_host(P, hi.annots[con], hi.contigs[con], seqs, req)
    prob["host_twin_s"] += time.perf_counter() - t
    genes = np.unique(np.stack([req["gene_start"], req["gene_end"]], 1), axis=0)
    prob["problems"] += len(req)
    prob["seq_bytes"] += len(seqs)
    prob["cells"] += h.stats[3]
    prob["log_events"] += h.stats[4]
    prob["longest_log"] = max(prob["longest_log"], h.stats[7])
    prob["distinct_genes"] += len(genes)
    prob["gene_bytes"] += int((genes[:, 1].astype(np.int64) - genes[:, 0] + 1).sum())
    prob["max_listed"] = max(prob["max_listed"], int(h.res["listed"].max()))
prob["upload_bytes"] = prob["seq_bytes"] + 32 * prob["problems"] + prob["gene_bytes"]          # mates + requests + gene spans (unmerged: an upper bound)
res["problems"] = prob
save()

lib = os.environ.get("PROF_LIB")
if lib and os.path.exists(lib):
    # one thread of (a) in a -DCM_S2_PROF build: a second copy of the library, called through ctypes with this process's index and batch
    import ctypes as C
    L2 = C.CDLL(lib)
    n_con = hi.n_contigs
    views = (cl.IndexView * n_con)(*hi.views)
    chrs = cl.chr_array(list(d.chr_table))
    stt = cl.CircStats()
    os.environ["CM_CIRC_THREADS"] = "1"
    L2.cm_circ_call.restype = C.c_int
    with Stderr() as err:
        rc = L2.cm_circ_call(C.byref(P), 0, n_con, views, hi.annots, chrs, len(d.chr_table), C.byref(b.fb), (prefix + ".p.c").encode(), (prefix + ".p.r").encode(), C.byref(stt))
    m = re.search(r"table build ([\d.]+), chains_of ([\d.]+), realign_at ([\d.]+) \(inside judge\), place_piece ([\d.]+), judge_single ([\d.]+), process total ([\d.]+)", err.text)
    if rc == 0 and m:
        tb, ch, ra, pl, js, tot = map(float, m.groups())
        res["s2_prof_one_thread_ms"] = {"table_build": tb, "chains_of": ch, "realign_at": ra, "place_piece": pl, "judge_single": js, "process_total": tot,
                                        "tables_and_chains_share": (tb + ch) / tot if tot else None}
    save()
print(json.dumps(res, indent=1))
