"""cm_detect_run against the two-call flows on the bench's workload, in ONE process on ONE box (numbers of different boxes do not
compare, see ab_multi.py).  Not run by the suite.  The sibling of remain_sorted_rate.py: the same files (8.39 M pairs of hg38like in
eight 2^20-pair batches, contigs from the packed FASTA, tables built on the device).
Variants, alternating, REPS times each:
  (a) cm_mapping_run + cm_circ_run, no variable set;
  (b) the same with all seven opt-ins set (CM_FASTQ_DEVICE, CM_PAM_DEVICE, CM_SAM_DEVICE, CM_REMAIN_DEVICE, CM_REMAIN_SORTED,
      CM_CIRC_PRESORTED, CM_CIRC_DEVICE);
  (c) cm_detect_run, memory hand-over;
  (d) cm_detect_run, files hand-over.
Per run: wall seconds per phase (load, map, hand-over, calling, and the whole), the allocation count of the chain calls
(CM_CIRC_TRACE's `workspace:` lines, read from fd 2), the counts; the output files of all variants must be the same bytes.  For (a)
and (b) "hand-over" is what cm_circ_run spends before the calling starts (sorts, genome, GTF, parse: its trace's laps) and the whole
is the sum of the two calls.  Writes OUT after every run.
env: WORKLOAD (hg38like), PAIRS (8388608), BATCH (1048576), REPS (2), THREADS (16), TMPFS (/dev/shm), VARIANTS (abcd),
OUT (profiles/detect_run.json), COMMIT (the commit to record where the tree has no git metadata), DEVICE (the device's name where
neither rocminfo nor the runtime gives one)"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np
import bench
from circminer_amd import lib as cl, synth

wl = os.environ.get("WORKLOAD", "hg38like")
n_pairs = int(os.environ.get("PAIRS", 1 << 23))
batch = int(os.environ.get("BATCH", 1 << 20))
reps = int(os.environ.get("REPS", "2"))
threads = int(os.environ.get("THREADS", "16"))
tmpfs = os.environ.get("TMPFS", "/dev/shm")
variants = os.environ.get("VARIANTS", "abcd")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "detect_run.json"))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
OPT_INS = ("CM_FASTQ_DEVICE", "CM_PAM_DEVICE", "CM_SAM_DEVICE", "CM_REMAIN_DEVICE", "CM_REMAIN_SORTED", "CM_CIRC_PRESORTED", "CM_CIRC_DEVICE")
res = {"workload": wl, "pairs": n_pairs, "batch_pairs": batch, "threads": threads, "date": time.strftime("%Y-%m-%d"), "runs": []}
try:
    res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or os.environ.get("COMMIT")
except OSError:
    res["commit"] = os.environ.get("COMMIT")


def save():
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


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


def chain_calls(text):
    """(calls, allocations summed, bytes held at the end) of the `workspace:` lines"""
    m = re.findall(r"workspace: (\d+) allocations, (\d+) held", text)
    return {"chain_calls": len(m), "allocations": sum(int(a) for a, _ in m), "held_bytes": int(m[-1][1]) if m else 0}


def lap(text, what):
    m = re.search(re.escape(what) + r" ([0-9.]+) s", text)
    return float(m.group(1)) if m else None


t = time.perf_counter()
d = synth.generate(wl, n_pairs=min(n_pairs, 1 << 21), seed=38)
print(f"{wl}: generated in {time.perf_counter() - t:.1f} s", flush=True)
base = os.path.join(tmpfs, f"cm_detect_{os.getpid()}")
shutil.rmtree(base, ignore_errors=True)
os.makedirs(base)
try:
    names = [l.split(":", 1)[1].strip() for l in subprocess.run(["rocminfo"], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l]
    res["device"] = ([x for x in names if "Instinct" in x or "MI3" in x] or [None])[0]
except OSError:
    pass
if not res.get("device"):
    try:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    except Exception:
        res["device"] = os.environ.get("DEVICE")
try:
    packed = os.path.join(base, "ref.fa.packed.fa")
    with open(packed, "wb") as f:
        for ci, c in enumerate(d.contigs):
            f.write(b">%d\n" % (ci + 1))
            np.ascontiguousarray(c).tofile(f)
            f.write(b"\n")
    info = packed + ".index.info"
    with open(info, "w") as f:
        for name, con, start, ln in d.chr_table:
            f.write(f"{con}\t{start}\t{start + ln}\t{name}\n")
    gtf = os.path.join(base, "ref.gtf")
    with open(gtf, "w") as f:
        f.write(d.gtf_text)
    fq = [os.path.join(base, f"reads_{m}.fq") for m in (1, 2)]
    have = d.seq1.shape[0]
    for m, arr in ((0, d.seq1), (1, d.seq2)):
        open(fq[m], "wb").close()
        for a in range(0, n_pairs, have):
            bench.write_fastq_fixed(fq[m], arr[:min(have, n_pairs - a)], m + 1, first=a, append=True)
    res["fastq_bytes"] = os.path.getsize(fq[0]) + os.path.getsize(fq[1])
    print(f"files written at {time.perf_counter() - t:.1f} s", flush=True)
    P = cl.default_params(kmer=20)
    os.environ["CM_CIRC_TRACE"] = "1"
    digests = {}
    for rep in range(reps):
        for v in variants:
            for var in OPT_INS:
                if v == "b":
                    os.environ[var] = "1"
                else:
                    os.environ.pop(var, None)
            out = os.path.join(base, f"run_{v}")
            row = {"variant": v, "rep": rep}
            t0 = time.perf_counter()
            with Stderr() as err:
                if v in "ab":
                    st = cl.run_mapping(packed, gtf, fq[0], fq[1], out, P, report=0, n_threads=threads, batch_pairs=batch, index_info=info)
                    t1 = time.perf_counter()
                    cs = cl.run_circ(packed, gtf, out, st.rounds, P, n_threads=threads, index_info=info)
                    t2 = time.perf_counter()
                    row.update(load_s=st.seconds_load, map_s=st.seconds_map, stage1_wall_s=t1 - t0, stage2_wall_s=t2 - t1, calling_s=cs.seconds,
                               handover_s=(t2 - t1) - cs.seconds, device_parsed_batches=int(st.device_parsed_batches), pairs=int(st.pairs), bsj_pairs=int(st.bsj_pairs),
                               calls=int(cs.calls))
                else:
                    ds = cl.run_detect(packed, gtf, fq[0], fq[1], out, P, report=0, n_threads=threads, batch_pairs=batch, index_info=info, handover=0 if v == "c" else 1)
                    row.update(load_s=ds.map.seconds_load, map_s=ds.map.seconds_map, handover_s=ds.seconds_handover, calling_s=ds.circ.seconds,
                               handover_used=int(ds.handover_used), problems=int(ds.problems), refused=int(ds.refused), recomputed=int(ds.recomputed),
                               device_parsed_batches=int(ds.map.device_parsed_batches), pairs=int(ds.map.pairs), bsj_pairs=int(ds.map.bsj_pairs), calls=int(ds.circ.calls),
                               detect_total_s=ds.seconds_total)
                    rounds = ds.map.rounds
            row["wall_s"] = time.perf_counter() - t0
            row.update(chain_calls(err.text))
            row["circ_trace"] = [ln for ln in err.text.split("\n") if ln.startswith("[circ]") and "workspace:" not in ln]
            rounds = st.rounds if v in "ab" else rounds
            names = [f"{out}_{rounds}_remain_R1.fastq", f"{out}_{rounds}_remain_R2.fastq", out + ".candidates.pam", out + ".circ_report"]
            row["sha1"] = [hashlib.sha1(open(p, "rb").read()).hexdigest() for p in names]
            digests.setdefault("first", row["sha1"])
            row["files_equal_to_first_run"] = row["sha1"] == digests["first"]
            res["runs"].append(row)
            print(json.dumps({k: row[k] for k in row if k not in ("sha1", "circ_trace")}), flush=True)
            save()
            for p in names + [n + ".srt" for n in names[:2]]:
                if os.path.exists(p):
                    os.remove(p)
    res["outputs_identical"] = all(r["files_equal_to_first_run"] for r in res["runs"])
    res["median_wall_s"] = {v: float(np.median([r["wall_s"] for r in res["runs"] if r["variant"] == v])) for v in variants}
    save()
    assert res["outputs_identical"]
finally:
    for var in OPT_INS + ("CM_CIRC_TRACE",):
        os.environ.pop(var, None)
    shutil.rmtree(base, ignore_errors=True)
print("written:", out_path)
