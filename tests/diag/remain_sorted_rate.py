"""The device-side order of the remain records against the host sort of stage 2 on the bench's workload, in ONE process on ONE box
(numbers of different boxes do not compare, see ab_multi.py).  Not run by the suite.  The sibling of remain_device_rate.py.
  (a) per batch, alternating: cm_format_remain against cm_format_remain_sorted, both into page-locked buffers: wall, and the
      kernels' own time by HIP events (ms[7] of cm_prof_get under cm_prof_enable); the sort's share is the difference of the two.
      No contig is loaded for this leg: the batches are staged from the FASTQ text and given concordant states with random positions
      below 2.5e8 through cm_state_poke, so EVERY pair of a batch is active (twenty times the set a real run re-queues) and ties
      are the few a random position gives -- no star forms: a batch of them is one tie group above the cap, which the device
      refuses by design;
  (c) cm_mapping_run (report 0) from the FASTQ files to the remain files with CM_FASTQ_DEVICE=1 CM_REMAIN_DEVICE=1, without and with
      CM_REMAIN_SORTED=1, alternating, REPS times each, with the legs of cm_mapping_stats and the merge's seconds (CM_REMAIN_TRACE=1,
      read from fd 2); the remain files of both must be the same bytes;
  (b) cm_circ_run on the files of (c) without and with CM_CIRC_PRESORTED=1, alternating, REPS times each, with its legs
      (CM_CIRC_TRACE=1, read from fd 2); candidates.pam and circ_report of both must be the same bytes.
The contigs come from the packed FASTA (tables built on the device: no index file to write); that time is seconds_load, outside
the rates.  Writes OUT after every leg.
env: WORKLOAD (hg38like), PAIRS (8388608), BATCH (1048576), REPS (2), THREADS (16), TMPFS (/dev/shm),
OUT (profiles/remain_sorted.json), COMMIT (the commit to record where the tree has no git metadata), DEVICE (the device's name
where neither rocminfo nor the runtime gives one)"""
import ctypes as C
import hashlib
import json
import os
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
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "remain_sorted.json"))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
res = {"workload": wl, "pairs": n_pairs, "batch_pairs": batch, "threads": threads, "date": time.strftime("%Y-%m-%d")}
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
        sys.stderr.write(self.text)


t = time.perf_counter()
d = synth.generate(wl, n_pairs=min(n_pairs, 1 << 21), seed=38)
print(f"{wl}: generated in {time.perf_counter() - t:.1f} s", flush=True)
base = os.path.join(tmpfs, f"cm_remainsrt_{os.getpid()}")
shutil.rmtree(base, ignore_errors=True)
os.makedirs(base)
try:
    names = [l.split(":", 1)[1].strip() for l in subprocess.run(["rocminfo"], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l]
    res["device"] = ([x for x in names if "Instinct" in x or "MI3" in x] or [None])[0]
except OSError:
    pass
if not res.get("device"):                                            # (no rocminfo on the PATH: the runtime's own name)
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
    with open(packed + ".index.info", "w") as f:
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
    chrs = list(d.chr_table)

    # (a) the records of every batch, in the set's order and sorted
    hp = cl.HotPath(cl.default_params())
    hp.prof(True)
    rng = np.random.default_rng(1)
    rd_text = cl.FastqReader(fq[0], fq[1], n_threads=threads)
    want = int(res["fastq_bytes"] / n_pairs / 2 * batch * 1.02) + (1 << 16)
    pin = None
    legs = {"unsorted": {"format_s": 0.0, "kernels_s": 0.0}, "sorted": {"format_s": 0.0, "kernels_s": 0.0}, "row_bytes": 0, "batches": 0,
            "active_set": "every pair of the batch (no contig loaded), concordant states at random positions"}
    table = cl.chr_array(chrs)
    got = 0
    k = 0
    while True:
        b1, e1, b2, e2 = rd_text.next_text(want)
        if len(b1) == 0 and e1:
            break
        tb, rec1, rec2 = hp.stage_text(b1, b2, batch, eof1=e1, eof2=e2, keep_names=True, keep_quals=True, keep_names2=True)
        assert tb.n_pairs > 0
        rd_text.consumed(tb.used1, tb.used2)
        hp.swap()
        m = int(tb.n_pairs)
        st = np.zeros(m, cl.MAPPED_DTYPE)
        st["spos_r1"] = rng.integers(1, 250_000_000, m)
        st["spos_r2"] = st["spos_r1"] + rng.integers(0, 400, m)
        st["epos_r1"], st["epos_r2"] = st["spos_r1"] + 149, st["spos_r2"] + 149
        for f in ("qspos_r1", "qspos_r2"):
            st[f] = 1
        for f in ("qepos_r1", "qepos_r2", "mlen_r1", "mlen_r2"):
            st[f] = 150
        st["tlen"] = rng.integers(150, 600, m)
        st["chr_id"] = rng.integers(0, max(len(chrs), 1), m)
        st["r1_forward"] = rng.integers(0, 2, m)
        st["r2_forward"] = 1 - st["r1_forward"]
        st["gm_compatible"] = 1
        hp.poke_states(st)
        nb = (C.c_uint64 * 2)()
        if pin is None:                                              # sized once, outside the timing, by the first batch's records
            hp.L.cm_format_remain(hp.h, table, len(chrs), 0, hp.n, None, 0, None, 0, nb, None, None, None)
            pin = [hp.host_array(int(x / hp.n * batch * 1.1) + (1 << 20), np.uint8) for x in nb]
            keys, offs = hp.host_array(batch + 1, np.int64), [hp.host_array(batch + 2, np.uint32) for _ in (0, 1)]
            for leg in ("unsorted", "sorted"):                       # (and the device buffers of either call grown once)
                if leg == "unsorted":
                    hp.L.cm_format_remain(hp.h, table, len(chrs), 0, hp.n, pin[0].ctypes.data, pin[0].size, pin[1].ctypes.data, pin[1].size, nb, keys.ctypes.data, None, None)
                else:
                    hp.L.cm_format_remain_sorted(hp.h, table, len(chrs), 0, hp.n, pin[0].ctypes.data, pin[0].size, pin[1].ctypes.data, pin[1].size, nb, keys.ctypes.data,
                                                 offs[0].ctypes.data, offs[1].ctypes.data, None, None)
        for leg in (("unsorted", "sorted") if k % 2 == 0 else ("sorted", "unsorted")):
            hp.prof_reset()
            t0 = time.perf_counter()
            if leg == "unsorted":
                rc = hp.L.cm_format_remain(hp.h, table, len(chrs), 0, hp.n, pin[0].ctypes.data, pin[0].size, pin[1].ctypes.data, pin[1].size, nb, keys.ctypes.data, None, None)
            else:
                rc = hp.L.cm_format_remain_sorted(hp.h, table, len(chrs), 0, hp.n, pin[0].ctypes.data, pin[0].size, pin[1].ctypes.data, pin[1].size, nb, keys.ctypes.data,
                                                  offs[0].ctypes.data, offs[1].ctypes.data, None, None)
            assert rc == 0, (rc, hp.L.cm_last_error(hp.h))
            legs[leg]["format_s"] += time.perf_counter() - t0
            legs[leg]["kernels_s"] += hp.prof_get()[0][7] / 1e3
            if leg == "sorted":
                assert bool((np.diff(keys[:m]) >= 0).all())
        legs["row_bytes"] += int(nb[0]) + int(nb[1])
        legs["batches"] += 1
        got += m
        k += 1
    rd_text.close()
    hp.close()
    assert got == n_pairs
    for leg in ("unsorted", "sorted"):
        legs[leg]["kernels_ms_per_2_20_pairs"] = legs[leg]["kernels_s"] * 1e3 / got * (1 << 20)
    legs["sort_share_of_sorted_kernels"] = 1.0 - legs["unsorted"]["kernels_s"] / legs["sorted"]["kernels_s"]
    res["records_per_batch"] = legs
    print(json.dumps(legs), flush=True)
    save()

    # (c) files to files, alternating: the remain files alone, and with the sorted runs beside them
    for var in ("CM_FASTQ_DEVICE", "CM_REMAIN_DEVICE", "CM_REMAIN_TRACE"):
        os.environ[var] = "1"
    runs, files, rounds = [], {}, 0
    for rep in range(reps):
        for srt in (0, 1):
            if srt:
                os.environ["CM_REMAIN_SORTED"] = "1"
            else:
                os.environ.pop("CM_REMAIN_SORTED", None)
            out = os.path.join(base, f"run{srt}")
            with Stderr() as err:
                st = cl.run_mapping(packed, gtf, fq[0], fq[1], out, cl.default_params(kmer=20), report=0, n_threads=threads, batch_pairs=batch,
                                    index_info=packed + ".index.info")
            trace = [ln for ln in err.text.split("\n") if ln.startswith("[remain] sorted runs:")]
            row = {"rep": rep, "sorted_runs": srt, "pairs": int(st.pairs), "bsj_pairs": int(st.bsj_pairs), "device_parsed_batches": int(st.device_parsed_batches),
                   "load_s": st.seconds_load, "map_s": st.seconds_map, "pairs_per_s": st.pairs / st.seconds_map,
                   "parts_s": {"read": st.seconds_parse, "device": st.seconds_device, "write": st.seconds_write}, "trace": trace}
            if srt:
                row["merge_s"] = float(trace[0].split("merge ")[1].split(" ")[0])
                row["batches_sorted_on_host"] = int(trace[0].split(" batches, ")[1].split(" ")[0])
            assert st.pairs == n_pairs and st.device_parsed_batches
            rounds = st.rounds
            runs.append(row)
            print(json.dumps(row), flush=True)
            if rep == 0:
                files[srt] = [hashlib.sha1(open(p, "rb").read()).hexdigest() for p in (f"{out}_{st.rounds}_remain_R1.fastq", f"{out}_{st.rounds}_remain_R2.fastq")]
            res["file_to_file"] = runs
            save()
    for var in ("CM_FASTQ_DEVICE", "CM_REMAIN_DEVICE", "CM_REMAIN_TRACE", "CM_REMAIN_SORTED"):
        os.environ.pop(var, None)
    res["remain_files_identical"] = files[0] == files[1]
    save()
    assert res["remain_files_identical"]

    # (b) stage 2 on the files of the run with the sorted runs: sorting them again against taking them as they are
    os.environ["CM_CIRC_TRACE"] = "1"
    out = os.path.join(base, "run1")
    srt_kept = [open(f"{out}_{rounds}_remain_R{m}.fastq.srt", "rb").read() for m in (1, 2)]
    circ, outs = [], {}
    for rep in range(reps):
        for pre in (0, 1):
            for m in (1, 2):                                         # (the unsorted run overwrites the .srt files: put the merge's back)
                open(f"{out}_{rounds}_remain_R{m}.fastq.srt", "wb").write(srt_kept[m - 1])
            if pre:
                os.environ["CM_CIRC_PRESORTED"] = "1"
            else:
                os.environ.pop("CM_CIRC_PRESORTED", None)
            t0 = time.perf_counter()
            with Stderr() as err:
                cs = cl.run_circ(packed, gtf, out, rounds, cl.default_params(kmer=20), n_threads=threads, index_info=packed + ".index.info")
            row = {"rep": rep, "presorted": pre, "wall_s": time.perf_counter() - t0, "pairs": int(cs.pairs), "calls": int(cs.calls),
                   "legs": [ln for ln in err.text.split("\n") if ln.startswith("[circ]")]}
            circ.append(row)
            print(json.dumps(row), flush=True)
            if rep == 0:
                outs[pre] = [hashlib.sha1(open(out + ext, "rb").read()).hexdigest() for ext in (".candidates.pam", ".circ_report")]
                if not pre:
                    res["srt_files_identical"] = [open(f"{out}_{rounds}_remain_R{m}.fastq.srt", "rb").read() for m in (1, 2)] == srt_kept
            res["stage2"] = circ
            save()
    os.environ.pop("CM_CIRC_PRESORTED", None)
    os.environ.pop("CM_CIRC_TRACE", None)
    res["stage2_outputs_identical"] = outs[0] == outs[1]
    save()
    assert res["stage2_outputs_identical"] and res["srt_files_identical"]
finally:
    shutil.rmtree(base, ignore_errors=True)
print("written:", out_path)
