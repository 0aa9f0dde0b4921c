"""The device-side FASTQ tokeniser against the host tokeniser on the bench's workload, in ONE process on ONE box (numbers of
different boxes do not compare, see ab_multi.py).  Not run by the suite.
  (1) host tokeniser alone: cm_fastq_next over both files, pairs/s;
  (2) cm_reads_stage_text alone: blocks from cm_fastq_next_text, wall time from pageable blocks and from page-locked copies of
      them (copy over PCIe included), and the kernels' own time by HIP events (cm_text_batch.reserved under cm_prof_enable);
  (3) cm_mapping_run (report 0) from the FASTQ files to the remain files with and without CM_FASTQ_DEVICE=1, alternating, REPS
      times each; the remain files of both must be the same bytes.  REPS=0 ends the script behind leg (2).
The contigs come from the packed FASTA (tables built on the device: no index file to write); that time is seconds_load, outside
the rates.  Writes OUT after every leg.
env: WORKLOAD (hg38like), PAIRS (8388608), BATCH (1048576), REPS (2), THREADS (16), TMPFS (/dev/shm), OUT (profiles/fastq_device.json)"""
import json
import os
import shutil
import sys
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
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "fastq_device.json"))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
res = {"workload": wl, "pairs": n_pairs, "batch_pairs": batch, "threads": threads, "date": time.strftime("%Y-%m-%d")}


def save():
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


t = time.perf_counter()
d = synth.generate(wl, n_pairs=min(n_pairs, 1 << 21), seed=38)
print(f"{wl}: generated in {time.perf_counter() - t:.1f} s", flush=True)
base = os.path.join(tmpfs, f"cm_fqdev_{os.getpid()}")
shutil.rmtree(base, ignore_errors=True)
os.makedirs(base)
try:
    import torch
    res["device"] = torch.cuda.get_device_name(0)
except Exception:
    pass
try:
    t = time.perf_counter()
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
    res["bytes_per_pair"] = res["fastq_bytes"] / n_pairs
    print(f"files written in {time.perf_counter() - t:.1f} s: {res['fastq_bytes'] / 1e9:.2f} GB of FASTQ text", flush=True)

    # (1) the host tokeniser alone (twice: the first pass also faults its buffers in)
    for name in ("host_tokeniser_first_pass", "host_tokeniser"):
        rd = cl.FastqReader(fq[0], fq[1], n_threads=threads)
        t0, got = time.perf_counter(), 0
        while True:
            b = rd.next_batch(batch)
            if b is None:
                break
            got += b.n
        dt = time.perf_counter() - t0
        rd.close()
        assert got == n_pairs
        res[name] = {"seconds": dt, "pairs_per_s": got / dt}
        print(name, json.dumps(res[name]), flush=True)
        save()

    # (2) cm_reads_stage_text alone
    hp = cl.HotPath(cl.default_params())
    hp.prof(True)
    want = int(res["bytes_per_pair"] / 2 * batch * 1.02) + (1 << 16)
    pin = [hp.host_array(want + (1 << 20), np.uint8) for _ in range(2)]
    for name in ("stage_text_pageable", "stage_text_pinned"):
        rd = cl.FastqReader(fq[0], fq[1], n_threads=threads)
        got, wall, dev_us, read_s, blocks = 0, 0.0, 0, 0.0, 0
        while True:
            t0 = time.perf_counter()
            b1, e1, b2, e2 = rd.next_text(want)
            read_s += time.perf_counter() - t0
            if len(b1) == 0 and e1:
                break
            if name.endswith("pinned"):
                pin[0][:len(b1)] = b1
                pin[1][:len(b2)] = b2
                b1, b2 = pin[0][:len(b1)], pin[1][:len(b2)]
            t0 = time.perf_counter()
            tb, _, _ = hp.stage_text(b1, b2, batch, eof1=e1, eof2=e2)
            wall += time.perf_counter() - t0
            assert tb.n_pairs > 0
            dev_us += tb.reserved
            got += tb.n_pairs
            blocks += 1
            rd.consumed(tb.used1, tb.used2)
        rd.close()
        assert got == n_pairs, (got, n_pairs)
        res[name] = {"blocks": blocks, "read_seconds": read_s, "stage_wall_seconds": wall, "kernels_seconds": dev_us / 1e6,
                     "pairs_per_s_wall": got / wall, "pairs_per_s_kernels": got / max(dev_us / 1e6, 1e-9),
                     "text_GBps_wall": res["fastq_bytes"] / wall / 1e9}
        print(name, json.dumps(res[name]), flush=True)
        save()
    hp.close()

    # (3) files to files, alternating
    runs = []
    files = {}
    for rep in range(reps):
        for dev in (0, 1):
            if dev:
                os.environ["CM_FASTQ_DEVICE"] = "1"
            else:
                os.environ.pop("CM_FASTQ_DEVICE", None)
            out = os.path.join(base, f"run{dev}")
            st = cl.run_mapping(packed, gtf, fq[0], fq[1], out, cl.default_params(kmer=20), report=0, n_threads=threads, batch_pairs=batch,
                                index_info=packed + ".index.info")
            row = {"rep": rep, "device_tokeniser": dev, "pairs": int(st.pairs), "bsj_pairs": int(st.bsj_pairs), "device_parsed_batches": int(st.device_parsed_batches),
                   "load_s": st.seconds_load, "map_s": st.seconds_map, "pairs_per_s": st.pairs / st.seconds_map,
                   "parts_s": {"parse_or_read": st.seconds_parse, "device": st.seconds_device, "write": st.seconds_write}}
            assert st.pairs == n_pairs and bool(st.device_parsed_batches) == bool(dev)
            runs.append(row)
            print(json.dumps(row), flush=True)
            if rep == 0:
                import hashlib
                files[dev] = [hashlib.sha1(open(f"{out}_{st.rounds}_remain_R{m}.fastq", "rb").read()).hexdigest() for m in (1, 2)]
            res["file_to_file"] = runs
            save()
    os.environ.pop("CM_FASTQ_DEVICE", None)
    if runs:                                 # (REPS=0: legs (1) and (2) only)
        res["remain_files_identical"] = files[0] == files[1]
        for dev, key in ((0, "host"), (1, "device")):
            v = [r["pairs_per_s"] for r in runs if r["device_tokeniser"] == dev]
            res[f"file_to_file_{key}_best_pairs_per_s"] = max(v)
        res["device_path_wins"] = res["file_to_file_device_best_pairs_per_s"] > res["file_to_file_host_best_pairs_per_s"]
        save()
        assert res["remain_files_identical"]
finally:
    shutil.rmtree(base, ignore_errors=True)
print("written:", out_path)
