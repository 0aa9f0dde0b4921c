"""The device-side remain formatter against the text-slicing writer of the device tokeniser's path on the bench's workload, in ONE
process on ONE box (numbers of different boxes do not compare, see ab_multi.py).  Not run by the suite.  The sibling of
rows_device_rate.py (--format pam | sam), for the third format; a script of its own because it compares other legs.
  (a) per batch, alternating: cm_collect_records + cm_write_remain_text (the records of the active set go to the host, the writer
      slices the text blocks) against cm_format_remain (into two page-locked buffers) + cm_write_bytes / cm_write_bytes2, into
      TMPFS; the kernels' own time by HIP events (ms[7] of cm_prof_get under cm_prof_enable).  No contig is loaded for this leg:
      the batches are staged from the FASTQ text and given states of the usual mix through cm_state_poke (90 % concordant pairs
      with positions below 2.5e8 and opposite strands, 10 % unmapped), so EVERY pair of a batch is active -- the set a real run
      re-queues is a few per cent of that: this leg is the formatter's worst case;
  (b) cm_mapping_run (report 0) from the FASTQ files to the remain files with CM_FASTQ_DEVICE=1, without and with
      CM_REMAIN_DEVICE=1, alternating, REPS times each, with the three legs of cm_mapping_stats; the files of both must be the
      same bytes.
The contigs come from the packed FASTA (tables built on the device: no index file to write); that time is seconds_load, outside
the rates.  Writes OUT after every leg.
env: WORKLOAD (hg38like), PAIRS (4194304), BATCH (1048576), REPS (2), THREADS (16), TMPFS (/dev/shm),
OUT (profiles/remain_device.json), COMMIT (the commit to record where the tree has no git metadata)"""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np
import bench
from circminer_amd import lib as cl, synth

wl = os.environ.get("WORKLOAD", "hg38like")
n_pairs = int(os.environ.get("PAIRS", 1 << 22))
batch = int(os.environ.get("BATCH", 1 << 20))
reps = int(os.environ.get("REPS", "2"))
threads = int(os.environ.get("THREADS", "16"))
tmpfs = os.environ.get("TMPFS", "/dev/shm")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "remain_device.json"))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
res = {"workload": wl, "pairs": n_pairs, "batch_pairs": batch, "threads": threads, "date": time.strftime("%Y-%m-%d")}
try:
    res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or os.environ.get("COMMIT")
except OSError:
    res["commit"] = os.environ.get("COMMIT")


def save():
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


t = time.perf_counter()
d = synth.generate(wl, n_pairs=min(n_pairs, 1 << 21), seed=38)
print(f"{wl}: generated in {time.perf_counter() - t:.1f} s", flush=True)
base = os.path.join(tmpfs, f"cm_remaindev_{os.getpid()}")
shutil.rmtree(base, ignore_errors=True)
os.makedirs(base)
try:
    names = [l.split(":", 1)[1].strip() for l in subprocess.run(["rocminfo"], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l]
    res["device"] = ([x for x in names if "Instinct" in x or "MI3" in x] or [None])[0]
except OSError:
    pass
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

    # (a) the records of every batch, both ways
    P = cl.default_params()
    hp = cl.HotPath(P)
    hp.prof(True)
    rng = np.random.default_rng(1)
    rd_text = cl.FastqReader(fq[0], fq[1], n_threads=threads)
    want = int(res["fastq_bytes"] / n_pairs / 2 * batch * 1.02) + (1 << 16)
    rows_pin = None
    legs = {"sliced": {"collect_records_s": 0.0, "write_remain_text_s": 0.0}, "device": {"format_s": 0.0, "write_bytes_s": 0.0, "kernels_s": 0.0, "row_bytes": 0},
            "active_set": "every pair of the batch (no contig loaded)"}
    sha = {"sliced": hashlib.sha1(), "device": hashlib.sha1()}
    call, table = hp.L.cm_format_remain, cl.chr_array(chrs)
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
        st["ed_r1"], st["ed_r2"] = rng.integers(0, 5, m), rng.integers(0, 5, m)
        st["tlen"] = rng.integers(150, 600, m)
        st["chr_id"] = rng.integers(0, max(len(chrs), 1), m)
        st["r1_forward"] = rng.integers(0, 2, m)
        st["r2_forward"] = 1 - st["r1_forward"]
        st["gm_compatible"] = 1
        st["type"] = np.where(rng.random(m) < 0.9, 0, 13)
        hp.poke_states(st)
        for leg in (("sliced", "device") if k % 2 == 0 else ("device", "sliced")):
            path = os.path.join(base, f"remain_{leg}_R1.fastq")
            w = cl.RecordWriter(path, path + "2", chrs)
            if leg == "sliced":
                t0 = time.perf_counter()
                recs = hp.collect_records()
                t1 = time.perf_counter()
                w.write_remain_text(b1, rec1, b2, rec2, recs)
                w.close()
                legs[leg]["collect_records_s"] += t1 - t0
                legs[leg]["write_remain_text_s"] += time.perf_counter() - t1
            else:
                hp.prof_reset()
                nb = (C.c_uint64 * 2)()
                if rows_pin is None:                                  # sized once, outside the timing, by the first batch's records
                    call(hp.h, table, len(chrs), 0, hp.n, None, 0, None, 0, nb, None, None, None)
                    rows_pin = [hp.host_array(int(x / hp.n * batch * 1.1) + (1 << 20), np.uint8) for x in nb]
                t0 = time.perf_counter()
                rc = call(hp.h, table, len(chrs), 0, hp.n, rows_pin[0].ctypes.data, rows_pin[0].size, rows_pin[1].ctypes.data, rows_pin[1].size, nb, None, None, None)
                assert rc == 0, rc
                t1 = time.perf_counter()
                w.write_bytes(rows_pin[0][:nb[0]])
                w.write_bytes2(rows_pin[1][:nb[1]])
                w.close()
                legs[leg]["format_s"] += t1 - t0
                legs[leg]["write_bytes_s"] += time.perf_counter() - t1
                legs[leg]["kernels_s"] += hp.prof_get()[0][7] / 1e3
                legs[leg]["row_bytes"] += int(nb[0]) + int(nb[1])
            for p in (path, path + "2"):
                sha[leg].update(open(p, "rb").read())
        got += m
        k += 1
    rd_text.close()
    hp.close()
    assert got == n_pairs
    for leg in ("sliced", "device"):
        legs[leg]["pairs_per_s"] = got / sum(x for key, x in legs[leg].items() if key.endswith("_s") and key != "kernels_s")
    legs["rows_identical"] = sha["sliced"].hexdigest() == sha["device"].hexdigest()
    legs["device"]["kernels_ms_per_2_20_pairs"] = legs["device"]["kernels_s"] * 1e3 / got * (1 << 20)
    legs["pcie_bytes_per_active_pair"] = {"sliced_out_record": 80, "device_out_records": legs["device"]["row_bytes"] / got}
    res["rows_per_batch"] = legs
    print(json.dumps(legs), flush=True)
    save()
    assert legs["rows_identical"]

    # (b) files to files, alternating: the device tokeniser's path without and with the variable
    os.environ["CM_FASTQ_DEVICE"] = "1"
    runs, files = [], {}
    for rep in range(reps):
        for dev in (0, 1):
            if dev:
                os.environ["CM_REMAIN_DEVICE"] = "1"
            else:
                os.environ.pop("CM_REMAIN_DEVICE", None)
            out = os.path.join(base, f"run{dev}")
            st = cl.run_mapping(packed, gtf, fq[0], fq[1], out, cl.default_params(kmer=20), report=0, n_threads=threads, batch_pairs=batch,
                                index_info=packed + ".index.info")
            row = {"rep": rep, "device_records": dev, "pairs": int(st.pairs), "bsj_pairs": int(st.bsj_pairs), "device_parsed_batches": int(st.device_parsed_batches),
                   "load_s": st.seconds_load, "map_s": st.seconds_map, "pairs_per_s": st.pairs / st.seconds_map,
                   "parts_s": {"read": st.seconds_parse, "device": st.seconds_device, "write": st.seconds_write}}
            assert st.pairs == n_pairs and st.device_parsed_batches
            runs.append(row)
            print(json.dumps(row), flush=True)
            if rep == 0:
                files[dev] = [hashlib.sha1(open(p, "rb").read()).hexdigest() for p in (f"{out}_{st.rounds}_remain_R1.fastq", f"{out}_{st.rounds}_remain_R2.fastq")]
            res["file_to_file"] = runs
            save()
    for var in ("CM_FASTQ_DEVICE", "CM_REMAIN_DEVICE"):
        os.environ.pop(var, None)
    res["files_identical"] = files[0] == files[1]
    for dev, key in ((0, "sliced"), (1, "device")):
        res[f"file_to_file_{key}_pairs_per_s"] = [r["pairs_per_s"] for r in runs if r["device_records"] == dev]
    save()
    assert res["files_identical"]
finally:
    shutil.rmtree(base, ignore_errors=True)
print("written:", out_path)
