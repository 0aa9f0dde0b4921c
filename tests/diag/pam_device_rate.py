"""The device-side PAM formatter against the host writer on the bench's workload, in ONE process on ONE box (numbers of different
boxes do not compare, see ab_multi.py).  Not run by the suite.
  (a) per batch, alternating: cm_reads_download + cm_write_pam into TMPFS against cm_format_pam + cm_write_bytes; the kernels'
      own time by HIP events (ms[7] of cm_prof_get under cm_prof_enable) next to the time the row bytes take over PCIe.  No
      contig is loaded for this leg: the batches are staged from the FASTQ text and given states of the usual mix through
      cm_state_poke (90 % concordant rows with positions below 2.5e8, 10 % unmapped), so only the writers are timed;
  (b) cm_mapping_run (report 1) from the FASTQ files to .mapping.pam and the remain files, host path against CM_FASTQ_DEVICE=1
      CM_PAM_DEVICE=1, alternating, REPS times each; the files of both must be the same bytes.
The contigs come from the packed FASTA (tables built on the device: no index file to write); that time is seconds_load, outside
the rates.  Writes OUT after every leg.
env: WORKLOAD (hg38like), PAIRS (4194304), BATCH (1048576), REPS (2), THREADS (16), TMPFS (/dev/shm), OUT (profiles/pam_device.json)"""
import hashlib
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
n_pairs = int(os.environ.get("PAIRS", 1 << 22))
batch = int(os.environ.get("BATCH", 1 << 20))
reps = int(os.environ.get("REPS", "2"))
threads = int(os.environ.get("THREADS", "16"))
tmpfs = os.environ.get("TMPFS", "/dev/shm")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "pam_device.json"))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
res = {"workload": wl, "pairs": n_pairs, "batch_pairs": batch, "threads": threads, "date": time.strftime("%Y-%m-%d")}


def save():
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


t = time.perf_counter()
d = synth.generate(wl, n_pairs=min(n_pairs, 1 << 21), seed=38)
print(f"{wl}: generated in {time.perf_counter() - t:.1f} s", flush=True)
base = os.path.join(tmpfs, f"cm_pamdev_{os.getpid()}")
shutil.rmtree(base, ignore_errors=True)
os.makedirs(base)
try:
    import torch
    res["device"] = torch.cuda.get_device_name(0)
except Exception:
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

    # (a) the rows of every batch, both ways
    P = cl.default_params()
    hp = cl.HotPath(P)
    hp.prof(True)
    rng = np.random.default_rng(1)
    rd_text = cl.FastqReader(fq[0], fq[1], n_threads=threads)
    rd_host = cl.FastqReader(fq[0], fq[1], chrs, P.max_ed, n_threads=threads)
    want = int(res["fastq_bytes"] / n_pairs / 2 * batch * 1.02) + (1 << 16)
    rows_pin = None
    legs = {"host": {"download_s": 0.0, "write_pam_s": 0.0}, "device": {"format_s": 0.0, "write_bytes_s": 0.0, "kernels_s": 0.0, "row_bytes": 0}}
    sha = {"host": hashlib.sha1(), "device": hashlib.sha1()}
    got = 0
    k = 0
    while True:
        b1, e1, b2, e2 = rd_text.next_text(want)
        if len(b1) == 0 and e1:
            break
        tb, _, _ = hp.stage_text(b1, b2, batch, eof1=e1, eof2=e2, keep_names=True)
        assert tb.n_pairs > 0
        rd_text.consumed(tb.used1, tb.used2)
        hb = rd_host.next_batch(int(tb.n_pairs))
        assert hb is not None and hb.n == tb.n_pairs
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
        for leg in (("host", "device") if k % 2 == 0 else ("device", "host")):
            path = os.path.join(base, f"rows_{leg}.pam")
            w = cl.RecordWriter(path, None, chrs)
            if leg == "host":
                t0 = time.perf_counter()
                st = hp.download()[0]
                t1 = time.perf_counter()
                w.write_pam(hb, st)
                w.close()
                legs[leg]["download_s"] += t1 - t0
                legs[leg]["write_pam_s"] += time.perf_counter() - t1
            else:
                hp.prof_reset()
                L, table = hp.L, cl.chr_array(chrs)
                import ctypes as C
                nb = C.c_uint64(0)
                if rows_pin is None:
                    L.cm_format_pam(hp.h, table, len(chrs), 0, hp.n, None, 0, C.byref(nb), None)
                    rows_pin = hp.host_array(int(nb.value * 1.2) + (1 << 20), np.uint8)
                t0 = time.perf_counter()
                rc = L.cm_format_pam(hp.h, table, len(chrs), 0, hp.n, rows_pin.ctypes.data, rows_pin.size, C.byref(nb), None)
                t1 = time.perf_counter()
                assert rc == 0, rc
                w.write_bytes(rows_pin[:nb.value])
                w.close()
                legs[leg]["format_s"] += t1 - t0
                legs[leg]["write_bytes_s"] += time.perf_counter() - t1
                legs[leg]["kernels_s"] += hp.prof_get()[0][7] / 1e3
                legs[leg]["row_bytes"] += int(nb.value)
            sha[leg].update(open(path, "rb").read())
        got += int(tb.n_pairs)
        k += 1
    rd_text.close()
    rd_host.close()
    hp.close()
    assert got == n_pairs
    for leg, v in legs.items():
        total = sum(x for key, x in v.items() if key in ("download_s", "write_pam_s", "format_s", "write_bytes_s"))
        v["pairs_per_s"] = got / total
    legs["rows_identical"] = sha["host"].hexdigest() == sha["device"].hexdigest()
    res["rows_per_batch"] = legs
    print(json.dumps(legs), flush=True)
    save()
    assert legs["rows_identical"]

    # (b) files to files, alternating
    runs, files = [], {}
    for rep in range(reps):
        for dev in (0, 1):
            for var in ("CM_FASTQ_DEVICE", "CM_PAM_DEVICE"):
                if dev:
                    os.environ[var] = "1"
                else:
                    os.environ.pop(var, None)
            out = os.path.join(base, f"run{dev}")
            st = cl.run_mapping(packed, gtf, fq[0], fq[1], out, cl.default_params(kmer=20), report=1, n_threads=threads, batch_pairs=batch,
                                index_info=packed + ".index.info")
            row = {"rep": rep, "device_rows": dev, "pairs": int(st.pairs), "bsj_pairs": int(st.bsj_pairs), "device_parsed_batches": int(st.device_parsed_batches),
                   "load_s": st.seconds_load, "map_s": st.seconds_map, "pairs_per_s": st.pairs / st.seconds_map,
                   "parts_s": {"parse_or_read": st.seconds_parse, "device": st.seconds_device, "write": st.seconds_write}}
            assert st.pairs == n_pairs and bool(st.device_parsed_batches) == bool(dev)
            runs.append(row)
            print(json.dumps(row), flush=True)
            if rep == 0:
                files[dev] = [hashlib.sha1(open(p, "rb").read()).hexdigest()
                              for p in (out + ".mapping.pam", f"{out}_{st.rounds}_remain_R1.fastq", f"{out}_{st.rounds}_remain_R2.fastq")]
            res["file_to_file"] = runs
            save()
    for var in ("CM_FASTQ_DEVICE", "CM_PAM_DEVICE"):
        os.environ.pop(var, None)
    res["files_identical"] = files[0] == files[1]
    for dev, key in ((0, "host"), (1, "device")):
        res[f"file_to_file_{key}_pairs_per_s"] = [r["pairs_per_s"] for r in runs if r["device_rows"] == dev]
    save()
    assert res["files_identical"]
finally:
    shutil.rmtree(base, ignore_errors=True)
print("written:", out_path)
