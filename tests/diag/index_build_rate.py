"""Three ways to make a packed contig resident, timed per contig in ONE process on ONE box (numbers of different boxes do not
compare, see ab_multi.py):
  (a) cm_host_build_index on THREADS host threads, then cm_load_contig;
  (b) the index file (written to tmpfs beforehand) through cm_host_next_contig_raw + cm_load_contig_raw;
  (c) cm_build_contig from the sequence: the table is built on the device.
Prints stats.ms_device and the temporary HBM of (c), checks that (c) left the arrays of (a) (the downloaded arrays are
compared), and writes everything to OUT as JSON after every contig.
env: WORKLOAD (hg38like), THREADS (16), KMER (20), TMPFS (/dev/shm), OUT (profiles/index_build.json), SKIP_FILE (0: run (b))"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np
from circminer_amd import lib as cl, synth

wl = os.environ.get("WORKLOAD", "hg38like")
threads = int(os.environ.get("THREADS", "16"))
kmer = int(os.environ.get("KMER", "20"))
tmpfs = os.environ.get("TMPFS", "/dev/shm")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "index_build.json"))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
res = {"workload": wl, "kmer": kmer, "threads": threads, "date": time.strftime("%Y-%m-%d"), "contigs": []}


def save():
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


t = time.perf_counter()
d = synth.generate(wl, n_pairs=64, seed=38)
print(f"{wl}: {len(d.contigs)} contigs of {[len(c) for c in d.contigs]} bp generated in {time.perf_counter() - t:.1f} s", flush=True)
L = cl.load()
hp = cl.HotPath(cl.default_params(kmer=kmer))
try:
    import torch
    res["device"] = torch.cuda.get_device_name(0)
except Exception:
    pass

for ci, g in enumerate(d.contigs):
    row = {"contig": ci, "bp": int(len(g))}
    # (a)
    iv = cl.IndexView()
    t0 = time.perf_counter()
    rc = L.cm_host_build_index(cl.ptr(g, cl.u8p), len(g), kmer, ci, threads, C.byref(iv))
    assert rc == 0, rc
    t1 = time.perf_counter()
    hp.load_contig(0, iv)
    t2 = time.perf_counter()
    row["a_host_build_s"], row["a_load_s"], row["a_total_s"] = t1 - t0, t2 - t1, t2 - t0
    arrays_a = hp.index_arrays(0)
    L.cm_host_free_index(C.byref(iv))
    # (c)
    t0 = time.perf_counter()
    st = hp.build_contig(0, ci, g)
    t1 = time.perf_counter()
    row["c_total_s"], row["c_ms_device"], row["c_tmp_mib"] = t1 - t0, st.ms_device, int(st.reserved)
    row["entries"], row["max_bucket"], row["buckets_by_path"] = int(st.n_entries), int(st.max_bucket), [int(x) for x in st.buckets_by_path]
    row["c_equals_a"] = bool(all(np.array_equal(x, y) for x, y in zip(arrays_a, hp.index_arrays(0))))
    del arrays_a
    print(json.dumps(row), flush=True)
    res["contigs"].append(row)
    save()
hp.sync()

if os.environ.get("SKIP_FILE", "0") != "1":
    # (b): the packed FASTA and its index file on tmpfs
    packed = os.path.join(tmpfs, f"cm_ibr_{os.getpid()}.packed.fa")
    idx = packed + ".index"
    try:
        t0 = time.perf_counter()
        with open(packed, "wb") as f:
            for ci, g in enumerate(d.contigs):
                f.write(b">%d\n" % (ci + 1))
                f.write(g.data)
                f.write(b"\n")
        t1 = time.perf_counter()
        cl.write_index(packed, kmer=kmer, n_threads=threads)
        t2 = time.perf_counter()
        res["file"] = {"packed_fa_write_s": t1 - t0, "write_index_s": t2 - t1, "index_bytes": os.path.getsize(idx)}
        print(json.dumps(res["file"]), flush=True)
        f = cl.IndexFile(idx, n_threads=threads, raw=True)
        ci = 0
        while True:
            t0 = time.perf_counter()
            try:
                raw = next(f)
            except StopIteration:
                break
            t1 = time.perf_counter()
            hp.load_contig_raw(0, raw)
            t2 = time.perf_counter()
            row = res["contigs"][ci]
            row["b_read_s"], row["b_load_raw_s"], row["b_total_s"] = t1 - t0, t2 - t1, t2 - t0
            print(json.dumps({k: v for k, v in row.items() if k.startswith("b_") or k == "contig"}), flush=True)
            save()
            ci += 1
        f.close()
    except Exception as e:                          # e.g. tmpfs too small for the index file: (a) and (c) stand
        res["file_error"] = repr(e)
        print("(b) not measured:", e, flush=True)
    finally:
        for p in (packed, idx):
            if os.path.exists(p):
                os.remove(p)
for row in res["contigs"]:
    row["c_lt_a"] = row["c_total_s"] < row["a_total_s"]
    if "b_total_s" in row:
        row["c_le_b"] = row["c_total_s"] <= row["b_total_s"]
save()
hp.close()
print("written:", out_path)
