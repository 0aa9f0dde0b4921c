"""A device-side row formatter (--format pam | sam) against the host writer on the bench's workload, in ONE process on ONE box
(numbers of different boxes do not compare, see ab_multi.py).  Not run by the suite.
  (a) per batch, alternating: cm_reads_download + cm_write_pam / cm_write_sam into TMPFS against cm_format_pam / cm_format_sam (in
      ranges of RANGE pairs, into a page-locked buffer) + cm_write_bytes; the kernels' own time by HIP events (ms[7] of cm_prof_get
      under cm_prof_enable) next to the time the row bytes take over PCIe; for sam also the bytes per pair that go in (FASTQ text)
      and come out (records).  No contig is loaded for this leg: the batches are staged from the FASTQ text and given states of
      the usual mix through cm_state_poke (90 % concordant pairs with positions below 2.5e8 and opposite strands, 10 % unmapped),
      so only the writers are timed;
  (b) cm_mapping_run (report 1 / 2) from the FASTQ files to .mapping.pam / .mapping.sam and the remain files, host path against
      CM_FASTQ_DEVICE=1 CM_PAM_DEVICE=1 / CM_SAM_DEVICE=1, alternating, REPS times each, with the three legs of cm_mapping_stats;
      the files of both must be the same bytes.
The contigs come from the packed FASTA (tables built on the device: no index file to write); that time is seconds_load, outside
the rates.  Writes OUT after every leg.  The keys of OUT are those of the recorded profiles/pam_device.json / sam_device.json.
env: WORKLOAD (hg38like), PAIRS (4194304), BATCH (1048576), RANGE (pam: the batch; sam: 131072), REPS (2), THREADS (16),
TMPFS (/dev/shm), OUT (profiles/<format>_device.json), COMMIT (sam: the commit to record where the tree has no git metadata)"""
import argparse
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

# what the two formats differ in: the host writer, the C call, cm_mapping_run's report and variable, the bits to stage with, the
# default range, and whether OUT also says the range, the commit, the kernels' time per 2^20 pairs and the PCIe bytes per pair
FORMATS = {"pam": dict(write="write_pam", call="cm_format_pam", report=1, var="CM_PAM_DEVICE", quals=False, range=None, extras=False),
           "sam": dict(write="write_sam", call="cm_format_sam", report=2, var="CM_SAM_DEVICE", quals=True, range=1 << 17, extras=True)}
ap = argparse.ArgumentParser()
ap.add_argument("--format", choices=sorted(FORMATS), required=True)
fmt = ap.parse_args().format
F = FORMATS[fmt]

wl = os.environ.get("WORKLOAD", "hg38like")
n_pairs = int(os.environ.get("PAIRS", 1 << 22))
batch = int(os.environ.get("BATCH", 1 << 20))
reps = int(os.environ.get("REPS", "2"))
threads = int(os.environ.get("THREADS", "16"))
tmpfs = os.environ.get("TMPFS", "/dev/shm")
rng_pairs = int(os.environ.get("RANGE", F["range"] or batch))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", f"{fmt}_device.json"))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
res = {"workload": wl, "pairs": n_pairs, "batch_pairs": batch, "threads": threads, "date": time.strftime("%Y-%m-%d")}
if F["extras"]:
    res["range_pairs"] = rng_pairs
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or os.environ.get("COMMIT")
    except OSError:
        res["commit"] = None


def save():
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


t = time.perf_counter()
d = synth.generate(wl, n_pairs=min(n_pairs, 1 << 21), seed=38)
print(f"{wl}: generated in {time.perf_counter() - t:.1f} s", flush=True)
base = os.path.join(tmpfs, f"cm_{fmt}dev_{os.getpid()}")
shutil.rmtree(base, ignore_errors=True)
os.makedirs(base)
try:
    names = [l.split(":", 1)[1].strip() for l in subprocess.run(["rocminfo"], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l]
    names = [x for x in names if x]
    res["device"] = ([x for x in names if "Instinct" in x or "MI3" in x] or names[-1:] or [None])[0]
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

    # (a) the rows of every batch, both ways
    P = cl.default_params()
    hp = cl.HotPath(P)
    hp.prof(True)
    rng = np.random.default_rng(1)
    rd_text = cl.FastqReader(fq[0], fq[1], n_threads=threads)
    rd_host = cl.FastqReader(fq[0], fq[1], chrs, P.max_ed, n_threads=threads)
    want = int(res["fastq_bytes"] / n_pairs / 2 * batch * 1.02) + (1 << 16)
    rows_pin = None
    write_s = F["write"] + "_s"
    legs = {"host": {"download_s": 0.0, write_s: 0.0}, "device": {"format_s": 0.0, "write_bytes_s": 0.0, "kernels_s": 0.0, "row_bytes": 0}}
    sha = {"host": hashlib.sha1(), "device": hashlib.sha1()}
    call, table = getattr(hp.L, F["call"]), cl.chr_array(chrs)
    got = 0
    k = 0
    bases_total = 0
    while True:
        b1, e1, b2, e2 = rd_text.next_text(want)
        if len(b1) == 0 and e1:
            break
        tb, _, _ = hp.stage_text(b1, b2, batch, eof1=e1, eof2=e2, keep_names=True, keep_quals=F["quals"])
        assert tb.n_pairs > 0
        rd_text.consumed(tb.used1, tb.used2)
        hb = rd_host.next_batch(int(tb.n_pairs))
        assert hb is not None and hb.n == tb.n_pairs
        bases_total += int(hb.c.off1[hb.n]) + int(hb.c.off2[hb.n])
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
            path = os.path.join(base, f"rows_{leg}.{fmt}")
            w = cl.RecordWriter(path, None, chrs)
            if leg == "host":
                t0 = time.perf_counter()
                st = hp.download()[0]
                t1 = time.perf_counter()
                getattr(w, F["write"])(hb, st)
                w.close()
                legs[leg]["download_s"] += t1 - t0
                legs[leg][write_s] += time.perf_counter() - t1
            else:
                hp.prof_reset()
                nb = C.c_uint64(0)
                if rows_pin is None:                                  # sized once, outside the timing: a range's bytes scaled to the batch
                    call(hp.h, table, len(chrs), 0, min(hp.n, rng_pairs), None, 0, C.byref(nb), None)
                    rows_pin = hp.host_array(int(nb.value / min(hp.n, rng_pairs) * batch * 1.2) + (1 << 20), np.uint8)
                t0 = time.perf_counter()
                filled = 0
                for a in range(0, hp.n, rng_pairs):
                    rc = call(hp.h, table, len(chrs), a, min(rng_pairs, hp.n - a), rows_pin.ctypes.data + filled, rows_pin.size - filled, C.byref(nb), None)
                    assert rc == 0, rc
                    filled += int(nb.value)
                t1 = time.perf_counter()
                w.write_bytes(rows_pin[:filled])
                w.close()
                legs[leg]["format_s"] += t1 - t0
                legs[leg]["write_bytes_s"] += time.perf_counter() - t1
                legs[leg]["kernels_s"] += hp.prof_get()[0][7] / 1e3
                legs[leg]["row_bytes"] += filled
            sha[leg].update(open(path, "rb").read())
        got += int(tb.n_pairs)
        k += 1
    rd_text.close()
    rd_host.close()
    hp.close()
    assert got == n_pairs
    for leg, v in legs.items():
        total = sum(x for key, x in v.items() if key in ("download_s", write_s, "format_s", "write_bytes_s"))
        v["pairs_per_s"] = got / total
    legs["rows_identical"] = sha["host"].hexdigest() == sha["device"].hexdigest()
    if F["extras"]:
        legs["device"]["kernels_ms_per_2_20_pairs"] = legs["device"]["kernels_s"] * 1e3 / got * (1 << 20)
        legs["pcie_bytes_per_pair"] = {"host_in_bases_and_offsets": bases_total / got + 16, "host_out_states_and_flags": 72 + 1,
                                       "device_in_text": res["fastq_bytes"] / got, "device_out_records": legs["device"]["row_bytes"] / got}
    res["rows_per_batch"] = legs
    print(json.dumps(legs), flush=True)
    save()
    assert legs["rows_identical"]

    # (b) files to files, alternating
    runs, files = [], {}
    for rep in range(reps):
        for dev in (0, 1):
            for var in ("CM_FASTQ_DEVICE", F["var"]):
                if dev:
                    os.environ[var] = "1"
                else:
                    os.environ.pop(var, None)
            out = os.path.join(base, f"run{dev}")
            st = cl.run_mapping(packed, gtf, fq[0], fq[1], out, cl.default_params(kmer=20), report=F["report"], n_threads=threads, batch_pairs=batch,
                                index_info=packed + ".index.info")
            row = {"rep": rep, "device_rows": dev, "pairs": int(st.pairs), "bsj_pairs": int(st.bsj_pairs), "device_parsed_batches": int(st.device_parsed_batches),
                   "load_s": st.seconds_load, "map_s": st.seconds_map, "pairs_per_s": st.pairs / st.seconds_map,
                   "parts_s": {"parse_or_read": st.seconds_parse, "device": st.seconds_device, "write": st.seconds_write}}
            assert st.pairs == n_pairs and bool(st.device_parsed_batches) == bool(dev)
            runs.append(row)
            print(json.dumps(row), flush=True)
            if rep == 0:
                files[dev] = [hashlib.sha1(open(p, "rb").read()).hexdigest()
                              for p in (out + f".mapping.{fmt}", f"{out}_{st.rounds}_remain_R1.fastq", f"{out}_{st.rounds}_remain_R2.fastq")]
            res["file_to_file"] = runs
            save()
    for var in ("CM_FASTQ_DEVICE", F["var"]):
        os.environ.pop(var, None)
    res["files_identical"] = files[0] == files[1]
    for dev, key in ((0, "host"), (1, "device")):
        res[f"file_to_file_{key}_pairs_per_s"] = [r["pairs_per_s"] for r in runs if r["device_rows"] == dev]
    save()
    assert res["files_identical"]
finally:
    shutil.rmtree(base, ignore_errors=True)
print("written:", out_path)
