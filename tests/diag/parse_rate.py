"""FASTQ ingest rate of cm_fastq_next (no GPU involved): record-by-record parser vs the chunk-parallel plain-text path, then
cm_fastq_next_text (64-MB blocks, everything consumed).  CM_LIB names another build of the library; KEEP_DIR=<dir> writes the
input there once and leaves it for the next run (an A/B of two libraries reads the same files).  The last line is the rates as JSON."""
import json, os, sys, time, tempfile, shutil, ctypes as C
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from circminer_amd import lib as cl
n = int(os.environ.get("PAIRS", "3000000"))
batch = int(os.environ.get("BATCH", str(1 << 18)))
keep = os.environ.get("KEEP_DIR")
td = keep or tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
if not (keep and os.path.exists(f"{td}/r_2.fq.done")):
    os.makedirs(td, exist_ok=True)
    rng = np.random.default_rng(1)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, 150), dtype=np.int8)]
    q = b"I" * 150
    for mate in (1, 2):
        with open(f"{td}/r_{mate}.fq", "wb") as f:
            for i in range(n):
                f.write(b"@read%d/%d\n" % (i, mate)); f.write(seq[i].tobytes()); f.write(b"\n+\n"); f.write(q); f.write(b"\n")
        open(f"{td}/r_{mate}.fq.done", "w").close()
    print("files written", flush=True)
rates = {}
for env in ({"CM_FASTQ_SERIAL": "1"}, {"CM_FASTQ_THREADS": "4"}, {"CM_FASTQ_THREADS": "8"}, {"CM_FASTQ_THREADS": "16"}, {"CM_FASTQ_THREADS": "32"}):
    for k in ("CM_FASTQ_SERIAL", "CM_FASTQ_THREADS"):
        os.environ.pop(k, None)
    os.environ.update(env)
    rd = cl.FastqReader(f"{td}/r_1.fq", f"{td}/r_2.fq", [], 4)
    tot = k = 0
    t = None
    while True:
        fb = cl.FastqBatch()
        rd.L.cm_fastq_next(rd.h, batch, C.byref(fb))
        if fb.reads.n_pairs == 0:
            break
        k += 1
        if k == 4:                      # steady state: the three storage generations have been touched
            t = time.time(); tot = 0
            continue
        tot += fb.reads.n_pairs
    rates[" ".join(f"{a}={b}" for a, b in env.items())] = tot / (time.time() - t) / 1e6
    print(env, "steady state %.2f M pairs/s" % (tot / (time.time() - t) / 1e6), flush=True)
    rd.close()
# text-block mode: the blocks as they are, everything consumed; pairs = R1's share of the file, in pairs
for k in ("CM_FASTQ_SERIAL", "CM_FASTQ_THREADS"):
    os.environ.pop(k, None)
rd = cl.FastqReader(f"{td}/r_1.fq", f"{td}/r_2.fq", [], 4)
size1 = os.path.getsize(f"{td}/r_1.fq")
tot = k = 0
t = None
while True:
    t1, e1, t2, e2 = rd.next_text(64 << 20)
    if len(t1) == 0 and len(t2) == 0:
        break
    rd.consumed(len(t1), len(t2))
    k += 1
    if k == 4:
        t = time.time(); tot = 0
        continue
    tot += len(t1)
rates["text blocks"] = tot / size1 * n / (time.time() - t) / 1e6
print("text blocks of 64 MB: steady state %.2f M pairs/s" % rates["text blocks"], flush=True)
rd.close()
if not keep:
    shutil.rmtree(td)
print(json.dumps(rates))
