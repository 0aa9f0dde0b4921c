"""The device's count of the chaining problems the round pipeline leaves unchained (NOTES 67) on the bench's step: word 7 of
cm_debug_counters next to the pair-rounds (word 3), to set against the CPU count of tests/diag/dead_chains.py.
usage: dead_chains_device.py      env: PAIRS (2^21), STEPS (2), WORKLOAD (hg38like), CM_LIB (default: this tree's library)"""
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
from circminer_amd import lib as cl, synth  # noqa: E402

pairs = int(os.environ.get("PAIRS", 1 << 21))
steps = int(os.environ.get("STEPS", "2"))
wl = os.environ.get("WORKLOAD", "hg38like")
d = synth.generate(wl, n_pairs=2 * pairs, seed=38)
with tempfile.TemporaryDirectory() as td:
    gtf = os.path.join(td, "a.gtf")
    with open(gtf, "w") as f:
        f.write(d.gtf_text)
    hi = cl.HostIndex(d.contigs, d.chr_table, gtf, kmer=20, n_threads=min(16, os.cpu_count() or 8))
hp = cl.HotPath(cl.default_params())
for ci in range(hi.n_contigs):
    hp.load_contig(ci, hi.views[ci], hi.annots[ci])
batches = [hp.pinned_batch(d.seq1[i * pairs:(i + 1) * pairs], d.seq2[i * pairs:(i + 1) * pairs]) for i in range(2)]
hp.stage(batches[0])
hp.swap()
hp.prof_reset()
for s in range(steps):
    if s + 1 < steps:                   # (nothing staged behind the last step: no item of a further batch is prefetched and counted)
        hp.stage(batches[(s + 1) & 1])
    hp.map_rounds(list(range(hi.n_contigs)), True)
    if s + 1 < steps:
        hp.swap()
hp.sync()
raw = (C.c_ulonglong * 32)()
hp._chk(hp.L.cm_debug_counters(hp.h, raw), "cm_debug_counters")
print(f"{wl}, {steps} steps of {pairs} pairs x {hi.n_contigs} rounds: {raw[7]} problems with hits left unchained, {raw[3]} pair-rounds, "
      f"{raw[7] / max(raw[3], 1):.4f} per pair-round")
hp.close()
