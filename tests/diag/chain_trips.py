"""The dependent round trips of a heavy chaining problem, counted: chain_phases.py's wave time per phase plus the words the
-DCM_CHAIN_DIAG build adds for the back-tracking's log paths and the DP's scores asked for ahead (cm_debug_counters [25..28]).
python tests/diag/chain_trips.py [pairs]      env CM_LIB: a diagnostic build of another tree (default: this tree's, built here)"""
import ctypes as C, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
if not os.environ.get("CM_LIB"):
    from circminer_amd import _build
    os.environ["CM_LIB"] = _build.build(tag="cdiag", flags=["-DCM_CHAIN_DIAG"])
from circminer_amd import lib as cl, synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
d = synth.generate("hg38like", n_pairs=n, seed=38)
with tempfile.TemporaryDirectory() as td:
    gtf = os.path.join(td, "ref.gtf"); open(gtf, "w").write(d.gtf_text)
    hi = cl.HostIndex(d.contigs, d.chr_table, gtf, kmer=20, n_threads=min(16, os.cpu_count() or 8))
hp = cl.HotPath(cl.default_params())
for ci in range(hi.n_contigs):
    hp.load_contig(ci, hi.views[ci], hi.annots[ci])
hp.upload(cl.ReadBatch(d.seq1, d.seq2))
slots = list(range(hi.n_contigs))
hp.map_rounds(slots, True); hp.sync(); hp.reset()
hp.prof(True); hp.prof_reset()
hp.map_rounds(slots, True); hp.sync()
ms, nl, _ = hp.prof_get()
raw = (C.c_ulonglong * 32)()
hp.L.cm_debug_counters(hp.h, raw)
t = [raw[k] / 1e5 for k in (13, 14, 15)]          # ms of wave time
np_ = max(raw[22], 1)
print(os.path.basename(os.environ["CM_LIB"]), f"k_chain_heavy {ms[6]:.2f} ms in {nl[6]} launches")
print(f"wave-ms: load + pre-pass {t[0]:.0f}, DP {t[1]:.0f}, back-tracking {t[2]:.0f} (sum {sum(t):.0f})")
print(f"per problem with a log ({raw[22]}): {raw[24] / np_:.0f} cells, {raw[20] / np_:.0f} events, {raw[21] / np_:.2f} score levels, "
      f"{raw[23] / np_:.2f} 64-event passes over the log, {raw[26] / np_:.2f} candidate batches; log in registers: {raw[25]} problems")
print(f"DP: {raw[11]} cells, {raw[12]} pair evaluations; scores asked for ahead of the window loop: {raw[27]} used, {raw[28]} unused")
hp.close()
