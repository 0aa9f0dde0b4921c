"""Builds circminer_amd/csrc/libcmhot.so (gfx950 HIP kernels + C-ABI + host-side builders) in-tree.

hipcc cross-compiles for gfx950 without a GPU; the .so travels to the GPU box with the repo
snapshot.  `-ffp-contract=off` is required for parity: chain scores are fp64 sums whose rounding
order is part of the result (reference src/chain.cpp:189).
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INC = os.path.join(HERE, "..", "include")
OUT = os.path.join(CSRC, "libcmhot.so")
SOURCES = ["cm_hot.hip", "cm_dp_probe.hip", "cm_annot_probe.hip", "cm_circ_chain.hip", "cm_dispatch.cpp", "host_index.cpp", "host_annot.cpp", "host_index_io.cpp", "host_fastq.cpp", "host_mapping.cpp", "host_circ.cpp",
           "host_circ_call.cpp", "host_detect.cpp"]
ABI_DEF = "cm_device_abi.def"
DEPS = SOURCES + sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [ABI_DEF, os.path.join("..", "..", "include", "circminer_hot.h")]
# cm_hot.hip is compiled twice (reads of <= 16 seeds / <= 24 seeds, see cm_dispatch.cpp): the names it exports get a suffix.  The
# entry points are the lines of the table; the context struct, the chain record and the kernel bodies' namespace are no entry points
# but differ in size between the builds, so they are renamed with them.
RENAMED_TYPES = ["cm_ctx", "cm_chain", "cmc"]
_ABI_LINE = re.compile(r"(CM_DEV|CM_DEV_OWN)\((.+?), (cm_\w+), \(([^()]*)\)(?:, \(([^()]*)\))?\)")


def device_abi(path: str = os.path.join(CSRC, ABI_DEF)):
    """The lines of the table as (macro, return type, name, parameters, arguments or None)."""
    rows = []
    for line in open(path):
        if line.startswith("CM_DEV"):
            m = _ABI_LINE.fullmatch(line.rstrip())
            if not m or (m.group(1) == "CM_DEV") != (m.group(5) is not None):
                raise RuntimeError(f"{ABI_DEF}: cannot read {line.rstrip()!r}")
            rows.append(m.groups())
    return rows


VARIANTS = (("k16", []), ("k24", ["-DCM_MAX_CHAIN_FRAGS=24"]))
HIP_ONCE = ["cm_dp_probe.hip", "cm_annot_probe.hip", "cm_circ_chain.hip"]      # device code that does not depend on CM_MAX_CHAIN_FRAGS: one build, its own names (the test hooks behind cm_dp_batch / cm_annot_batch, stage 2's seeds and chains behind cm_circ_chain_batch)


def needs_build(out: str = OUT) -> bool:
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS)


def build(force: bool = False, verbose: bool = False, tag: str = "", flags=()) -> str:
    """tag / flags: a second library libcmhot_<tag>.so compiled with extra -D flags (test builds, e.g. a 2-entry extension
    memo that sends many pairs through the re-run launch); the product library has neither."""
    OUT = os.path.join(CSRC, f"libcmhot_{tag}.so") if tag else globals()["OUT"]
    if not force and not needs_build(OUT):
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("CM_EXTRA_FLAGS", "").split() + list(flags)
    sfx = ("_" + tag) if tag else ""
    renamed = [row[2] for row in device_abi()] + RENAMED_TYPES
    objs = []
    jobs = []
    for s in SOURCES:
        base = [hipcc, "-c", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", *extra, "-I", INC, "-I", CSRC]
        if s.endswith(".hip"):
            arch = ["--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage"] if verbose else ["--offload-arch=gfx950"]
            if s in HIP_ONCE:
                o = os.path.join(CSRC, s.rsplit(".", 1)[0] + sfx + ".o")
                jobs.append((s, [base[0]] + arch + base[1:] + [os.path.join(CSRC, s), "-o", o]))
                objs.append(o)
                continue
            for vtag, vflags in VARIANTS:
                o = os.path.join(CSRC, s.rsplit(".", 1)[0] + "_" + vtag + sfx + ".o")
                ren = [f"-D{n}={n}_{vtag}" for n in renamed]
                jobs.append((s + " [" + vtag + "]", [base[0]] + arch + base[1:] + vflags + ren + [os.path.join(CSRC, s), "-o", o]))
                objs.append(o)
        else:
            o = os.path.join(CSRC, s.rsplit(".", 1)[0] + sfx + ".o")
            jobs.append((s, [base[0], "-x", "c++"] + base[1:] + [os.path.join(CSRC, s), "-o", o]))   # host-only sources: plain C++
            objs.append(o)
    if verbose:
        sys.stderr.write("".join(" ".join(cmd) + "\n" for _, cmd in jobs))
    procs = [(name, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for name, cmd in jobs]   # in parallel
    failed = []
    for name, pr in procs:
        out, _ = pr.communicate()
        if verbose or pr.returncode != 0:
            sys.stderr.write(out)
        if pr.returncode != 0:
            failed.append(name)
    if failed:
        raise RuntimeError(f"hipcc failed on {failed}")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs + ["-lpthread", "-lz"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("link failed")
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
