"""Build the HIP extension (libavexhip.so) in-tree for gfx950.

    python -m avex_amd.build [--force]

hipcc cross-compiles without a GPU.  Objects land in avex_amd/_build/, the shared library in
avex_amd/lib/libavexhip.so (git-ignored, but it travels to the GPU box with the snapshot).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# AVEX_AMD_DIAG=1: the diagnostic build (-DAVEX_DIAG: clock stamps in the GEMM, debug knobs in the attention kernel, the LDS canary
# and the avexhip_debug_* exports) goes to its own object directory and library; the product library contains none of it.
DIAG = os.environ.get("AVEX_AMD_DIAG", "") == "1"
# AVEX_AMD_LIB_SUFFIX=x: an A/B build (with AVEX_AMD_EXTRA_CFLAGS) into _build_x/ and lib/libavexhip_x.so, selected at run time with
# AVEX_AMD_LIB=.../libavexhip_x.so; the product library is the one without a suffix.
_SUFFIX = os.environ.get("AVEX_AMD_LIB_SUFFIX", "") or ("diag" if DIAG else "")
OBJ = os.path.join(HERE, "_build_" + _SUFFIX if _SUFFIX else "_build")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, f"libavexhip_{_SUFFIX}.so" if _SUFFIX else "libavexhip.so")
SOURCES = ["api.cpp", "encoders.cpp", "effnet_handle.cpp", "gemm.hip", "elementwise.hip", "fbank.hip", "attention.hip", "attention16.hip", "attention_hd.hip", "posconv.hip", "wavconv.hip", "melspec.hip", "effnet.hip", "probe.hip", "lstm.hip", "ingest.hip", "windows.hip", "flac.hip", "retrieval.hip", "search.hip", "events.hip", "clustering.hip", "silhouette.hip", "examples.hip", "density.hip", "activity.hip", "annotations.hip", "soundscape.hip", "measure.hip", "regions.hip"]
ARCH = "gfx950"
# Per-file flags.  hipcc's SLP vectoriser turns complex (float2) arithmetic into packed-fp32 instructions whose second source
# swaps halves (v_pk_add_f32 ... op_sel:[0,1]); on gfx950 that form reads a wrong value while another wave on the CU issues
# MFMAs (avex_amd/isa_lint.py).  The files whose arithmetic the compiler vectorises that way are built without that pass;
# packed math written out by hand (GEMM / attention epilogues) never swaps halves.  isa_lint checks the linked library.
EXTRA_FLAGS = {"fbank.hip": ["-fno-slp-vectorize"], "wavconv.hip": ["-fno-slp-vectorize"], "melspec.hip": ["-fno-slp-vectorize"],
               "lstm.hip": ["-fno-slp-vectorize"], "activity.hip": ["-fno-slp-vectorize"], "soundscape.hip": ["-fno-slp-vectorize"],
               "measure.hip": ["-fno-slp-vectorize"], "regions.hip": ["-fno-slp-vectorize"]}


def kernel_source_sha16(files=("gemm.hip", "gemm_epi.h", "common.h")) -> str:
    """First 16 hex digits of the SHA-256 over the named csrc files: the identity of a kernel's source, recorded by the PMC summaries
    under profiles/ so that bench.py can tell whether a committed counter file describes the kernel it is running."""
    import hashlib
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm; set HIPCC=/path/to/hipcc)")


def _deps_mtime() -> float:
    m = os.path.getmtime(os.path.abspath(__file__))      # the flags live here
    for root in (CSRC, os.path.join(os.path.dirname(HERE), "include")):
        for f in os.listdir(root):
            if f.endswith((".h", ".hpp")):
                m = max(m, os.path.getmtime(os.path.join(root, f)))
    return m


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    cc = hipcc()
    hdr = _deps_mtime()
    flags = [f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-x", "hip", "-Wno-unused-result",
             "-fno-gpu-rdc", "-ffp-contract=off"]
    if DIAG:
        flags.append("-DAVEX_DIAG")
    flags += os.environ.get("AVEX_AMD_EXTRA_CFLAGS", "").split()      # e.g. -DATT_STAMPS=1
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, os.path.splitext(src)[0] + ".o")
        stale = force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(s), hdr)
        if stale:
            jobs.append((s, o))

    def run(job):
        s, o = job
        cmd = [cc] + flags + EXTRA_FLAGS.get(os.path.basename(s), []) + ["-c", s, "-o", o]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {s}:\n{r.stdout}\n{r.stderr}")
        return s

    if jobs:
        if verbose:
            print(f"[avex_amd.build] compiling {len(jobs)} file(s) for {ARCH}", flush=True)
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(run, jobs))
    objs = [os.path.join(OBJ, os.path.splitext(src)[0] + ".o") for src in SOURCES]
    if jobs or force or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(o) for o in objs):
        cmd = [cc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        if verbose:
            print(f"[avex_amd.build] linked {LIB}", flush=True)
        from . import isa_lint
        n = isa_lint.check_library(LIB)      # raises on instruction forms that are wrong beside matrix work on gfx950
        if verbose:
            print(f"[avex_amd.build] isa_lint: {n} gfx950 code objects clean", flush=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
