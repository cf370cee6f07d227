"""Build libdruggen_hip.so (gfx950) in-tree with hipcc.

    python -m druggen_amd.build            # rebuild if sources are newer
    python -m druggen_amd.build --force
The shared object has no PyTorch / pybind dependency: it is the C ABI declared
in include/druggen_hip.h, include/druggen_hip_text.h, include/druggen_hip_fp.h, include/druggen_hip_valid.h,
include/druggen_hip_desc.h, include/druggen_hip_sub.h and include/druggen_hip_scaf.h and is loaded with ctypes (druggen_amd/_lib.py).
"""
from __future__ import annotations

import glob
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB_DIR = os.path.join(PKG, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libdruggen_hip.so")
INCLUDE = os.path.join(os.path.dirname(PKG), "include")
HEADERS = [os.path.join(INCLUDE, "druggen_hip.h"), os.path.join(INCLUDE, "druggen_hip_text.h"),
           os.path.join(INCLUDE, "druggen_hip_fp.h"), os.path.join(INCLUDE, "druggen_hip_valid.h")]
# the fifth header, beside the list: tests/test_mol_valid_host.py pins HEADERS to the four above
DESC_HEADER = os.path.join(INCLUDE, "druggen_hip_desc.h")
# ... and the sixth
SUB_HEADER = os.path.join(INCLUDE, "druggen_hip_sub.h")
# ... and the seventh
SCAF_HEADER = os.path.join(INCLUDE, "druggen_hip_scaf.h")
ARCH = "gfx950"


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def _stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = sources() + glob.glob(os.path.join(CSRC, "*.h")) + HEADERS + [DESC_HEADER, SUB_HEADER, SCAF_HEADER]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libdruggen_hip.so")
    os.makedirs(LIB_DIR, exist_ok=True)
    objs, jobs = [], []
    headers = glob.glob(os.path.join(CSRC, "*.h")) + HEADERS + [DESC_HEADER, SUB_HEADER, SCAF_HEADER]
    for src in sources():
        obj = os.path.join(LIB_DIR, os.path.basename(src) + ".o")
        objs.append(obj)
        if (not force and os.path.exists(obj) and os.path.getmtime(obj) > os.path.getmtime(src)
                and all(os.path.getmtime(obj) > os.path.getmtime(h) for h in headers)):
            continue
        jobs.append([hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast",
                     "-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if jobs:     # one hipcc per translation unit, in parallel
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as pool:
            list(pool.map(run, jobs))
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
