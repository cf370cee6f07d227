#!/usr/bin/env python
"""Record tests/golden/n384_bits.json: SHA-256 of every output buffer of the cases of tests/test_hip_n384_bits.py, as the
library that is loaded writes them (GPU box).  Run it at the commit whose bits are to be pinned and name that commit:

    python scripts/record_n384_bits.py --parent <commit> [--out tests/golden/n384_bits.json]

(DG_LIB=<path> records another build of the library.)  Every case is also held against float64 while it is recorded."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_hip_n384_bits as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the commit whose build is recorded")
    ap.add_argument("--out", default=cases.GOLDEN)
    args = ap.parse_args()
    table = cases.record()
    for name in cases.case_names():
        ins, first, second = cases.case_outputs(name)
        for inp, a, b in (zip(ins, first, second) if name == "pair" else [(ins, first, second)]):
            assert cases.digest(a) == cases.digest(b), name
            cases.check_float64(inp, a)
    doc = {"parent": args.parent, "kernel": "druggen_amd/csrc/row_gemm_n384.hip",
           "instances": ["row_gemm_n384_kernel<3,1> (DG_DTYPE_F32_H32 forward)", "row_gemm_n384_kernel<1,2,2> (DG_DTYPE_F32_H16 backward)"],
           "hash": "sha256", "cases": table}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(table)} cases at {args.parent} -> {args.out}")


if __name__ == "__main__":
    main()
