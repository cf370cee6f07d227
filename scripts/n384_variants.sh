#!/bin/bash
# Ablation timing of the 128 -> 384 producer / consumer row GEMM: one line per -DN3_DBG=<bits> build (scripts/build_variant.sh
# n3_<bits> row_gemm_n384.hip -DN3_DBG=<bits>; bits: 1 no MFMAs, 2 no epilogue arithmetic, 4 no output stores, 8 no fetch), the
# two hot instances alone (scripts/n384_time.py), all inside one GPU call.  Every run has its own time limit; the first run
# that fails ends the script.
cd "$(dirname "$0")/.." || exit 1
for rep in 1 2; do
for v in druggen_amd/lib/variants/n3_*.so; do
  DG_LIB=$PWD/$v timeout -k 10 120 python scripts/n384_time.py || exit 1
done
done
