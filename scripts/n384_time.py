#!/usr/bin/env python
"""Timing of the two hot instances of csrc/row_gemm_n384.hip alone (developer tool, GPU box): the fc1 forward writing
DG_DTYPE_F32_H32 (row_gemm_n384_kernel<3,1>) and dh = (dz W2) * m writing DG_DTYPE_F32_H16 (row_gemm_n384_kernel<1,2,2>), at
R = 518 400 and 1 036 800 rows.  One line per library build: run once per DG_LIB (scripts/n384_variants.sh runs every
-DN3_DBG=<bits> ablation build of scripts/build_variant.sh).  Rates are the launch's accounted bytes over its time."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from druggen_amd import _lib as L, functional as dgf  # noqa: E402
from bench_kernels import timeit  # noqa: E402

C, H = 128, 384
name = os.path.basename(os.environ.get("DG_LIB", "shipped")).replace(".so", "")
torch.manual_seed(0)
w1, b1, w2 = torch.randn(H, C, device="cuda") * 0.1, torch.randn(H, device="cuda"), torch.randn(C, H, device="cuda") * 0.1
pw1, pw2 = dgf.packed_weight(w1, 0), dgf.packed_weight(w2, 1)
parts = []
for R in (518400, 1036800):
    x = torch.randn(R, C, device="cuda")
    words = (R + 31) // 32 * 512
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int32, device="cuda")
    t_f = timeit(lambda: dgf.row_gemm(x, pw1, C, H, bias=b1, relu=True, want_relu_bits=True, code=L.F32_H32))
    t_b = timeit(lambda: dgf.row_gemm(x, pw2, C, H, mask_bits=bits, code=L.F32_H16))
    by_f, by_b = R * (512 + 1536 + 4 + 64), R * (512 + 64 + 768 + 4)
    parts.append(f"R={R}: fwd<3,1> {t_f:6.1f} us {by_f / t_f / 1e6:4.2f} TB/s  bwd<1,2,2> {t_b:6.1f} us {by_b / t_b / 1e6:4.2f} TB/s")
    del x, bits
print(f"{name:12s} " + " | ".join(parts), flush=True)
