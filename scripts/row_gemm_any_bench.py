#!/usr/bin/env python
"""A/B of the hook ``options.row_gemm_any`` (float32 nn.Linear of other widths than 128 / 384 on dg_row_gemm_any,
csrc/row_gemm_any.hip, against the ROCm BLAS route it replaces) in ONE process on one GPU; the hook alternates False / True.
    python scripts/row_gemm_any_bench.py [rounds=5] [iters=20] [steps=3] > profiles/row_gemm_any.txt
Kernel level: ``_mm_rows`` at the edge-level row count R = 256 * 45 * 45, forward (mode 0, with bias: the BLAS route adds it in a
launch of its own) and input gradient (mode 1), HIP-event averages over ``iters`` launches after warm-up.
Step level: a full GAN step (GANStep: D step with gradient penalty, G step, both AdamW updates) of the dim = 64 and dim = 256
models at B = 256, N = 45, L = 4, ``steps`` steps per run, synchronised before and after.
A setting is slower only if its mean exceeds the other's by more than the largest difference between two runs of one setting."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from druggen_amd import functional as dgf, synth  # noqa: E402
from druggen_amd.model import Discriminator, Generator  # noqa: E402
from druggen_amd.options import options  # noqa: E402
from druggen_amd.trainer import GANStep  # noqa: E402

R = 256 * 45 * 45
SHAPES = [(64, 64), (64, 192), (192, 64), (256, 256), (256, 768), (768, 256)]
MODELS = [dict(dim=64, heads=8, mlp_ratio=3, depth=4), dict(dim=256, heads=8, mlp_ratio=3, depth=4)]


def summary(runs, unit):
    mean = {k: sum(v) / len(v) for k, v in runs.items()}
    spread = max(max(v) - min(v) for v in runs.values())
    verdict = "slower" if mean[True] > mean[False] + spread else ("faster" if mean[True] < mean[False] - spread else "same")
    return (f"blas {mean[False]:9.3f} {unit}  any {mean[True]:9.3f} {unit}  ratio {mean[False] / mean[True]:5.2f}  "
            f"spread {spread:7.3f} {unit}  -> {verdict}")


def kernel_level(rounds, iters, dev):
    print(f"# kernel level: _mm_rows, R = {R}, {iters} launches per run, {rounds} alternations; us per launch")
    g = torch.Generator(device=dev).manual_seed(1)
    for K, N in SHAPES:
        for mode in (0, 1):
            a = torch.randn(R, K, device=dev, generator=g)
            w = torch.randn((N, K) if mode == 0 else (K, N), device=dev, generator=g) * K ** -0.5
            b = torch.randn(N, device=dev, generator=g) if mode == 0 else None
            runs = {False: [], True: []}
            outs = {}
            for on in (False, True):      # warm-up of both routes (pack, BLAS algorithm choice)
                options.row_gemm_any = on
                for _ in range(3):
                    outs[on] = dgf._mm_rows(a, w, mode, b)
            err = ((outs[True] - outs[False]).double().norm() / outs[False].double().norm()).item()
            del outs
            for _ in range(rounds):
                for on in (False, True):
                    options.row_gemm_any = on
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        dgf._mm_rows(a, w, mode, b)
                    e1.record()
                    e1.synchronize()
                    runs[on].append(e0.elapsed_time(e1) / iters * 1e3)
            nbytes = 4 * R * (K + N)
            t = sum(runs[True]) / len(runs[True]) * 1e-6
            print(f"  K={K:4d} N={N:4d} {'fwd+bias' if mode == 0 else 'dgrad   '} {summary(runs, 'us')}  "
                  f"any: {nbytes / t / 1e12:5.2f} TB/s {2 * R * K * N / t / 1e12:6.1f} TFLOP/s  rel. diff {err:.1e}", flush=True)


def step_level(rounds, steps, dev):
    B, N, E, M = 256, 45, 5, 13
    print(f"# step level: GANStep at B = {B}, N = {N}, {steps} steps per run, {rounds} alternations; ms per step")
    a, x, _, _ = synth.molecule_batch(B, N, E, M, seed=1234)
    da, dx, _, _ = synth.molecule_batch(B, N, E, M, seed=2234)
    batch = [torch.from_numpy(t).to(dev) for t in (da, dx, a, x)]
    for kw in MODELS:
        torch.manual_seed(0)
        G, D = Generator("relu", N, E, M, 0.0, **kw).to(dev), Discriminator("relu", N, E, M, 0.0, **kw).to(dev)
        st = GANStep(G, D, lambda_gp=10.0)
        for on in (False, True):
            options.row_gemm_any = on
            for _ in range(2):
                st.step(*batch)
        runs = {False: [], True: []}
        for _ in range(rounds):
            for on in (False, True):
                options.row_gemm_any = on
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(steps):
                    st.step(*batch)
                torch.cuda.synchronize(dev)
                runs[on].append((time.perf_counter() - t0) / steps * 1e3)
        print(f"  dim={kw['dim']:4d} heads={kw['heads']} mlp_ratio={kw['mlp_ratio']} depth={kw['depth']}  {summary(runs, 'ms')}", flush=True)
        del st, G, D
        torch.cuda.empty_cache()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dev = torch.device("cuda", 0)
    kernel_level(rounds, iters, dev)
    if steps > 0:
        step_level(rounds, steps, dev)


if __name__ == "__main__":
    main()
