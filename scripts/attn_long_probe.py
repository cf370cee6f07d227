"""Attention core at long neighbour lists: forward, backward and second order timed with HIP events.

    python scripts/attn_long_probe.py [--out FILE]

N = 90 runs the short kernels (dg_attn_core_*), for comparison; N = 97 ... 256 the long ones (dg_attn_core_long_*).  B is
chosen so that every [B,N,N,C] tensor has at least 500k edge rows.  "floor" is the time the [B,N,N,C] tensors take at
8 TB/s when each is read or written once (fwd: e, s; bwd: e, ws, de; bwd2: e, ws, te, ge, gws); the [B,N,C] operands and
the column partials of the long backward are left out of it.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from druggen_amd import functional as dgf  # noqa: E402

HBM = 8.0e12
EDGE_TENSORS = {"fwd": 2, "bwd": 3, "bwd2": 5}


def time_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    C, alpha = 128, 0.25
    lines = [f"attention core, C = {C}, HIP events, mean of {args.reps} launches after one warm-up; "
             f"{torch.cuda.get_device_name(0)}",
             f"{'N':>4} {'B':>4} {'rows':>8} {'dtype':>5} {'op':>5} {'kernel':>6} {'us':>9} {'floor us':>9} {'of floor':>8}"]
    for N in (90, 97, 128, 192, 256):
        B = math.ceil(500_000 / (N * N))
        for dt in (torch.float32, torch.bfloat16):
            g = torch.Generator(device="cuda").manual_seed(0)
            mk = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.7).to(dt)
            q, k, v, e = mk(B, N, C), mk(B, N, C), mk(B, N, C), mk(B, N, N, C)
            ws, wo = mk(B, N, N, C), mk(B, N, C)
            tq, tk, tv, te = mk(B, N, C), mk(B, N, C), mk(B, N, C), mk(B, N, N, C)
            ops = (("fwd", lambda: dgf._AttnCore.apply(q, k, v, e, alpha, True)),
                   ("bwd", lambda: dgf._attn_bwd_launch(q, k, v, e, ws, wo, alpha)),
                   ("bwd2", lambda: dgf._attn_bwd2_launch(q, k, v, e, ws, wo, tq, tk, tv, te, alpha)))
            for name, fn in ops:
                us = time_us(fn, args.reps)
                floor = EDGE_TENSORS[name] * B * N * N * C * e.element_size() / HBM * 1e6
                kind = "short" if N <= dgf.ATTN_SHORT_MAX_N else "long"
                lines.append(f"{N:>4} {B:>4} {B * N * N:>8} {str(dt)[6:]:>5} {name:>5} {kind:>6} {us:>9.1f} {floor:>9.1f} "
                             f"{floor / us:>8.2f}")
                print(lines[-1], flush=True)
            del q, k, v, e, ws, wo, tq, tk, tv, te
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
