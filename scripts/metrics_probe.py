#!/usr/bin/env python
"""Fingerprint similarity: device time of `metrics.tanimoto_aggregate` (packed words, dg_fp_tanimoto) against the dense
float32 matrix-product route on the SAME GPU in the same process.

Shapes (1024-bit fingerprints, density 2-8 % per row): G = 100 and G = 10 000 against S = 1 000 000 (max: SNN), and a
10 000-row self-comparison (mean: IntDiv, and max).  The baseline is what a user could do with torch alone: keep the
fingerprints as dense float32 on the GPU, take the intersections with `torch.mm` block by block, divide, and reduce.
Both routes are timed with HIP events around `reps` calls (the packed route: at least 10 where a call is short) after a
warm-up at the same shape; the outputs are compared.
The roof is VALU issue: a pair needs 2 W wave-instructions-per-lane (v_and_b32 + v_bcnt_u32_b32 per word) and the chip
issues 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz.

    python scripts/metrics_probe.py [--out profiles/metrics_probe.txt] [--reps 3]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from druggen_amd import metrics

NBITS = 1024
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def random_dense(n, seed):
    """[n, NBITS] float32 0/1 on the GPU, made in chunks."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(n, NBITS, dtype=torch.float32, device="cuda")
    for i in range(0, n, 65536):
        m = min(65536, n - i)
        density = 0.02 + 0.06 * torch.rand(m, 1, device="cuda", generator=g)
        out[i:i + m] = (torch.rand(m, NBITS, device="cuda", generator=g) < density).float()
    return out


def dense_route(stock, gen, agg, block=8192):
    """Blocks of the stock against all of gen: intersections by float32 matmul, a + b - c, divide, 0 / 0 -> 1, reduce."""
    b = gen.sum(1)[None, :]
    gen_t = gen.t().contiguous()
    acc = torch.zeros(gen.shape[0], dtype=torch.float64 if agg == "mean" else torch.float32, device=gen.device)
    for i in range(0, stock.shape[0], block):
        x = stock[i:i + block]
        c = x @ gen_t
        sim = c / (x.sum(1, keepdim=True) + b - c)
        sim = torch.nan_to_num_(sim, nan=1.0)
        if agg == "max":
            acc = torch.maximum(acc, sim.amax(0))
        else:
            acc += sim.sum(0, dtype=torch.float64)
    return acc / stock.shape[0] if agg == "mean" else acc.double()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stock", type=int, default=1_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_probe.py measures on the GPU: none found")
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# metrics_probe: {NBITS}-bit fingerprints, density 2-8 %; ms per call, HIP events around `reps` calls after a warm-up")
    say("# (reps p/d = calls timed of the packed / dense route)")
    say("# packed = metrics.tanimoto_aggregate on PackedFingerprints (dg_fp_tanimoto + combine); dense = float32 torch.mm route, same GPU")
    say("# roof = pairs x 2 W lane-instructions / (256 CUs x 4 SIMDs x 32 lanes/clk x 2.4 GHz)")
    say("# max |diff| = packed vs dense outputs")
    say("#       G         S   agg  reps p/d    packed ms    dense ms   dense/packed   roof ms   packed: share of roof   max |diff|")
    stock = random_dense(args.stock, 1)
    gen_big = random_dense(10_000, 2)
    p_stock, p_big = metrics.pack_fingerprints(stock), metrics.pack_fingerprints(gen_big)
    p_small = metrics.PackedFingerprints(p_big.words[:100].contiguous(), p_big.counts[:100].contiguous(), NBITS)
    shapes = [("max", p_stock, p_small, stock, gen_big[:100]), ("max", p_stock, p_big, stock, gen_big),
              ("mean", p_big, p_big, gen_big, gen_big), ("max", p_big, p_big, gen_big, gen_big)]
    slower = []
    for agg, ps, pg, ds, dg in shapes:
        S, G = len(ps), len(pg)
        reps_p = max(args.reps, 10 if S * G < 5e8 else args.reps)
        t_packed, got = timed(lambda: metrics.tanimoto_aggregate(ps, pg, agg), reps_p)
        t_dense, want = timed(lambda: dense_route(ds, dg, agg), args.reps)
        roof = S * G * 2 * (NBITS // 32) / LANE_OPS_PER_S * 1e3
        diff = float((got - want).abs().max())
        say(f"{G:9d} {S:9d}   {agg:4s} {reps_p:5d}/{args.reps:<3d} {t_packed:11.3f} {t_dense:11.3f} {t_dense / t_packed:14.1f} {roof:9.3f} {roof / t_packed:23.3f} {diff:12.2e}")
        if t_packed >= t_dense:
            slower.append((G, S, agg))
    say("# packed is faster than the dense route at every shape" if not slower else f"# packed is NOT faster at {slower}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
