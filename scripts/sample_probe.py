#!/usr/bin/env python
"""Molecule sampling: ms per batch of three routes, alternated in one process.

  (a) today's route: eager G(a, x) under inference_mode, decode_molecule_labels, per-molecule `.cpu().numpy()` of both
      label tensors (reference inference.py:200-201);
  (b) eager forward + decode_molecule_graphs + one `.cpu()` for the batch;
  (c) MoleculeSampler(graph=True): forward + decode replayed as one hipGraph, one `.cpu()`.
N = 45, E = 5, M = 13, dim 128, depth 4 and 1, B in {1, 8, 64, 256}; every figure is the median over rounds of a host clock
around `reps` batches that end in the device->host copy (each route synchronises itself), with the min-max spread.
Then dg_decode_graph alone at B = 1, 256, 2048 and 8192: device time per launch against the streaming time of its input.

    python scripts/sample_probe.py [--out profiles/sample_probe.txt] [--rounds 7]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from druggen_amd import decode, synth
from druggen_amd.model import Generator
from druggen_amd.sampling import MoleculeSampler

N, E, M, DIM = 45, 5, 13, 128
ORDER2 = [0, 2, 4, 6, 3]
HBM_TBS = 6.3      # achievable streaming rate of an MI355X (8 TB/s peak), TB/s


def route_a(G, a, x):
    with torch.inference_mode():
        _, _, ns, es = G(a, x)
        n_lab, e_lab = decode.decode_molecule_labels(ns, es)
    return [(n_.data.cpu().numpy(), e_.data.cpu().numpy()) for n_, e_ in zip(n_lab, e_lab)]


def route_b(G, a, x):
    with torch.inference_mode():
        _, _, ns, es = G(a, x)
        batch = decode.decode_molecule_graphs(ns, es, bond_order2=ORDER2)
    return batch.cpu()


def clock(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_probe.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# sample_probe: N={N} E={E} M={M} dim={DIM}; ms per batch, median [min-max] over {args.rounds} alternated rounds")
    say("# depth     B   (a) eager+labels+per-mol cpu   (b) eager+graph decode+1 cpu   (c) graphed sampler      b/a    c/a")
    for depth in (4, 1):
        torch.manual_seed(depth)
        G = Generator("relu", N, E, M, 0.0, dim=DIM, depth=depth, heads=8, mlp_ratio=3).cuda().eval()
        for B in (1, 8, 64, 256):
            a_np, x_np, _, _ = synth.molecule_batch(B, N, E, M, seed=100 + B)
            a, x = torch.from_numpy(a_np).cuda(), torch.from_numpy(x_np).cuda()
            sampler = MoleculeSampler(G, a, x, bond_order2=ORDER2)
            routes = {"a": lambda: route_a(G, a, x), "b": lambda: route_b(G, a, x), "c": lambda: sampler.sample(a, x).cpu()}
            reps = max(3, min(50, 2000 // (B * depth)))
            for fn in routes.values():      # warm every route at this shape
                clock(fn, 3)
            times = {k: [] for k in routes}
            for _ in range(args.rounds):
                for k, fn in routes.items():
                    times[k].append(clock(fn, reps))
            med = {k: statistics.median(v) for k, v in times.items()}
            cell = {k: f"{med[k]:9.3f} [{min(v):.3f}-{max(v):.3f}]" for k, v in times.items()}
            say(f"{depth:7d} {B:5d}   {cell['a']:>28s}   {cell['b']:>28s}   {cell['c']:>28s}   {med['b'] / med['a']:5.2f}  {med['c'] / med['a']:5.2f}")
            del sampler
    say("# dg_decode_graph alone: 20 launches captured into one hipGraph (no host time between them), device events around")
    say("# 5 replays; random logits = dense graphs / biased = ~95 % no-bond pairs; input read from wherever it lives after")
    say("# the previous launch (88 MB at B = 2048 fit the Infinity Cache)")
    say("#     B   logits     us/launch   input MB   input stream us @6.3 TB/s   fraction of streaming rate")
    order2 = torch.tensor(ORDER2, dtype=torch.uint8, device="cuda")
    for B in (1, 256, 2048, 8192):
        g = torch.Generator(device="cuda").manual_seed(B)
        ns = torch.randn(B, N, M, device="cuda", generator=g)
        es = torch.randn(B, N, N, E, device="cuda", generator=g)
        for kind in ("dense", "sparse"):
            if kind == "sparse":
                es[..., 0] += torch.where(torch.rand(B, N, N, device="cuda", generator=g) < 0.95, 20.0, 0.0)
            out = decode.MoleculeBatch.empty(B, N, N * (N - 1) // 2, True, "cuda")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    decode.decode_molecule_graphs(ns, es, bond_order2=order2, out=out)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(20):
                    decode.decode_molecule_graphs(ns, es, bond_order2=order2, out=out)
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / 100 * 1e3
            in_bytes = 4 * B * N * (N * E + M)
            floor = in_bytes / (HBM_TBS * 1e12) * 1e6
            say(f"{B:7d}   {kind:6s}   {us:10.1f}   {in_bytes / 1e6:8.2f}   {floor:24.2f}   {floor / us:10.3f}")
            del graph
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
