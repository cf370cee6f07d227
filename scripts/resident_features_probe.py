#!/usr/bin/env python
"""Feeding the step with --features node matrices: ms per batch of two routes to the same (a_tensor, labels, x_tensor),
alternated in one process.

  (a) ResidentMolecules.batch(idx, out=...) on a store with the feature plane, idx already on the GPU
      (dg_mol_gather_features);
  (b) the route without the plane: smiles.collate of B host graphs (the dense [N, atom_dim + F] float32 node matrices) ->
      .to(device) -> load_molecules(check="deferred") (dg_densify).
B = 256, N = 45, E = 5, atom_dim = 13, F = 54 in the reference's descriptor blocks, synthetic molecules (druggen_amd.synth), a
store of 4096 of them, a fresh random index per batch.  Two clocks per route, each the median over rounds with the min-max
spread: the HOST clock around `reps` batches followed by one synchronise, and HIP events around the same `reps` batches
(device time including the gaps the host leaves).  The two routes' outputs are compared bit for bit.

    python scripts/resident_features_probe.py [--out profiles/resident_features_probe.txt] [--rounds 9] [--reps 20]
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from druggen_amd import data, functional, smiles, synth
from druggen_amd.resident import ResidentMolecules

B, N, E, A, STOCK = 256, 45, 5, 13, 4096
BLOCKS = (5, 9, 6, 9, 1, 1, 5, 5, 5, 1, 7)      # the reference's descriptor blocks (dataset.py:161-185): F = 54
M = A + sum(BLOCKS)


def synthetic_graphs(n, seed):
    _, x, bonds, _ = synth.molecule_batch(n, N, E, A, seed=seed)
    rng = np.random.default_rng(seed)
    feats = []
    for width in BLOCKS:      # one-hot inside a multi-column block, a coin per single column
        block = np.zeros((n, N, width), dtype=np.float32)
        if width == 1:
            block[..., 0] = rng.integers(0, 2, size=(n, N))
        else:
            np.put_along_axis(block, rng.integers(0, width, size=(n, N, 1)), 1.0, axis=-1)
        feats.append(block)
    x = np.concatenate([x.astype(np.float32)] + feats, axis=-1)
    graphs = []
    for i in range(n):
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x[i], edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    return graphs


def clock(fn, reps):
    """(host ms, device ms) per call over `reps` calls."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for k in range(reps):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resident_features_probe.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    graphs = synthetic_graphs(STOCK, 7)
    store = ResidentMolecules.from_graphs(graphs, b_dim=E, atom_dim=A)
    assert store.m_dim == M and store.bits is not None
    out = (torch.empty(B, N, N, E, device="cuda"), torch.empty(B, N, N, dtype=torch.int32, device="cuda"),
           torch.empty(B, N, M, device="cuda"))
    rng = np.random.default_rng(11)
    host_idx = [rng.integers(0, STOCK, size=B) for _ in range(args.reps)]
    dev_idx = [torch.from_numpy(i).cuda() for i in host_idx]

    def route_a(k):
        return store.batch(dev_idx[k], out=out)

    def route_b(k):
        batch = smiles.collate([graphs[i] for i in host_idx[k]]).to("cuda")
        return data.load_molecules(batch, b_dim=E, m_dim=M, batch_size=B, check="deferred")

    (_, a_a, x_a), (_, a_b, x_b) = route_a(0), route_b(0)
    same = (torch.equal(a_a, a_b) and torch.equal(x_a, x_b)
            and torch.equal(functional.one_hot_labels(a_a), functional.one_hot_labels(a_b)))
    routes = {"a": route_a, "b": route_b}
    for fn in routes.values():
        clock(fn, args.reps)
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(clock(fn, args.reps))
    data.raise_deferred_checks(wait=True)
    store.raise_bad_indices(wait=True)

    say(f"# resident_features_probe on {torch.cuda.get_device_name(0)}: B={B} N={N} E={E} atom_dim={A} F={M - A}, synthetic molecules,")
    say(f"# a store of {STOCK} ({store.nbytes()} bytes on the device); ms per batch, median [min-max] over {args.rounds} alternated")
    say(f"# rounds of {args.reps} batches; host = host clock to the end of a final synchronise, device = HIP events around the batches")
    say("# route                                                       host ms per batch            device ms per batch")
    names = {"a": "(a) ResidentMolecules.batch(idx, out=...) with the plane", "b": "(b) smiles.collate -> .to(device) -> load_molecules(deferred)"}
    med = {}
    for k in routes:
        host, dev = [t[0] for t in times[k]], [t[1] for t in times[k]]
        med[k] = (statistics.median(host), statistics.median(dev))
        say(f"{names[k]:<60s} {med[k][0]:8.4f} [{min(host):.4f}-{max(host):.4f}]   {med[k][1]:8.4f} [{min(dev):.4f}-{max(dev):.4f}]")
    say(f"# b / a: host {med['b'][0] / med['a'][0]:.1f}, device {med['b'][1] / med['a'][1]:.1f}; outputs bit-identical: {same}")
    say(f"# bytes written per batch by (a): {4 * B * N * (N * E + N + M)} (a, labels, x); node matrix uploaded per batch by (b): {4 * B * N * M}")
    say(f"# the store per atom position: {1 + 4 * store.bits.shape[2]} bytes (dense row: {4 * M})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
