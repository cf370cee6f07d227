#!/usr/bin/env python
"""Feeding the captured step: ms per training step of two loops over the same synthetic sets, alternated in one process
(DESIGN 3.21).

  (a) the reference-style feed: per step and per side, smiles.collate of B host graphs -> .to(device) ->
      load_molecules(check="deferred"), then GraphedGANStep.step(...) (copies into the static inputs, replay);
  (b) ResidentTrainer(graph=True): indices drawn on the device, dg_mol_gather straight into the static inputs, replay.
Shapes: the launch-bound one of DESIGN 3.5 (N = 9, L = 1, B = 32: BASELINE configs[0]) and BASELINE configs[1] (N = 45, L = 4,
B = 256); E = 5, M = 13, dim 128, float32; a molecule set and a drug set of `--stock` synthetic molecules each.  Each figure
is the median over rounds, with the min-max spread, of a host clock around `reps` steps that ends in a device synchronise.
Both loops train their own copy of the same networks; neither reads a loss on the host inside the timed window.

    python scripts/loop_probe.py [--out profiles/loop_probe.txt] [--rounds 7] [--budget 420]
"""
import argparse
import itertools
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from druggen_amd import data, smiles, synth
from druggen_amd.loop import ResidentTrainer
from druggen_amd.model import Discriminator, Generator
from druggen_amd.resident import ResidentMolecules
from druggen_amd.trainer import GANStep, GraphedGANStep

E, M, DIM = 5, 13, 128
SHAPES = [("launch-bound (DESIGN 3.5, configs[0])", 9, 1, 32, 40), ("BASELINE configs[1]", 45, 4, 256, 8)]   # name, N, L, B, reps


def synthetic_graphs(n, N, seed):
    _, x, bonds, _ = synth.molecule_batch(n, N, E, M, seed=seed)
    graphs = []
    for i in range(n):
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x[i], edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    return graphs


def networks(N, L):
    nets = []
    for cls, seed in ((Generator, 11), (Discriminator, 12)):
        net = cls("relu", N, E, M, 0.0, dim=DIM, depth=L, heads=8, mlp_ratio=3)
        params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=seed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        nets.append(net.cuda())
    return nets


def clock(step, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--stock", type=int, default=2048)
    ap.add_argument("--budget", type=float, default=420.0, help="seconds: no new round is started after this long")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loop_probe.py measures on the GPU: none found")
    started = time.perf_counter()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# loop_probe on {torch.cuda.get_device_name(0)}: E={E} M={M} dim={DIM} float32, {args.stock} molecules + {args.stock} drugs,")
    say("# synthetic; ms per training step, median [min-max] over alternated rounds; host clock around `reps` steps to the end")
    say("# of a device synchronise")
    say("# shape                                    N  L    B  rounds x reps   (a) collate+upload+densify+step   (b) ResidentTrainer       a / b")
    for name, N, L, B, reps in SHAPES:
        mol_graphs, drug_graphs = synthetic_graphs(args.stock, N, 7), synthetic_graphs(args.stock, N, 8)

        # (a): host permutations (DataLoader(shuffle=True, drop_last=True)), collate, upload, densify, copy into the capture
        def loaded(graphs, idx):
            batch = smiles.collate([graphs[i] for i in idx]).to("cuda")
            return data.load_molecules(batch, b_dim=E, m_dim=M, batch_size=B, check="deferred")[1:]
        rng = np.random.default_rng(11)

        def host_batches(n):
            while True:
                order = rng.permutation(n)
                for s in range(n // B):
                    yield order[s * B:(s + 1) * B]
        mol_idx, drug_idx = host_batches(len(mol_graphs)), host_batches(len(drug_graphs))
        G, D = networks(N, L)
        first = (*loaded(drug_graphs, range(B)), *loaded(mol_graphs, range(B)))
        graphed = GraphedGANStep(GANStep(G, D), *first)

        def step_a():
            graphed.step(*loaded(drug_graphs, next(drug_idx)), *loaded(mol_graphs, next(mol_idx)))

        # (b)
        mols = ResidentMolecules.from_graphs(mol_graphs, m_dim=M, b_dim=E)
        drugs = ResidentMolecules.from_graphs(drug_graphs, m_dim=M, b_dim=E)
        G2, D2 = networks(N, L)
        trainer = ResidentTrainer(GANStep(G2, D2), mols, drugs, batch_size=B, seed=11)
        schedule = itertools.chain.from_iterable(trainer.schedule() for _ in itertools.count())

        def step_b():
            trainer.step(*next(schedule))

        routes = {"a": step_a, "b": step_b}
        for fn in routes.values():
            clock(fn, 3)
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            if time.perf_counter() - started > args.budget:
                break
            for k, fn in routes.items():
                times[k].append(clock(fn, reps))
        data.raise_deferred_checks(wait=True)
        for store in (mols, drugs):
            store.raise_bad_indices(wait=True)
        if not times["a"]:
            say(f"{name:<40s} {N:2d} {L:2d} {B:4d}   not measured: the time budget of {args.budget:.0f} s ran out")
            continue
        finite = all(bool(torch.isfinite(torch.stack(l)).all()) for l in (graphed.losses, trainer.graphed.losses))
        med = {k: statistics.median(v) for k, v in times.items()}
        cell = {k: f"{med[k]:9.3f} [{min(v):.3f}-{max(v):.3f}]" for k, v in times.items()}
        say(f"{name:<40s} {N:2d} {L:2d} {B:4d}   {len(times['a']):4d} x {reps:<4d}   {cell['a']:>32s}   {cell['b']:>28s}   {med['a'] / med['b']:6.2f}"
            + ("" if finite else "   LOSSES NOT FINITE"))
        del graphed, trainer, schedule
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
