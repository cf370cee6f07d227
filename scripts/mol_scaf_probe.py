#!/usr/bin/env python
"""What the scaffold kernel costs.

`dg_mol_scaffold` alone: us per call between two HIP events around a captured chain of `--event-reps` back-to-back calls (the
method of scripts/monitor_probe.py), min-max over alternated rounds, scope `whole`, with `dg_mol_descriptors` on the same batch
next to it -- the call whose keys and bond classes it reads.  The batches of scripts/mol_desc_probe.py:

  trees      molecule-like graphs of scripts/mol_canon_probe.py -- those that are not valid leave the kernel at once;
  phenyls    six-rings of aromatic carbon joined by single bonds: every atom is kept, one ring-size search per ring bond, each
             six levels deep;
  ethers     one chain of single bonds: no ring, the deepest peel (N / 2 rounds), an empty scaffold;
  strips     fused three-rings: two ring bonds per atom, every search ends at its first level, one ring system of N atoms.

at B = 1024 with N = 45 and at B = 64 with N = 256.  No bar is set: nothing comparable exists at the parent commit and RDKit is
absent here, so these are unreviewed measurements.

    python scripts/mol_scaf_probe.py [--out profiles/mol_scaf_probe.txt] [--rounds 5]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from druggen_amd import decode, descriptors, scaffolds, validity
from mol_canon_probe import E, M, logits, trees
from mol_desc_probe import CARBON, ethers, strips
from mol_fp_probe import ATOM_DECODER, BOND_DECODER
from mol_valid_probe import phenyls
from monitor_probe import chain_of, event_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--event-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mol_scaf_probe.py measures on the GPU: none found")
    reps = args.event_reps
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# mol_scaf_probe on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}: E={E} M={M}, scope whole; unreviewed measurements")
    say(f"# us per call between two HIP events around a captured chain of {reps} calls: min-max over {args.rounds} alternated rounds")
    say("# batch          B    N  bonds/mol  valid  scaffold atoms/valid  ring bonds/valid  max ring   dg_mol_descriptors   dg_mol_scaffold")
    vtables = validity.ValenceTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")
    dtables = descriptors.DescriptorTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)

    def same(B, atoms, labels):
        return (torch.from_numpy(np.broadcast_to(atoms, (B,) + atoms.shape).copy()).cuda(),
                torch.from_numpy(np.broadcast_to(labels, (B,) + labels.shape).copy()).cuda())

    batches = []
    for B, N in ((1024, 45), (64, 256)):
        carbon = np.full(N, CARBON, dtype=np.int64)
        batches += [("trees", trees(B, N, gen)), ("phenyls", same(B, carbon, phenyls(N))), ("ethers", same(B, *ethers(N))),
                    ("strips", same(B, *strips(N)))]
    for name, (atoms, labels) in batches:
        B, N = atoms.shape
        cap = N * (N - 1) // 2
        decoded = decode.decode_molecule_graphs(*logits(atoms, labels))
        checked = validity.check_molecules(decoded, vtables, "whole")
        described = descriptors.MoleculeDescriptors.empty(B, N, cap, "cuda")
        out = scaffolds.MoleculeScaffolds.empty(B, N, cap, "cuda")
        chains = [chain_of(lambda: descriptors.describe_molecules(decoded, checked, dtables, "whole", out=described), reps),
                  chain_of(lambda: scaffolds.murcko_scaffolds(decoded, described, dtables, out=out), reps)]
        spans = [[] for _ in chains]
        for r in range(args.rounds):
            for k in (range(len(chains)) if r % 2 == 0 else reversed(range(len(chains)))):
                spans[k].append(event_us(chains[k], reps))
        bonds = float(decoded.cpu().n_bonds.mean())
        host = out.cpu()
        ok = host.status == 0
        valid = int(ok.sum())
        per = (lambda x: float(x[ok].mean())) if valid else (lambda x: float("nan"))
        say(f"{name:10s} {B:6d} {N:4d} {bonds:10.1f} {valid:6d} {per(host.n_scaffold_atoms):21.1f} {per(host.n_ring_bonds):17.1f} "
            f"{int(host.max_ring.max()):9d}   " + "   ".join(f"{min(s):8.1f}-{max(s):<9.1f}" for s in spans))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
