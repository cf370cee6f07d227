#!/usr/bin/env python
"""What the descriptors cost.

`dg_mol_descriptors` alone: us per call between two HIP events around a captured chain of `--event-reps` back-to-back calls (the
method of scripts/monitor_probe.py), min-max over alternated rounds, scope `whole`, with `dg_mol_validity` on the same batch
next to it -- the call whose verdicts it reads.  The batches:

  trees      molecule-like graphs of scripts/mol_canon_probe.py (`trees`: a random tree plus two ring closures) -- those that
             are not valid leave the descriptor kernel at once, which is the regime of an untrained generator;
  phenyls    six-rings of aromatic carbon joined by single bonds (scripts/mol_valid_probe.py): every molecule is valid, every
             second bridge rotatable, no polar atom;
  ethers     one chain C C O C C N ... of single bonds: every molecule valid, the longest breadth-first forest (one level per
             atom) and a table search for every third atom;
  strips     fused three-rings (i - i + 1, i - i + 2): four neighbours per atom, every triangle test finds one.

at B = 1024 with N = 45 and at B = 64 with N = 256, the sizes of scripts/mol_valid_probe.py.  Both kernels walk the bond list
per phase and build the same forest, one level per turn; the descriptor kernel has no matching to run.

    python scripts/mol_desc_probe.py [--out profiles/mol_desc_probe.txt] [--rounds 5]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from druggen_amd import decode, descriptors, validity
from mol_canon_probe import E, M, logits, trees
from mol_fp_probe import ATOM_DECODER, BOND_DECODER
from mol_valid_probe import phenyls
from monitor_probe import chain_of, event_us

SINGLE, CARBON, NITROGEN, OXYGEN = 1, 1, 2, 3


def ethers(N):
    atoms = np.array([(CARBON, CARBON, OXYGEN, CARBON, CARBON, NITROGEN)[a % 6] for a in range(N)], dtype=np.int64)
    atoms[-1] = CARBON
    labels = np.zeros((N, N), dtype=np.int64)
    labels[np.arange(1, N), np.arange(N - 1)] = SINGLE
    return atoms, labels


def strips(N):
    labels = np.zeros((N, N), dtype=np.int64)
    labels[np.arange(1, N), np.arange(N - 1)] = SINGLE
    labels[np.arange(2, N), np.arange(N - 2)] = SINGLE
    return np.full(N, CARBON, dtype=np.int64), labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--event-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mol_desc_probe.py measures on the GPU: none found")
    reps = args.event_reps
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# mol_desc_probe on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}: E={E} M={M}, scope whole")
    say(f"# us per call between two HIP events around a captured chain of {reps} calls: min-max over {args.rounds} alternated rounds")
    say("# batch          B    N  bonds/mol  valid  rot/valid  tpsa/valid  untyped   dg_mol_validity   dg_mol_descriptors")
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
        checked = validity.MoleculeValidity.empty(B, N, cap, "cuda")
        out = descriptors.MoleculeDescriptors.empty(B, N, cap, "cuda")
        chains = [chain_of(lambda: validity.check_molecules(decoded, vtables, "whole", out=checked), reps),
                  chain_of(lambda: descriptors.describe_molecules(decoded, checked, dtables, "whole", out=out), reps)]
        spans = [[] for _ in chains]
        for r in range(args.rounds):
            for k in (range(len(chains)) if r % 2 == 0 else reversed(range(len(chains)))):
                spans[k].append(event_us(chains[k], reps))
        bonds = float(decoded.cpu().n_bonds.mean())
        host = out.cpu()
        ok = host.status == 0
        valid = int(ok.sum())
        per = (lambda x: float(x[ok].mean())) if valid else (lambda x: float("nan"))
        say(f"{name:10s} {B:6d} {N:4d} {bonds:10.1f} {valid:6d} {per(host.n_rot):10.1f} {per(host.tpsa) / 100:11.2f} {int(host.n_untyped.sum()):8d}   "
            + "   ".join(f"{min(s):7.1f}-{max(s):<8.1f}" for s in spans))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
