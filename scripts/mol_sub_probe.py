#!/usr/bin/env python
"""What the substructure matcher costs.

`dg_mol_substructure` alone: us per call between two HIP events around a captured chain of `--event-reps` back-to-back calls (the
method of scripts/monitor_probe.py), min-max over alternated rounds, with `dg_mol_descriptors` on the same batch next to it -- the
call whose keys and bond classes it reads.  Two tables:

  built-in    `substructure.LOGP` + `substructure.GROUPS`: 29 typing rows and 12 counted ones, most of them one or two atoms;
  synthetic   480 counted patterns: every pairing of 8 first atoms, 6 bonds and 10 tails of one to five atoms (chains, a branch,
              five- and six-ring closures), the size of a structural-alert catalogue.

The batches (scope `whole`, every molecule valid, so that no workgroup leaves early):

  phenyls    six-rings of aromatic carbon joined by single bonds (scripts/mol_valid_probe.py): ring closures succeed;
  ethers     one chain C C O C C N ... of single bonds (scripts/mol_desc_probe.py): hetero atoms, no ring.

at B = 256 and 2048 with N = 45 and 90.  The pattern records are read through L1 / L2 (320 bytes each, the same for every
workgroup); the kernel stages no pattern in LDS.  No bar is set: nothing comparable exists at the parent commit and RDKit is
absent here, so these are unreviewed measurements.

    python scripts/mol_sub_probe.py [--out profiles/mol_sub_probe.txt] [--rounds 5]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from druggen_amd import decode, descriptors, substructure, validity
from mol_canon_probe import E, M, logits
from mol_desc_probe import CARBON, ethers
from mol_fp_probe import ATOM_DECODER, BOND_DECODER
from mol_valid_probe import phenyls
from monitor_probe import chain_of, event_us


def synthetic():
    """480 counted patterns."""
    heads = ("[C]", "[C;a]", "[C;A]", "[N]", "[O]", "[!C]", "[*;R]", "[C;H0]")
    bonds = ("", "-", "=", ":", "~", "-!@")
    tails = ("{b}[C]", "{b}[!C]", "{b}[C]~[C]", "{b}[C]~[*]~[*]", "{b}[*]~[*]~[*]~[*]", "{b}[C]([*])~[*]", "{b}[*]~[*]~[*]~[*]~[*]",
             "1{b}[*]~[*]~[*]~[*]~[*]~1", "1{b}[*]~[*]~[*]~[*]~1", "{b}[C;a]:[C;a]-[*]")
    rows = []
    for h in heads:
        for b in bonds:
            for t in tails:
                rows.append((f"s{len(rows)}", h + t.format(b=b)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--event-reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mol_sub_probe.py measures on the GPU: none found")
    reps = args.event_reps
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    vtables = validity.ValenceTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")
    dtables = descriptors.DescriptorTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")
    tables = [("built-in", substructure.SubstructureTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")),
              ("synthetic", substructure.SubstructureTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda", typing=(), patterns=synthetic()))]
    say(f"# mol_sub_probe on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}: E={E} M={M}, scope whole; unreviewed measurements")
    say(f"# us per call between two HIP events around a captured chain of {reps} calls: min-max over {args.rounds} alternated rounds")
    say("# tables: " + ", ".join(f"{name} {t.n_patterns} patterns" for name, t in tables) + "; pattern records read through L1 / L2")
    say("# batch          B    N  valid  hit/valid(built-in)  hit/valid(synthetic)  over   dg_mol_descriptors   dg_mol_substructure: built-in   synthetic")

    def same(B, atoms, labels):
        return (torch.from_numpy(np.broadcast_to(atoms, (B,) + atoms.shape).copy()).cuda(),
                torch.from_numpy(np.broadcast_to(labels, (B,) + labels.shape).copy()).cuda())

    for B in (256, 2048):
        for N in (45, 90):
            carbon = np.full(N, CARBON, dtype=np.int64)
            for name, (atoms, labels) in (("phenyls", same(B, carbon, phenyls(N))), ("ethers", same(B, *ethers(N)))):
                cap = N * (N - 1) // 2
                decoded = decode.decode_molecule_graphs(*logits(atoms, labels))
                checked = validity.check_molecules(decoded, vtables, "whole")
                described = descriptors.MoleculeDescriptors.empty(B, N, cap, "cuda")
                outs = [substructure.MoleculeMatches.empty(B, N, t.n_patterns, "cuda") for _, t in tables]
                chains = [chain_of(lambda: descriptors.describe_molecules(decoded, checked, dtables, "whole", out=described), reps)]
                chains += [chain_of(lambda t=t, o=o: substructure.match_molecules(decoded, described, t, out=o), reps)
                           for (_, t), o in zip(tables, outs)]
                spans = [[] for _ in chains]
                for r in range(args.rounds):
                    for k in (range(len(chains)) if r % 2 == 0 else reversed(range(len(chains)))):
                        spans[k].append(event_us(chains[k], reps))
                hosts = [o.cpu() for o in outs]
                ok = hosts[0].status == 0
                valid = int(ok.sum())
                per = (lambda x: float(x[ok].mean())) if valid else (lambda x: float("nan"))
                say(f"{name:10s} {B:6d} {N:4d} {valid:6d} {per(hosts[0].n_patterns_hit):20.1f} {per(hosts[1].n_patterns_hit):21.1f} "
                    f"{int(hosts[0].n_over.sum() + hosts[1].n_over.sum()):5d}   "
                    + "   ".join(f"{min(s):8.1f}-{max(s):<9.1f}" for s in spans))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
