#!/usr/bin/env python
"""What the validity check costs.

`dg_mol_validity` alone: us per call between two HIP events around a captured chain of `--event-reps` back-to-back calls (the
method of scripts/monitor_probe.py), min-max over alternated rounds, scope `whole`, with `dg_mol_canon` and
`dg_mol_fingerprint` (radius 2, 1024 bits) on the same batch next to it for scale.  The batches:

  trees      molecule-like graphs of scripts/mol_canon_probe.py (`trees`: a random tree plus two ring closures, labelled single
             or aromatic) -- most of them stop at the valence or the bridge test;
  phenyls    six-rings of aromatic carbon joined by single bonds, the rest of the positions a chain: every molecule is valid, the
             matching runs over every ring;
  triangles  N // 3 disjoint three-rings of aromatic carbon: the most searches that fail (one per ring);
  azulenes   one chain of fused five- and seven-rings with an odd atom count: nested blossoms, one search across all of them.

at B = 1024 with N = 45 and at B = 64 with N = 256 (255 for the last two).  One lane per workgroup runs the matching, so the
time follows the serial work of the slowest molecules, not the bytes, which are far below any roof.

    python scripts/mol_valid_probe.py [--out profiles/mol_valid_probe.txt] [--rounds 5]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from druggen_amd import canon, decode, fingerprint, validity
from mol_canon_probe import E, M, logits, trees
from mol_fp_probe import ATOM_DECODER, BOND_DECODER
from monitor_probe import chain_of, event_us

SINGLE, AROMATIC, CARBON = 1, 4, 1


def _ring(labels, atoms, label):
    for u, v in zip(atoms, atoms[1:] + atoms[:1]):
        labels[max(u, v), min(u, v)] = label


def phenyls(N):
    labels = np.zeros((N, N), dtype=np.int64)
    for first in range(0, N - N % 6, 6):
        _ring(labels, list(range(first, first + 6)), AROMATIC)
        if first:
            labels[first, first - 3] = SINGLE
    for a in range(N - N % 6, N):
        labels[a, a - 1] = SINGLE
    return labels


def triangles(N):
    labels = np.zeros((N, N), dtype=np.int64)
    for first in range(0, N - N % 3, 3):
        _ring(labels, [first, first + 1, first + 2], AROMATIC)
    return labels


def azulenes(N):
    """Rings of 5, 7, 5, ... atoms, each fused over a bond between two new atoms of the one before, while they fit."""
    labels = np.zeros((N, N), dtype=np.int64)
    new, used, size = list(range(5)), 5, 7
    _ring(labels, new, AROMATIC)
    while used + size - 2 <= N:
        k = len(new) // 2 - 1
        path = [new[k]] + list(range(used, used + size - 2)) + [new[k + 1]]
        for u, v in zip(path, path[1:]):
            labels[max(u, v), min(u, v)] = AROMATIC
        new, used, size = path[1:-1], used + size - 2, 12 - size
    return labels, used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--event-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mol_valid_probe.py measures on the GPU: none found")
    reps = args.event_reps
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# mol_valid_probe on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}: E={E} M={M}, scope whole")
    say(f"# us per call between two HIP events around a captured chain of {reps} calls: min-max over {args.rounds} alternated rounds")
    say("# batch          B    N  bonds/mol  valid  not kek.  other  mean deficiency    dg_mol_canon   fp r=2 1024 bits   dg_mol_validity")
    tables = validity.ValenceTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")
    fp_tables = fingerprint.FingerprintTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)

    def carbon(B, labels, used=None):
        atoms = np.zeros((B, labels.shape[0]), dtype=np.int64)
        atoms[:, :labels.shape[0] if used is None else used] = CARBON
        return torch.from_numpy(atoms).cuda(), torch.from_numpy(np.broadcast_to(labels, (B,) + labels.shape).copy()).cuda()

    batches = []
    for B, N in ((1024, 45), (64, 256)):
        odd = N - 1 + N % 2                                            # 45, 255
        batches += [("trees", trees(B, N, gen)), ("phenyls", carbon(B, phenyls(N))), ("triangles", carbon(B, triangles(odd))),
                    ("azulenes", carbon(B, *azulenes(odd)))]
    for name, (atoms, labels) in batches:
        B, N = atoms.shape
        cap = N * (N - 1) // 2
        decoded = decode.decode_molecule_graphs(*logits(atoms, labels))
        forms = canon.CanonicalForms.empty(B, N, cap, "cuda", "whole")
        fps = fingerprint.CircularFingerprints.empty(B, 1024, "cuda")
        out = validity.MoleculeValidity.empty(B, N, cap, "cuda")
        chains = [chain_of(lambda: canon.canonical_forms(decoded, "whole", out=forms), reps),
                  chain_of(lambda: fingerprint.circular_fingerprints(decoded, fp_tables, 2, 1024, "whole", out=fps), reps),
                  chain_of(lambda: validity.check_molecules(decoded, tables, "whole", out=out), reps)]
        spans = [[] for _ in chains]
        for r in range(args.rounds):
            for k in (range(len(chains)) if r % 2 == 0 else reversed(range(len(chains)))):
                spans[k].append(event_us(chains[k], reps))
        bonds = float(decoded.cpu().n_bonds.mean())
        host = out.cpu()
        valid, odd_out = int((host.status == 0).sum()), int((host.status == 5).sum())
        computed = host.deficiency[host.deficiency >= 0]
        say(f"{name:10s} {B:6d} {N:4d} {bonds:10.1f} {valid:6d} {odd_out:9d} {B - valid - odd_out:6d} "
            f"{float(computed.mean()) if len(computed) else float('nan'):16.2f}   "
            + "   ".join(f"{min(s):7.1f}-{max(s):<8.1f}" for s in spans))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
