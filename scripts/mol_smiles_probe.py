#!/usr/bin/env python
"""What writing the strings costs: `dg_mol_smiles` next to `dg_mol_canon` on the same decoded batch, us per call
between two HIP events around a captured chain of `--event-reps` back-to-back calls (the method of scripts/monitor_probe.py),
min-max over alternated rounds.  Molecule-like graphs (scripts/mol_canon_probe.py `trees`: a random tree plus two ring
closures), scope "whole", at B = 256 / 2048 with N = 45 and at B = 64 with N = 256; the writer from the batch and from its
canonical forms.  Bytes: what one launch of the writer reads (atom labels, the listed bond rows, counts) and writes (text,
order, length, n_written).

    python scripts/mol_smiles_probe.py [--out profiles/mol_smiles_probe.txt] [--rounds 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from druggen_amd import canon, decode, smiles_out
from mol_canon_probe import E, M, logits, trees
from monitor_probe import chain_of, event_us

# 13 atom labels as mol_canon_probe's logits have them: pad, C, N, O, F, P, S, Cl, Br, I, Se, Si, B
ATOM_DECODER = {0: 0, 1: 6, 2: 7, 3: 8, 4: 9, 5: 15, 6: 16, 7: 17, 8: 35, 9: 53, 10: 34, 11: 14, 12: 5}
BOND_DECODER = {0: 0, 1: 1, 2: 2, 3: 3, 4: 12}
assert len(ATOM_DECODER) == M and len(BOND_DECODER) == E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--event-reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mol_smiles_probe.py measures on the GPU: none found")
    reps = args.event_reps
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# mol_smiles_probe on {torch.cuda.get_device_name(0)}: E={E} M={M}, scope whole, str_cap = 8 N")
    say(f"# us per call between two HIP events around a captured chain of {reps} calls: min-max over {args.rounds} alternated rounds")
    say("#     B    N  bonds/mol  chars/mol  failed   KiB read  KiB written    dg_mol_canon     dg_mol_smiles   dg_mol_smiles(forms)")
    tables = smiles_out.SmilesTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)
    for B, N in ((256, 45), (2048, 45), (64, 256)):
        cap = N * (N - 1) // 2
        node, edge = logits(*trees(B, N, gen))
        decoded = decode.decode_molecule_graphs(node, edge)
        del node, edge
        forms = canon.CanonicalForms.empty(B, N, cap, "cuda", "whole")
        out, out_forms = smiles_out.SmilesBatch.empty(B, N, 8 * N, "cuda"), smiles_out.SmilesBatch.empty(B, N, 8 * N, "cuda")
        chains = [chain_of(lambda: canon.canonical_forms(decoded, "whole", out=forms), reps),
                  chain_of(lambda: smiles_out.write_smiles(decoded, tables, "whole", out=out), reps),
                  chain_of(lambda: smiles_out.write_smiles(forms, tables, "whole", out=out_forms), reps)]
        spans = [[] for _ in chains]
        for r in range(args.rounds):
            for k in (range(len(chains)) if r % 2 == 0 else reversed(range(len(chains)))):
                spans[k].append(event_us(chains[k], reps))
        host, text = decoded.cpu(), out.cpu()
        bonds = float(host.n_bonds.mean())
        ok = text.length >= 0
        read = B * (N + 4 * bonds + 4) + 4 * len(ATOM_DECODER) + 2 * len(BOND_DECODER)
        written = B * (8 * N + N + 8)
        say(f"{B:7d} {N:4d} {bonds:10.1f} {float(text.length[ok].mean()):10.1f} {int((~ok).sum()):7d} {read / 1024:10.1f} "
            f"{written / 1024:12.1f}   " + "   ".join(f"{min(s):7.1f}-{max(s):<8.1f}" for s in spans))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
