#!/usr/bin/env python
"""What the canonical forms cost: `dg_mol_canon` and `dg_mol_canon_match` next to `dg_decode_graph` and
`dg_mol_stats` on the same inputs, us per call between two HIP events around a captured chain of `--event-reps` back-to-back
calls (the method of scripts/monitor_probe.py), min-max over alternated rounds.

  regimes  sparse  molecule-like: a random tree (atom i bonds to one of the 4 atoms before it) plus two ring closures, the
                   second half of the batch repeats the first with its atoms renumbered
           dense   normal random logits: a random label per pair, the untrained generator's regime
           worst   no bonds and one atom label: N - 1 individualisations per molecule
  All under scope "whole" (under "largest" a molecule without bonds is a single atom).
  stocks   none, 4 096 and 1 000 000 forms of random trees (bond list of 64 rows), the first quarter of the sparse batch among them

    python scripts/mol_canon_probe.py [--out profiles/mol_canon_probe.txt] [--rounds 5] [--stock 1000000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from druggen_amd import canon, decode, monitor
from monitor_probe import chain_of, event_us

E, M = 5, 13
STOCK_CAP = 64


def trees(n, N, gen, closures=2):
    """(atoms [n,N] int64, labels [n,N,N] int64, lower triangle) of molecule-like graphs, made on the device."""
    dev = "cuda"
    atoms = torch.tensor([1, 1, 1, 1, 2, 3], device=dev)[torch.randint(0, 6, (n, N), device=dev, generator=gen)]
    labels = torch.zeros(n, N, N, dtype=torch.int64, device=dev)
    rows = torch.arange(n, device=dev)
    for k in range(1, N):
        parent = k - 1 - torch.randint(0, 4, (n,), device=dev, generator=gen) % k
        labels[rows, k, parent] = torch.tensor([1, 1, 1, 2], device=dev)[torch.randint(0, 4, (n,), device=dev, generator=gen)]
    for _ in range(closures):
        i = torch.randint(2, N, (n,), device=dev, generator=gen)
        j = torch.randint(0, N, (n,), device=dev, generator=gen) % (i - 1)      # j < i - 1; an existing bond is left alone
        free = labels[rows, i, j] == 0
        labels[rows[free], i[free], j[free]] = 1
    return atoms, labels


def renumber(atoms, labels, gen):
    n, N = atoms.shape
    perm = torch.rand(n, N, device="cuda", generator=gen).argsort(1)
    full = labels + labels.transpose(1, 2)
    moved = full.gather(1, perm[:, :, None].expand(n, N, N)).gather(2, perm[:, None, :].expand(n, N, N))
    return atoms.gather(1, perm), torch.tril(moved, -1)


def logits(atoms, labels):
    return (4.0 * torch.nn.functional.one_hot(atoms, M).float()).contiguous(), (4.0 * torch.nn.functional.one_hot(labels, E).float()).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--event-reps", type=int, default=50)
    ap.add_argument("--vertexes", type=int, default=45)
    ap.add_argument("--stock", type=int, default=1_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mol_canon_probe.py measures on the GPU: none found")
    N, reps = args.vertexes, args.event_reps
    cap = N * (N - 1) // 2
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# mol_canon_probe on {torch.cuda.get_device_name(0)}: N={N} E={E} M={M}, scope whole")
    say(f"# us per call between two HIP events around a captured chain of {reps} calls: min-max over {args.rounds} alternated rounds")
    gen = torch.Generator(device="cuda").manual_seed(5)
    batches = {}
    for B in (256, 2048):
        a, l = trees(B, N, gen)
        half = B // 2
        a[half:], l[half:] = renumber(a[:B - half], l[:B - half], gen)
        batches[B] = {"sparse": logits(a, l),
                      "dense": (torch.randn(B, N, M, device="cuda", generator=gen), torch.randn(B, N, N, E, device="cuda", generator=gen)),
                      "worst": logits(torch.ones(B, N, dtype=torch.int64, device="cuda"),
                                      torch.zeros(B, N, N, dtype=torch.int64, device="cuda"))}
    # ---- the stocks: random trees in chunks, then the first quarter of the sparse batch of 2 048 ----
    stocks = {0: None}
    for S in sorted({4096, args.stock}):
        t0 = time.perf_counter()
        forms = canon.CanonicalForms.empty(S, N, STOCK_CAP, "cuda", "whole")
        own = 512
        for at in range(0, S - own, 8192):
            n = min(8192, S - own - at)
            canon._launch_canon(decode.decode_molecule_graphs(*logits(*trees(n, N, gen)), bond_cap=STOCK_CAP), 0, forms, at)
        node, edge = batches[2048]["sparse"]
        canon._launch_canon(decode.decode_molecule_graphs(node[:own], edge[:own], bond_cap=STOCK_CAP), 0, forms, S - own)
        stocks[S] = canon.CanonicalSet.from_forms(forms)
        torch.cuda.synchronize()
        say(f"# stock of {S} forms built and sorted in {time.perf_counter() - t0:.1f} s, {forms.buffer.numel() / 2**20:.0f} MiB")
    say("# regime      B   bonds/mol  splits/mol  rounds/mol  distinct   dg_decode_graph   dg_mol_stats      dg_mol_canon    " +
        "  ".join(f"match S={S:<9d}" for S in stocks))
    for B in (256, 2048):
        for name, (node, edge) in batches[B].items():
            decoded = decode.MoleculeBatch.empty(B, N, cap, False, "cuda")
            stats = monitor.MolStats.empty(B, N, "cuda")
            forms = canon.CanonicalForms.empty(B, N, cap, "cuda", "whole")
            outs = {S: canon.FormMatches.empty(B, "cuda") for S in stocks}
            chains = [chain_of(lambda: decode.decode_molecule_graphs(node, edge, out=decoded), reps),
                      chain_of(lambda: monitor.molecule_statistics(decoded, out=stats), reps),
                      chain_of(lambda: canon.canonical_forms(decoded, "whole", out=forms), reps)]
            chains += [chain_of(lambda S=S: canon.match_forms(forms, stocks[S], out=outs[S]), reps) for S in stocks]
            spans = [[] for _ in chains]
            for r in range(args.rounds):
                for k in (range(len(chains)) if r % 2 == 0 else reversed(range(len(chains)))):
                    spans[k].append(event_us(chains[k], reps))
            f = forms.cpu()
            hits = {S: outs[S].cpu() for S in stocks}
            say(f"{name:<8s} {B:5d} {f.n_bonds.mean():10.1f} {f.n_splits.mean():11.2f} {f.n_rounds.mean():11.2f} "
                f"{hits[0].total('n_distinct'):9d}   " + "   ".join(f"{min(s):6.1f}-{max(s):<7.1f}" for s in spans) +
                "   in stock: " + ", ".join(str(hits[S].total("n_in_stock")) for S in stocks if S))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
