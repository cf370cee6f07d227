#!/usr/bin/env python
"""What the circular fingerprint costs.

`dg_mol_fingerprint` alone: us per call between two HIP events around a captured chain of `--event-reps` back-to-back calls
(the method of scripts/monitor_probe.py), min-max over rounds, on molecule-like graphs (scripts/mol_canon_probe.py `trees`: a
random tree plus two ring closures), radius 2, 1024 bits, at B = 1024 with N = 45 -- both scopes, and radius 4 -- and at
B = 64 with N = 256; `dg_mol_canon` on the same batch next to it for scale.  Bytes: what one launch reads (atom labels, the
listed bond rows, counts, components) and writes (words, counts, n_features).

`fingerprint_store` end to end: a `ResidentMolecules` store of `--store` molecules of N = 45 -- `--distinct` molecules of
`druggen_amd.synth.molecule_batch`, repeated: the kernel's time does not depend on what its neighbours hold, and the generator
is a host loop -- through gather, decode and fingerprint in chunks; a host clock around the call that ends in a device
synchronise, after a warm-up call, per round.

    python scripts/mol_fp_probe.py [--out profiles/mol_fp_probe.txt] [--rounds 5] [--store 100000]
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from druggen_amd import canon, decode, fingerprint, synth
from druggen_amd.resident import ResidentMolecules
from mol_canon_probe import E, M, logits, trees
from monitor_probe import chain_of, event_us

# 13 atom labels as mol_canon_probe's logits have them: pad, C, N, O, F, P, S, Cl, Br, I, Se, Si, B
ATOM_DECODER = {0: 0, 1: 6, 2: 7, 3: 8, 4: 9, 5: 15, 6: 16, 7: 17, 8: 35, 9: 53, 10: 34, 11: 14, 12: 5}
BOND_DECODER = {0: 0, 1: 1, 2: 2, 3: 3, 4: 12}
assert len(ATOM_DECODER) == M and len(BOND_DECODER) == E


def synthetic_store(n, distinct, N, seed):
    """`distinct` molecules of synth.molecule_batch, repeated to `n`, as one resident store."""
    _, x, bonds, _ = synth.molecule_batch(distinct, N, E, M, seed=seed)
    graphs = []
    for i in range(distinct):
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x[i], edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    atoms, ptr, entries = ResidentMolecules.pack(graphs, m_dim=M, b_dim=E)
    times = -(-n // distinct)
    counts = np.tile(np.diff(ptr), times)[:n]
    full = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=full[1:])
    return ResidentMolecules.from_arrays(np.tile(atoms, (times, 1))[:n], full, np.tile(entries, times)[:full[-1]], M, E, "cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--event-reps", type=int, default=20)
    ap.add_argument("--store", type=int, default=100_000)
    ap.add_argument("--distinct", type=int, default=2_000)
    ap.add_argument("--chunk", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mol_fp_probe.py measures on the GPU: none found")
    reps = args.event_reps
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# mol_fp_probe on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}: E={E} M={M}, 1024 bits")
    say(f"# us per call between two HIP events around a captured chain of {reps} calls: min-max over {args.rounds} alternated rounds")
    say("#     B    N  bonds/mol  features/mol  bits/mol   KiB read  KiB written    dg_mol_canon    fp r=2 largest      fp r=2 whole      fp r=4 whole")
    tables = fingerprint.FingerprintTables.from_decoders(ATOM_DECODER, BOND_DECODER, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)
    for B, N in ((1024, 45), (64, 256)):
        cap = N * (N - 1) // 2
        node, edge = logits(*trees(B, N, gen))
        decoded = decode.decode_molecule_graphs(node, edge)
        del node, edge
        forms = canon.CanonicalForms.empty(B, N, cap, "cuda", "whole")
        outs = [fingerprint.CircularFingerprints.empty(B, 1024, "cuda") for _ in range(3)]
        chains = [chain_of(lambda: canon.canonical_forms(decoded, "whole", out=forms), reps),
                  chain_of(lambda: fingerprint.circular_fingerprints(decoded, tables, 2, 1024, "largest", out=outs[0]), reps),
                  chain_of(lambda: fingerprint.circular_fingerprints(decoded, tables, 2, 1024, "whole", out=outs[1]), reps),
                  chain_of(lambda: fingerprint.circular_fingerprints(decoded, tables, 4, 1024, "whole", out=outs[2]), reps)]
        spans = [[] for _ in chains]
        for r in range(args.rounds):
            for k in (range(len(chains)) if r % 2 == 0 else reversed(range(len(chains)))):
                spans[k].append(event_us(chains[k], reps))
        bonds = float(decoded.cpu().n_bonds.mean())
        fps = outs[1].cpu()
        read = B * (2 * N + 4 * bonds + 8) + 4 * len(ATOM_DECODER) + 8 * len(BOND_DECODER)
        written = B * (128 + 8)
        say(f"{B:7d} {N:4d} {bonds:10.1f} {float(fps.n_features.float().mean()):13.1f} {float(fps.counts.float().mean()):9.1f} "
            f"{read / 1024:10.1f} {written / 1024:12.1f}   " + "   ".join(f"{min(s):7.1f}-{max(s):<8.1f}" for s in spans))

    n, N = args.store, 45
    t0 = time.perf_counter()
    store = synthetic_store(n, min(args.distinct, n), N, seed=7)
    say(f"# store: {n} molecules of N = {N} ({min(args.distinct, n)} distinct synth molecules, repeated), "
        f"{int(store.ptr[-1])} directed bond entries, built in {time.perf_counter() - t0:.1f} s on the host")
    say(f"# fingerprint_store(store, tables, chunk={args.chunk}), radius 2, 1024 bits, scope largest: ms per call, host clock to a "
        "device synchronise, after one warm-up call")
    fingerprint.fingerprint_store(store, tables, chunk=args.chunk)
    torch.cuda.synchronize()
    spans = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        fps = fingerprint.fingerprint_store(store, tables, chunk=args.chunk)
        torch.cuda.synchronize()
        spans.append((time.perf_counter() - t0) * 1e3)
    host = fps.cpu()
    say(f"{n:9d} molecules  {min(spans):9.1f}-{max(spans):<9.1f} ms   {n / min(spans) / 1e3:7.2f} M molecules/s at best   "
        f"mean features {float(host.n_features.float().mean()):.1f}, no graph: {int((host.n_features < 0).sum())}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
