#!/usr/bin/env python
"""What watching every step costs: ms per training step with the step monitor off and on, alternated in one process, eager and
captured, at the headline shape (BASELINE configs[1]: B = 256, N = 45, L = 4; E = 5, M = 13, dim 128, float32), and the two
launches' own HIP-event times.

  eager    one GANStep, `set_monitor(None)` / `set_monitor(monitor)` between the timed windows;
  graphed  three GraphedGANStep captures of twin networks: without, with, and without the monitor again.
Each step figure is the median over rounds, with the min-max spread, of a host clock around `reps` steps that ends in a device
synchronise.  The decode (`dg_decode_graph`) and the statistics (`dg_mol_stats`: three kernels) are timed alone between two HIP
events around a captured chain of `--event-reps` back-to-back calls, on normal random logits (a random label per pair: 4 / 5 of
the pairs are bonds) and on the same logits with label 0 raised on 95 % of the pairs (the sparse, trained-model regime of
tests/test_hip_decode_graph.py).  Rounds alternate the order of the routes, so that neither setting always follows the other.

    python scripts/monitor_probe.py [--out profiles/monitor_probe.txt] [--rounds 7] [--budget 420]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from druggen_amd import decode, monitor, synth
from druggen_amd.functional import as_one_hot, one_hot_labels
from druggen_amd.model import Discriminator, Generator
from druggen_amd.trainer import GANStep, GraphedGANStep

E, M, DIM = 5, 13, 128
ORDER2 = (0, 2, 4, 6, 3)
TABLE = (0xFFFF, 8, 6, 4, 2, 8, 6, 4, 2, 8, 6, 4, 2)


def networks(N, L):
    nets = []
    for cls, seed in ((Generator, 11), (Discriminator, 12)):
        net = cls("relu", N, E, M, 0.0, dim=DIM, depth=L, heads=8, mlp_ratio=3)
        params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=seed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        nets.append(net.cuda())
    return nets


def batch(B, N, seed):
    a, x, _, _ = synth.molecule_batch(B, N, E, M, seed=seed)
    return as_one_hot(torch.from_numpy(a).cuda()), torch.from_numpy(x).cuda()


def clock(step, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def chain_of(fn, reps):
    """`reps` back-to-back calls of `fn` as one captured chain: the span between two events around a replay is device time,
    not the host's launch rate."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    return graph


def event_us(graph, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def cell(values, fmt="{:.3f}"):
    return f"{fmt.format(statistics.median(values))} [{fmt.format(min(values))}-{fmt.format(max(values))}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--event-reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--vertexes", type=int, default=45)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--budget", type=float, default=420.0, help="seconds: no new round is started after this long")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("monitor_probe.py measures on the GPU: none found")
    started = time.perf_counter()
    B, N, L = args.batch, args.vertexes, args.depth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# monitor_probe on {torch.cuda.get_device_name(0)}: B={B} N={N} L={L} E={E} M={M} dim={DIM} float32, synthetic batches")
    say(f"# ms per step: median [min-max] over alternated rounds of a host clock around {args.reps} steps to the end of a device synchronise")
    real, gen = batch(B, N, 21), batch(B, N, 22)

    def mon():
        return monitor.StepMonitor(bond_order2=ORDER2, max_valence2=TABLE)

    # ---- eager: one stepper, the monitor attached and detached ----
    G, D = networks(N, L)
    eager, eager_mon = GANStep(G, D), mon()

    def eager_route(m):
        def run():
            eager.set_monitor(m)
            eager.step(*real, *gen)
        return run
    # ---- graphed: twin networks, captured without, with, and without again (two captures of ONE setting differ by where
    # their pools landed: the second "off" shows by how much) ----
    graphed_mon = mon()
    captures = []
    for m in (None, graphed_mon, None):
        Gk, Dk = networks(N, L)
        captures.append(GraphedGANStep(GANStep(Gk, Dk, monitor=m), *real, *gen))
    routes = {"eager off": eager_route(None), "eager on": eager_route(eager_mon), "graphed off": captures[0].replay,
              "graphed on": captures[1].replay, "graphed off, second capture": captures[2].replay}
    for fn in routes.values():
        clock(fn, 2)
    times = {k: [] for k in routes}
    for r in range(args.rounds):
        if time.perf_counter() - started > args.budget:
            break
        order = list(routes.items())
        for k, fn in (order if r % 2 == 0 else order[::-1]):      # off/on, then on/off: neither always follows the other
            times[k].append(clock(fn, args.reps))
    say(f"# route          rounds   monitor off ms/step            monitor on ms/step             on - off (medians)")
    for kind in ("eager", "graphed"):
        off, on = times[f"{kind} off"], times[f"{kind} on"]
        if not off:
            say(f"{kind:<14s} not measured: the time budget of {args.budget:.0f} s ran out")
            continue
        say(f"{kind:<14s} {len(off):6d}   {cell(off):>28s}   {cell(on):>28s}   {statistics.median(on) - statistics.median(off):+8.3f} ms")
    if times["graphed off, second capture"]:
        again = times["graphed off, second capture"]
        say(f"graphed, a second capture with the monitor off: {cell(again)} ms/step, "
            f"{statistics.median(again) - statistics.median(times['graphed off']):+.3f} ms against the first")
    for m, name in ((eager_mon, "eager"), (graphed_mon, "graphed")):
        s = m.stats.cpu()
        say(f"# last {name} step: " + ", ".join(f"{k}={s.total(k)}" for k in monitor.TOT_FIELDS[:13]))

    # ---- the two launches alone ----
    say(f"# the two launches alone, us per call between two HIP events around a captured chain of {args.event_reps} calls: median [min-max] over rounds")
    say("# logits                       B   bonds / molecule   duplicates   dg_decode_graph us         dg_mol_stats us")
    for Bk in sorted({B, 2048}):
        g = torch.Generator(device="cuda").manual_seed(5)
        ns = torch.randn(Bk, N, M, device="cuda", generator=g)
        es = torch.randn(Bk, N, N, E, device="cuda", generator=g)
        ns[Bk // 2:], es[Bk // 2:] = ns[:Bk - Bk // 2], es[:Bk - Bk // 2]      # the second half repeats the first: verified matches
        sparse = es.clone()
        sparse[..., 0] += torch.where(torch.rand(Bk, N, N, device="cuda", generator=g) < 0.95, 20.0, 0.0)
        in_atoms = torch.randint(0, M, (Bk, N), device="cuda", generator=g).to(torch.uint8)
        in_labels = (torch.randint(0, E, (Bk, N, N), device="cuda", generator=g) *
                     (torch.rand(Bk, N, N, device="cuda", generator=g) < 0.05)).to(torch.int32)
        for name, edge in (("normal (dense)", es), ("label 0 on 95 % (sparse)", sparse)):
            decoded = decode.MoleculeBatch.empty(Bk, N, N * (N - 1) // 2, True, "cuda")
            stats = monitor.MolStats.empty(Bk, N, "cuda")
            chains = (chain_of(lambda: decode.decode_molecule_graphs(ns, edge, bond_order2=ORDER2, out=decoded), args.event_reps),
                      chain_of(lambda: monitor.molecule_statistics(decoded, in_atoms=in_atoms, in_labels=in_labels,
                                                                   max_valence2=TABLE, out=stats), args.event_reps))
            dec, cnt = [], []
            for _ in range(max(args.rounds, 3)):      # alternated
                dec.append(event_us(chains[0], args.event_reps))
                cnt.append(event_us(chains[1], args.event_reps))
            host = stats.cpu()
            say(f"{name:<24s} {Bk:7d} {host.total('n_bonds') / Bk:12.1f} {Bk - host.total('n_distinct'):12d}   "
                f"{cell(dec, '{:.1f}'):>24s}   {cell(cnt, '{:.1f}'):>24s}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
