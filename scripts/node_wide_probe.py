"""What the wide node kernels (csrc/node_wide.hip) return on a --features model (m_dim = 13 atom types + 54 descriptor columns).

    python scripts/node_wide_probe.py [--parent TREE] [--out profiles/node_wide_probe.txt]

(a) The gradient-penalty pattern of the node chain alone (reference loss.py:28-39 + train.py:367) at B = 256, N = 45, E = 67,
    relu: forward under ``second_order_forward()``, ``autograd.grad(create_graph=True)`` with respect to z under
    ``inputs_only_backward()``, then the final backward to the parameters, the upstream gradient and z.  The native route
    (``dgf.node_embed``: dg_embed_node_wide_chain / _bwd / _wgrad) against the composite route (dgf.linear twice + ATen
    activations: what models.py took at this width before), alternated in one process; device events.  Also at E = 17 and 255.
(b) One whole ``ResidentTrainer(graph=True)`` step on a synthetic feature store (atom_dim = 13, F = 54) at the launch-bound
    shape of DESIGN 3.21 (N = 9, L = 1, B = 32) and at BASELINE configs[1] (N = 45, L = 4, B = 256), for this tree and -- with
    ``--parent TREE``, a built checkout of the commit to compare against -- for that tree, in fresh child processes that
    alternate; host clock around ``reps`` replays to the end of a device synchronise.
Medians with [min-max] over the rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOM_DIM, F, E_BOND, DIM = 13, 54, 5, 128
BLOCKS = (5, 9, 6, 9, 1, 1, 5, 5, 5, 1, 7)      # the reference's descriptor blocks (dataset.py:161-185)
SHAPES = [("launch-bound (DESIGN 3.21)", 9, 1, 32, 40), ("BASELINE configs[1] + features", 45, 4, 256, 8)]      # name, N, L, B, reps


def cell(v):
    return f"{statistics.median(v):8.3f} [{min(v):.3f}-{max(v):.3f}]"


# ---------------------------------------------------------------------------------------------------------------- (a)
def chain_pattern(say, B, N, E, act, rounds, iters):
    import torch
    from druggen_amd import functional as dgf
    fn = {"relu": torch.relu}[act]
    torch.manual_seed(0)
    dev = "cuda"
    z = (torch.rand(B, N, E, device=dev) < 0.3).float().requires_grad_(True)
    l1, l2 = torch.nn.Linear(E, 64).to(dev), torch.nn.Linear(64, 128).to(dev)
    g = torch.randn(B, N, 128, device=dev, requires_grad=True)
    t = torch.randn(B, N, E, device=dev)

    def pattern(native):
        with dgf.second_order_forward():
            if native:
                out = dgf.node_embed(z, l1, l2, act)
            else:
                out = fn(dgf.linear(fn(dgf.linear(z, l1.weight, l1.bias)), l2.weight, l2.bias))
        with dgf.inputs_only_backward():
            (dz,) = torch.autograd.grad(out, z, g, create_graph=True)
        return torch.autograd.grad((dz * t).sum(), [l1.weight, l2.weight, g], allow_unused=True) + (out.detach(), dz.detach())

    def timed(native):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            pattern(native)
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / iters

    assert dgf.node_embed_supported(z, l1, l2, act)
    res = {}
    for native in (True, False):
        for _ in range(3):
            pattern(native)
        res[native] = pattern(native)
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30))
    agree = "  ".join(f"{n} {rel(x, y):.1e}" for n, x, y in zip("gw1 gw2 gg out dz".split(), res[True], res[False]))
    times = {True: [], False: []}
    for _ in range(rounds):
        for native in (True, False):
            times[native].append(timed(native))
    mn, mc = statistics.median(times[True]), statistics.median(times[False])
    say(f"  {B:4d} {N:3d} {E:4d} {act:>6s}   {cell(times[True]):>28s}   {cell(times[False]):>28s}   {mc / mn:6.2f}   {agree}")


# ---------------------------------------------------------------------------------------------------------------- (b)
def feature_graphs(n, N, seed):
    import numpy as np
    from types import SimpleNamespace
    from druggen_amd import synth
    _, x, bonds, _ = synth.molecule_batch(n, N, E_BOND, ATOM_DIM, seed=seed)
    rng = np.random.default_rng([n, N, seed])
    feats = np.zeros((n, N, F), dtype=np.float32)
    start = 0
    for width in BLOCKS:
        if width == 1:
            feats[..., start] = rng.integers(0, 2, size=(n, N))
        else:
            np.put_along_axis(feats[..., start:start + width], rng.integers(0, width, size=(n, N, 1)), 1.0, axis=-1)
        start += width
    x = np.concatenate([x.astype(np.float32), feats], axis=-1)
    graphs = []
    for i in range(n):
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x[i], edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    return graphs


def child(tree, shape, rounds, stock):
    """One tree, one shape: the round times of a graphed ResidentTrainer step as a JSON line."""
    sys.path.insert(0, tree)
    import itertools
    import torch
    import druggen_amd
    assert os.path.dirname(os.path.abspath(druggen_amd.__file__)) == os.path.join(os.path.abspath(tree), "druggen_amd")
    from druggen_amd import synth
    from druggen_amd.loop import ResidentTrainer
    from druggen_amd.model import Discriminator, Generator
    from druggen_amd.resident import ResidentMolecules
    from druggen_amd.trainer import GANStep
    _, N, L, B, reps = SHAPES[shape]
    M = ATOM_DIM + F
    nets = []
    for cls, seed in ((Generator, 11), (Discriminator, 12)):
        net = cls("relu", N, E_BOND, M, 0.0, dim=DIM, depth=L, heads=8, mlp_ratio=3)
        params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=seed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        nets.append(net.cuda())
    mols = ResidentMolecules.from_graphs(feature_graphs(stock, N, 7), device="cuda", b_dim=E_BOND, atom_dim=ATOM_DIM)
    drugs = ResidentMolecules.from_graphs(feature_graphs(stock, N, 8), device="cuda", b_dim=E_BOND, atom_dim=ATOM_DIM)
    trainer = ResidentTrainer(GANStep(*nets), mols, drugs, batch_size=B, seed=11, graph=True)
    schedule = itertools.chain.from_iterable(trainer.schedule() for _ in itertools.count())

    def clock(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            trainer.step(*next(schedule))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    clock(3)
    times = [clock(reps) for _ in range(rounds)]
    for store in (mols, drugs):
        store.raise_bad_indices(wait=True)
    finite = bool(torch.isfinite(torch.stack(trainer.graphed.losses)).all())
    print("RESULT " + json.dumps({"times": times, "finite": finite}), flush=True)


def whole_step(say, trees, rounds, passes, stock):
    for i, (name, N, L, B, reps) in enumerate(SHAPES):
        times = {k: [] for k in trees}
        finite = True
        for _ in range(passes):
            for k, tree in trees.items():      # a fresh process per tree and pass, one after the other
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--shape", str(i), "--rounds",
                                      str(rounds), "--stock", str(stock)], capture_output=True, text=True, timeout=600)
                line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
                if out.returncode != 0 or not line:
                    raise SystemExit(f"node_wide_probe: child for {k} failed ({out.returncode}):\n{out.stderr[-2000:]}")
                got = json.loads(line[0][7:])
                times[k] += got["times"]
                finite = finite and got["finite"]
        cells = "   ".join(f"{k} {cell(v)}" for k, v in times.items())
        ratio = (f"   parent / this {statistics.median(times['parent']) / statistics.median(times['this']):5.3f}"
                 if "parent" in times else "")
        say(f"  {name:<32s} N={N:2d} L={L} B={B:3d}  {passes} x {rounds} rounds x {reps} steps   {cells}{ratio}"
            + ("" if finite else "   LOSSES NOT FINITE"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the commit to compare (b) against")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--stock", type=int, default=512)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shape", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.shape, args.rounds, args.stock)
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("node_wide_probe.py measures on the GPU: none found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# node_wide_probe on {torch.cuda.get_device_name(0)}")
    say(f"# (a) penalty pattern of the node chain alone; ms per iteration, median [min-max] over {args.rounds} alternated rounds x "
        f"{args.iters} iterations, device events")
    say("#     B   N    E    act                       native                      composite   comp / native   native vs composite, relative L2")
    for E in (67, 17, 255):
        chain_pattern(say, 256, 45, E, "relu", args.rounds, args.iters)
    chain_pattern(say, 32, 9, 67, "relu", args.rounds, args.iters)
    trees = {"this": HERE}
    if args.parent:
        trees = {"parent": os.path.abspath(args.parent), "this": HERE}
    say(f"# (b) ResidentTrainer(graph=True) step on a synthetic feature store (atom_dim {ATOM_DIM}, F {F}, {args.stock} + {args.stock} "
        "molecules); ms per step, median [min-max], host clock to the end of a device synchronise; one fresh process per tree and pass")
    whole_step(say, trees, args.rounds, args.passes, args.stock)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
