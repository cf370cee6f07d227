#!/usr/bin/env python
"""Step-level A/B of the hook ``options.embed_keep`` (edge embedding on kept signs, csrc/embed_sym_keep.hip) at bench.py's
headline workload (configs[1] shapes, bench.py's seeds), in ONE process: the hook alternates False / True, every run is
STEPS steps of the same GANStep, synchronised before and after.
    python scripts/embed_keep_ab.py [rounds=6] [steps=20] > profiles/embed_keep_ab.txt
The gain counts only if every alternation has the same sign and the mean difference exceeds twice the largest difference
between two runs of the same setting."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from druggen_amd import functional as dgf, synth  # noqa: E402
from druggen_amd.model import Discriminator, Generator  # noqa: E402
from druggen_amd.options import options  # noqa: E402
from druggen_amd.trainer import GANStep  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    overrides, B, dtype, text = bench.CONFIGS["c2"]
    w = dict(bench.WORKLOAD, **overrides)
    dgf.set_activation_dtype(dtype)
    dev = torch.device("cuda", 0)
    ctor = (w["act"], w["vertexes"], w["edges"], w["nodes"], w["dropout"])
    kw = dict(dim=w["dim"], depth=w["depth"], heads=w["heads"], mlp_ratio=w["mlp_ratio"])
    torch.manual_seed(0)
    G, D = Generator(*ctor, **kw).to(dev), Discriminator(*ctor, **kw).to(dev)
    a, x, _, _ = synth.molecule_batch(B, w["vertexes"], w["edges"], w["nodes"], seed=1234)
    da, dx, _, _ = synth.molecule_batch(B, w["vertexes"], w["edges"], w["nodes"], seed=2234)
    batch = [torch.from_numpy(t).to(dev) for t in (da, dx, a, x)]
    st = GANStep(G, D, lambda_gp=10.0)
    for keep in (False, True):      # warm-up of both paths
        options.embed_keep = keep
        for _ in range(3):
            st.step(*batch)
    print(f"# {text}; B={B}; {steps} steps per run; ms per step")
    print(f"# {'round':>5} {'keep=False':>11} {'keep=True':>11} {'diff':>8}")
    runs = {False: [], True: []}
    for r in range(rounds):
        for keep in (False, True):
            options.embed_keep = keep
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                st.step(*batch)
            torch.cuda.synchronize(dev)
            runs[keep].append((time.perf_counter() - t0) / steps * 1e3)
        print(f"  {r:5d} {runs[False][-1]:11.3f} {runs[True][-1]:11.3f} {runs[False][-1] - runs[True][-1]:8.3f}")
    diffs = [o - n for o, n in zip(runs[False], runs[True])]
    mean = sum(diffs) / len(diffs)
    spread = max(max(v) - min(v) for v in runs.values())
    same_sign = all(d > 0 for d in diffs) or all(d < 0 for d in diffs)
    print(f"# mean keep=False {sum(runs[False]) / rounds:.3f} ms, keep=True {sum(runs[True]) / rounds:.3f} ms, mean difference "
          f"{mean:.3f} ms; largest difference between two runs of one setting {spread:.3f} ms; same sign in every round: "
          f"{same_sign}; counts as a gain: {same_sign and mean > 2 * spread}")


if __name__ == "__main__":
    main()
