"""Gradient-penalty pattern of the edge embedding alone, for a smooth activation: the native route (dg_embed_sym_fwd,
dg_embed_sym_bwd, dg_embed_sym_bwd2_smooth) against the composite route (``_composite_embed_sym``: dgf.linear + torch
activations, what ``embed_sym`` took for sigmoid / tanh inside ``second_order_forward()`` before), alternated in one process.

    python scripts/embed_smooth_probe.py [B N E act rounds iters]        default 256 45 5 tanh 5 10

Pattern (reference loss.py:28-39 + train.py:367): forward under ``second_order_forward()``, ``autograd.grad(create_graph=True)``
with respect to ``a`` under ``inputs_only_backward()``, then the final backward of <t, da> to the parameters, the upstream
gradient and ``a`` (a leaf that requires a gradient, as the interpolated sample is).  Per side and output dtype: device-event
time per iteration over rounds x iters iterations after a warm-up, peak allocated memory above the resident inputs, and the
two routes' results against each other."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from druggen_amd import functional as dgf      # noqa: E402

args = sys.argv[1:]
B, N, E = (int(args[i]) if len(args) > i else d for i, d in enumerate((256, 45, 5)))
act = args[3] if len(args) > 3 else "tanh"
ROUNDS, ITERS = (int(args[i]) if len(args) > i else d for i, d in ((4, 5), (5, 10)))
if not torch.cuda.is_available():
    raise SystemExit("embed_smooth_probe: needs a GPU (timings are device events)")
dev = "cuda"
torch.manual_seed(0)
a = torch.softmax(2 * torch.randn(B, N, N, E, device=dev), -1).requires_grad_(True)
w1, b1 = (torch.randn(64, E, device=dev) * 0.5).requires_grad_(True), (torch.randn(64, device=dev) * 0.3).requires_grad_(True)
w2, b2 = (torch.randn(128, 64, device=dev) * 0.2).requires_grad_(True), (torch.randn(128, device=dev) * 0.3).requires_grad_(True)
t = torch.randn(B, N, N, E, device=dev)


def pattern(native, g):
    with dgf.second_order_forward():
        if native:
            out = dgf.embed_sym(a, w1, b1, w2, b2, act, g.dtype)
        else:
            out = dgf._composite_embed_sym(a, w1, b1, w2, b2, act).to(g.dtype)
    with dgf.inputs_only_backward():
        (da,) = torch.autograd.grad(out, a, g, create_graph=True)
    return torch.autograd.grad((da * t).sum(), [w1, b1, w2, b2, g, a])


def timed(native, g, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        pattern(native, g)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30))
print(f"# embed_smooth_probe B={B} N={N} E={E} act={act}: {ROUNDS} rounds x {ITERS} iterations per side, alternated; ms per iteration")
for odt in (torch.float32, torch.bfloat16):
    g = torch.randn(B, N, N, 128, device=dev).to(odt).requires_grad_(True)
    name = str(odt).split(".")[-1]
    res, peak = {}, {}
    for native in (True, False):      # warm-up, results, peak memory
        for _ in range(3):
            pattern(native, g)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res[native] = pattern(native, g)
        torch.cuda.synchronize()
        peak[native] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    print(f"# {name}: native vs composite, relative L2: "
          + "  ".join(f"{n} {rel(x, y):.2e}" for n, x, y in zip("gw1 gb1 gw2 gb2 gg ga".split(), res[True], res[False])))
    del res
    times = {True: [], False: []}
    print(f"# {name}  round   native   composite")
    for r in range(ROUNDS):
        for native in (True, False):
            times[native].append(timed(native, g, ITERS))
        print(f"  {name}  {r:5d} {times[True][-1]:8.3f}  {times[False][-1]:10.3f}")
    mn, mc = sum(times[True]) / ROUNDS, sum(times[False]) / ROUNDS
    spread = max(max(v) - min(v) for v in times.values())
    print(f"# {name}: native {mn:.3f} ms, composite {mc:.3f} ms, composite / native {mc / mn:.2f}x; largest spread between rounds of "
          f"one side {spread:.3f} ms; native faster in every round: {all(x < y for x, y in zip(times[True], times[False]))}")
    print(f"# {name}: peak allocated above the inputs: native {peak[True]:.0f} MiB, composite {peak[False]:.0f} MiB")
