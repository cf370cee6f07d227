#!/usr/bin/env python
"""Headline benchmark: molecules/sec of one full WGAN-GP iteration.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is the reference's inner loop body (train.py:351-384): reset_grad ->
discriminator_loss -> backward -> AdamW(D) -> reset_grad -> generator_loss ->
backward -> AdamW(G), on synthetic molecule graphs already resident in HBM.
Workload = BASELINE.json configs[1]: DrugGEN default (dim 128, 8 heads, 4 layers,
mlp_ratio 3), N=45 atoms, E=5 bond classes, M=13 atom classes, batch 256 per GPU,
fp32.  Multi-GPU: one process per GPU, the batch is sharded (weak scaling: 256
molecules per rank), gradients averaged with one RCCL all-reduce per backward.

Rank 0 prints ONE JSON line of < 6 KB.  Besides the contract fields it carries
  roofline      the time-dominant edge-level kernel of the step (chosen by
                measurement: one instrumented step before the timed region ranks
                them): algorithmic bytes / HIP-event time measured during the timed
                steps, against the 8 TB/s HBM3E peak (+ its MFMA-side fraction, its
                kernel symbol, and the same rate against the section-8d FLOOR bytes:
                inputs + outputs only, nothing saved for a backward);
  roofline_attention  the same for the attention kernel north_star names.
A plain run does only that: set up, warm up, the instrumented step, the timed steps, the dump, the line.
`--full` adds everything measured beside the headline, after the timed steps:
  step_hbm, kernels, roofline_all  two more fully instrumented steps; the per-kernel table
                (`kernels`, `roofline_all`) goes to profiles/bench_detail_<config>_<dtype>.json, not to stdout;
  hip_graph_replay_same_step, strict_f32_hidden  the same steps replayed from a captured hipGraph, and
                with the feed-forward's hidden tensors in plain float32;
  bf16_configs2 BASELINE configs[2] (bf16 activations, batch 2048) in the same process;
  cpu_baseline  the oracle (CPU restatement of the reference path) timed on the
                host cores on a bounded sample of the same workload;
  parity_margin the committed golden-parity margin of the hidden-storage mode;
  replicas_identical  N > 1: per-tensor checksums of G and D compared across ranks (also with --check-replicas).
`--dump-outputs DIR` writes what the last timed step returned (both losses, the updated G and D
parameters) as DIR/<name>.npy, so that two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3   # same guide: fp32-input MFMA (v_mfma_f32_32x32x2_f32), dense
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA
WORKLOAD = dict(act="relu", vertexes=45, edges=5, nodes=13, dropout=0.0, dim=128, depth=4, heads=8, mlp_ratio=3)
# BASELINE.json configs -> (workload overrides, batch per GPU, activation dtype, description)
CONFIGS = {
    "c2": (dict(), 256, "f32", "BASELINE configs[1]: DrugGEN default 4-layer/8-head dim128 mlp_ratio3, N=45, E=5, M=13, fp32"),
    "c3": (dict(), 2048, "bf16", "BASELINE configs[2]: same model, bf16 activations (MFMA QKV/FFN path), batch 2048"),
    "c4": (dict(), 2048, "f32", "BASELINE configs[3]: DrugGEN default, batch 2048 per GPU (data parallel over the node's GPUs)"),
    "c5": (dict(vertexes=90, edges=10, depth=8), 64, "f32",
           "BASELINE configs[4]: deep variant, 8-layer encoder, N=90, E=10, global batch 512 = 64 per GPU on 8 GPUs"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c2",
                    help="BASELINE.json configuration (c2 = configs[1] is the headline the metric is quoted on)")
    ap.add_argument("--batch", type=int, default=0, help="molecules per GPU (0 = the configuration's)")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default=None,
                    help="storage of the encoder activations (default: the configuration's)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what lies beside the headline: the per-kernel table, "
                         "the hipGraph-replay and strict-float32 regions, the bf16 configs[2] line, the CPU baseline, the "
                         "parity margin and (N > 1) the cross-rank replica comparison")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--check-replicas", action="store_true",
                    help="N > 1: compare the per-tensor checksums of G and D across ranks after the timed steps (as --full "
                         "does, reported as replicas_identical) and exit non-zero when they differ")
    ap.add_argument("--graph", action="store_true", help="time hipGraph replays only and skip the eagerly launched, event-instrumented "
                    "region (one graph per step on one GPU; N > 1: three graphs per step, cut at the two gradient all-reduces)")
    ap.add_argument("--eager", action="store_true",
                    help="--full: skip the secondary hipGraph-replay and strict-float32 regions")
    ap.add_argument("--vertexes", type=int, default=0, help="override N (parity-case shapes; not the headline)")
    ap.add_argument("--depth", type=int, default=0, help="override L")
    ap.add_argument("--no-extra", action="store_true",
                    help="--full: skip the secondary measurement (BASELINE configs[2]: bf16 activations, batch 2048) that "
                         "a single-GPU run appends as `bf16_configs2` after the timed region")
    ap.add_argument("--cpu-batch", type=int, default=32)
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = the reference's own setting (train.py:16: 5 threads)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned to its caller -- both losses and the "
                         "updated G and D parameters -- as DIR/<name>.npy (rank 0; float32, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_BUDGET_BYTES = 64 << 20


def snapshot_outputs(losses, G, D):
    """Host copies of what a timed step hands its caller: the two losses and every parameter of G and D after the step's
    AdamW updates (float32 / float64 as computed)."""
    def host(t):
        t = t.detach()
        return t.to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()
    outs = {"d_loss": host(losses[0]), "g_loss": host(losses[1])}
    for tag, net in (("G", G), ("D", D)):
        for name, p in net.named_parameters():
            outs[f"{tag}.{name}"] = host(p)
    return outs


def dump_outputs(outs, out_dir, budget=DUMP_BUDGET_BYTES):
    """Write every array as out_dir/<name>.npy.  Over the byte budget, each array is cut to a fixed, seeded sample of its
    flattened elements (sorted indices; the same for every run and build) sized to its share of the budget."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    header = 128      # bytes of a .npy header (format 1.0, padded to a multiple of 64; 128 for these shapes)
    fixed = sum(header + (v.nbytes if v.size <= 1 else 0) for v in outs.values())
    total = sum(v.nbytes for v in outs.values() if v.size > 1)
    room = budget - fixed
    for name, v in outs.items():
        if fixed + total > budget and v.size > 1:
            keep = max(1, v.size * room // total)
            idx = np.sort(np.random.default_rng(0).choice(v.size, size=keep, replace=False))
            v = v.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), v)


def _cpu_gan_step_rate(workload, batch, threads, steps=5, budget_s=60.0):
    """molecules/s of the oracle's GAN step (torch CPU restatement of src/model + train.py:351-384): MEDIAN step time of
    `steps` steps after one warm-up (fewer only if `budget_s` runs out; at least one)."""
    from oracle import druggen_oracle as orc
    from druggen_amd import synth
    cfg = orc.NetConfig(**workload)
    torch.manual_seed(0)
    G = orc.OracleNet("G", cfg, {k: torch.from_numpy(v) for k, v in
                                 synth.fill_parameters(orc.generator_schema(cfg), 1, 1.0).items()})
    D = orc.OracleNet("D", cfg, {k: torch.from_numpy(v) for k, v in
                                 synth.fill_parameters(orc.discriminator_schema(cfg), 2, 1.0).items()})
    g_opt, d_opt = orc.make_optimizers(G, D)
    a, x, _, _ = synth.molecule_batch(batch, cfg.vertexes, cfg.edges, cfg.nodes, seed=1234)
    da, dx, _, _ = synth.molecule_batch(batch, cfg.vertexes, cfg.edges, cfg.nodes, seed=2234)
    ee, en = synth.interpolation_eps(batch, 1234)
    t = lambda v: torch.from_numpy(v)
    args = (t(da), t(dx), t(a), t(x), 10.0, t(ee), t(en))
    torch.set_num_threads(threads)
    orc.gan_step(G, D, g_opt, d_opt, *args)          # warm-up
    times, t_all = [], time.perf_counter()
    while len(times) < steps and (not times or time.perf_counter() - t_all < budget_s):
        t0 = time.perf_counter()
        orc.gan_step(G, D, g_opt, d_opt, *args)
        times.append(time.perf_counter() - t0)
    times.sort()
    return batch / times[len(times) // 2], len(times)


def cpu_baseline(workload, batch: int, threads: int = 0):
    """The CPU path timed beside the GPU number (SURVEY.md section 8d / BASELINE.md section 3): the oracle's GAN
    step on the host cores with (i) the reference's own thread setting (train.py:16 `torch.set_num_threads(5)`)
    and (ii) all physical cores, at the bench workload's shape (reduced batch: a bounded sample) and at
    BASELINE configs[0] (N=9, L=1, B=32, the reference's CPU-runnable case)."""
    logical = os.cpu_count() or 1
    physical = max(1, logical // 2)
    c1 = dict(WORKLOAD, vertexes=9, nodes=5, depth=1)
    ref_threads = threads or min(5, logical)
    variants = []
    for name, wl, b, thr, n, budget in (("bench", workload, batch, ref_threads, 5, 60.0),
                                        ("bench", workload, batch, min(physical, 64), 5, 90.0),
                                        ("c1", c1, 32, ref_threads, 5, 10.0),
                                        ("c1", c1, 32, min(physical, 64), 5, 10.0)):
        rate, steps = _cpu_gan_step_rate(wl, b, thr, n, budget)
        variants.append({"workload": name, "batch": b, "threads": thr, "value": rate, "steps": steps,
                         "statistic": "median step time"})
    head = variants[0]
    return {"value": head["value"], "unit": "molecules/s", "cores": head["threads"], "kind": "port",
            "sample": f"oracle GAN step (torch CPU restatement of src/model + train.py:351-384) at the bench workload's "
                      f"shape, batch {head['batch']}, median of {head['steps']} steps after 1 warm-up, {head['threads']} "
                      f"threads (train.py:16) of {logical} logical cores",
            # [workload, batch, threads, molecules/s, steps]; c1 = BASELINE configs[0] (N=9, L=1)
            "variants": [[v["workload"], v["batch"], v["threads"], round(v["value"], 2), v["steps"]] for v in variants],
            "logical_cores": logical}


def parity_margin(mode):
    """Worst per-tensor gradient error of the shipped hidden-storage mode on the reference goldens, read from the committed
    table (profiles/r06_parity_by_hidden_storage.txt, scripts/parity_report.py on an MI355X); None when the table has no row
    for the mode."""
    path = os.path.join(ROOT, "profiles", "r06_parity_by_hidden_storage.txt")
    try:
        worst, inside = None, False
        for ln in open(path):
            if ln.startswith("== "):
                inside = ln.strip() == f"== DG_HIDDEN={mode}"
            elif inside and ln.strip().startswith("golden "):
                parts = ln.split()
                e, name = float(parts[2]), parts[1]
                if worst is None or e > worst[0]:
                    worst = (e, name, parts[3] if len(parts) > 3 else "")
        if worst is None:
            return None
        return {"worst_golden_tensor_error": worst[0], "golden": worst[1], "tensor": worst[2], "bar": 1e-3,
                "hidden_storage": mode, "source": "profiles/r06_parity_by_hidden_storage.txt"}
    except OSError:
        return None


def secondary_bf16_line(dev, G, D, synth, dgf, GANStep, w, batch=2048, steps=4, warmup=2):
    """BASELINE configs[2] beside the headline: the same model with bf16 activations at batch 2048, measured in the same
    process AFTER the headline's timed region (same timing discipline: synchronize, K steps, synchronize).  Not part of
    `value`; `python bench.py --config c3` is the full-length version of this line."""
    torch.cuda.empty_cache()
    a, x, _, _ = synth.molecule_batch(batch, w["vertexes"], w["edges"], w["nodes"], seed=4321)
    da, dx, _, _ = synth.molecule_batch(batch, w["vertexes"], w["edges"], w["nodes"], seed=5321)
    ge, gn = torch.from_numpy(a).to(dev), torch.from_numpy(x).to(dev)
    de, dn = torch.from_numpy(da).to(dev), torch.from_numpy(dx).to(dev)
    prev = dgf.activation_dtype()
    dgf.set_activation_dtype("bf16")
    try:
        st = GANStep(G, D, lambda_gp=10.0)
        for _ in range(warmup):
            st.step(de, dn, ge, gn)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            losses = st.step(de, dn, ge, gn)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        ok = all(bool(torch.isfinite(v)) for v in losses)
    finally:
        dgf.set_activation_dtype(prev)
    return {"value": batch * steps / dt, "unit": "molecules/s", "ms_per_step": 1e3 * dt / steps, "steps": steps,
            "warmup": warmup, "dtype": "bf16", "batch_per_gpu": batch, "finite_losses": ok,
            "config": "BASELINE configs[2]: same model, bf16 activations in HBM, batch 2048, 1 GPU (a 1-2 % gradient-error "
                      "configuration, README: never the headline)"}


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: druggen_amd has no CPU path")
    ndev = torch.cuda.device_count()
    backend = os.environ.get("DG_DIST_BACKEND", "nccl")     # "gloo": functional test of the N>1 path on one GPU
    dev_index = local_rank % ndev if backend != "nccl" else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    if args.gpus != world:
        # the driver's scaling run launches `torchrun --nproc-per-node N bench.py --gpus N`: a mismatch means the
        # launcher did not start N ranks, and an N=1 measurement must not be recorded as an N-GPU number
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with "
                         f"`python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} ... bench.py --gpus {args.gpus}`")

    from druggen_amd import _lib, functional as dgf, synth
    from druggen_amd.model import Discriminator, Generator
    from druggen_amd.trainer import GANStep, GraphedGANStep, broadcast_parameters

    overrides, cfg_batch, cfg_dtype, cfg_text = CONFIGS[args.config]
    w = dict(WORKLOAD, **overrides)
    act_dtype = args.dtype or cfg_dtype
    dgf.set_activation_dtype(act_dtype)
    if args.vertexes:
        w["vertexes"] = args.vertexes
    if args.depth:
        w["depth"] = args.depth
    ctor = (w["act"], w["vertexes"], w["edges"], w["nodes"], w["dropout"])
    kw = dict(dim=w["dim"], depth=w["depth"], heads=w["heads"], mlp_ratio=w["mlp_ratio"])
    torch.manual_seed(0)                       # PyTorch default init, on CPU, then moved
    G, D = Generator(*ctor, **kw).to(dev), Discriminator(*ctor, **kw).to(dev)
    broadcast_parameters(G)
    broadcast_parameters(D)
    B = args.batch or cfg_batch
    a, x, _, _ = synth.molecule_batch(B, w["vertexes"], w["edges"], w["nodes"], seed=1234 + rank)
    da, dx, _, _ = synth.molecule_batch(B, w["vertexes"], w["edges"], w["nodes"], seed=2234 + rank)
    gen_edge, gen_node = torch.from_numpy(a).to(dev), torch.from_numpy(x).to(dev)
    disc_edge, disc_node = torch.from_numpy(da).to(dev), torch.from_numpy(dx).to(dev)
    stepper = GANStep(G, D, lambda_gp=10.0)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    losses = None
    for _ in range(args.warmup):
        losses = stepper.step(disc_edge, disc_node, gen_edge, gen_node)
    run = lambda: stepper.step(disc_edge, disc_node, gen_edge, gen_node)
    if args.graph:      # one graph on one GPU; three graphs cut at the two all-reduces under torch.distributed.run
        graphed = GraphedGANStep(stepper, disc_edge, disc_node, gen_edge, gen_node, warmup=1)
        run = graphed.step
    # Which edge-level kernel (and shape) is the time-dominant one is MEASURED, not assumed: one fully instrumented,
    # untimed step after the warm-up ranks every edge-level key by its total HIP-event time ...
    edge_keys = ("attn_fwd", "attn_bwd", "attn_bwd2", "attn_half_fwd", "attn_half_bwd", "row_gemm_e128",
                 "row_gemm_e_n384", "row_gemm_e_k384", "linear_wgrad_e128", "linear_wgrad_e_n384", "linear_wgrad_e_k384",
                 "ffn", "ffn_wgrad", "ffn_f32")
    # the attention kernel north_star names (scores + adjacency-modulated softmax + AV fused): the fused attention half
    # where the shape has one (bf16: N <= 48 since round 3; float32: N <= 48 since round 4, N <= 96 since round 5), else the attention core
    from druggen_amd.options import options as dg_options
    fused_half = ((act_dtype == "bf16" and dgf.attn_half_supported(torch.bfloat16, w["vertexes"], w["dim"])
                   and dg_options.attn_half != "unfused") or
                  (act_dtype == "f32" and w["vertexes"] <= (48 if dg_options.attn_half_f32 == "n48" else 96)
                   and w["dim"] == 128 and dg_options.attn_half_f32 != "off"))
    attn_key = "attn_half_fwd" if fused_half else "attn_fwd"
    top_key = None
    if not args.graph:
        _lib.prof_reset()
        _lib.prof_enable(kernels=edge_keys)
        stepper.step(disc_edge, disc_node, gen_edge, gen_node)
        torch.cuda.synchronize(dev)
        _lib.prof_enable(False)
        ranked = sorted(((_lib.prof_read(k)[1], k) for k in edge_keys), reverse=True)
        top_key = ranked[0][1] if ranked and ranked[0][0] > 0 else None
    _lib.prof_reset()
    dgf.traffic_reset()
    # ... and the timed region carries HIP events only around that kernel plus the attention kernel north_star names
    # (~50 of the ~1.1 k launches of a step: every pair of events costs a few microseconds of stream time)
    attn_kernels = tuple(dict.fromkeys(k for k in (top_key, attn_key) if k))
    if not args.graph:
        _lib.prof_enable(kernels=attn_kernels)
    if world > 1:
        stepper.time_collectives(True)      # HIP events around the two gradient all-reduces of every step
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses = run()
    sync()
    elapsed = time.perf_counter() - t0
    _lib.prof_enable(False)
    # the last timed step's results, taken before the untimed steps below move the parameters again
    dumped = snapshot_outputs(losses, G, D) if args.dump_outputs and rank == 0 else None
    n_ar, ms_ar = stepper.collective_ms() if world > 1 else (0, 0.0)      # the timed steps' all-reduces only
    stepper.time_collectives(False)
    attn_stats = {k: (_lib.prof_read(k), dgf.traffic_bytes(k), dgf.traffic_floor_bytes(k)) for k in attn_kernels}
    traffic_flops = {k: dgf.traffic_flops(k) for k in attn_kernels}
    # ---- everything below up to the result line, bar the N > 1 timing, runs with --full only
    # per-kernel table of every HIP kernel: two extra, untimed, fully instrumented steps
    detail_steps, detail_elapsed, detail_traffic = 2, None, {}
    if args.full:
        _lib.prof_reset()
        dgf.traffic_reset()
        _lib.prof_enable(True)
        t1 = time.perf_counter()
        for _ in range(detail_steps):
            stepper.step(disc_edge, disc_node, gen_edge, gen_node)
        sync()
        detail_elapsed = time.perf_counter() - t1
        _lib.prof_enable(False)
        # (functional._account keeps counting bytes whenever a step is traced in Python: read the two instrumented steps'
        # totals before the graph region below warms up and captures)
        detail_traffic = {name: (dgf.traffic_bytes(name), dgf.traffic_floor_bytes(name), dgf.traffic_flops(name))
                          for name in _lib.KERNEL_IDS}
    # ---- secondary regions at the headline, reported BESIDE `value` (which is always the eagerly launched region above):
    # (1) the same K steps replayed from a captured hipGraph (trainer.GraphedGANStep; N > 1: three graphs per step cut at the two
    # gradient all-reduces).  A step is ~700 launches issued from Python, 30-40 ms of host work against ~50 ms of GPU work at
    # configs[1]: on a box with a slow host the replay is the faster mode, on a fast one the eager stream is (a replayed kernel
    # node costs ~2 us of dependency handling).  Round 5 reported the faster of the two as `value`; a best-of-two biases the
    # metric upward, so the definition is fixed now: eager launches, always.  The roofline blocks come from that region too (HIP
    # events cannot be timed inside a replayed graph: hipEventElapsedTime -> hipErrorInvalidHandle).
    # (2) `strict_f32_hidden`: the same steps with the feed-forward's [R,384] hidden tensors in plain float32 (hidden storage
    # "f32": no fp16 plane for dh, no fused forward) -- the number the default mode's precision trade is measured against.
    graph_region = None
    want_graph = (args.full and not args.graph and not args.eager and args.config == "c2" and act_dtype == "f32"
                  and not stepper._low_memory(gen_edge))
    if want_graph:
        graphed, err = None, None
        try:      # (the capture issues no collective: a rank that fails here cannot leave the others waiting)
            graphed = GraphedGANStep(stepper, disc_edge, disc_node, gen_edge, gen_node, warmup=1)
            # other tensor objects than the captured ones: every step copies its batch (and the one-hot labels, validated once
            # per tensor object during the warm-up) into the graph's static buffers
            batch2 = [t.clone() for t in (disc_edge, disc_node, gen_edge, gen_node)]
        except Exception as exc:      # a failed capture must not cost the line: the eager region is the value then
            graphed, err = None, repr(exc)[:200]
        ok = torch.tensor([0 if graphed is None else 1], device=dev, dtype=torch.int32)
        if world > 1:      # every rank replays, or none does
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            for _ in range(max(1, args.warmup)):
                glosses = graphed.step(*batch2)
            sync()
            tg = time.perf_counter()
            # (N > 1: a bounded secondary region -- the three-graph replay has never run over RCCL on several devices, and the
            # record must not wait minutes for a region that is not `value`)
            graph_steps = args.steps if world == 1 else min(args.steps, 10)
            for _ in range(graph_steps):
                glosses = graphed.step(*batch2)
            sync()
            tg = time.perf_counter() - tg
            if all(bool(torch.isfinite(v)) for v in glosses):
                graph_region = {"elapsed": tg, "steps": graph_steps, "losses": [float(v.item()) for v in glosses]}
            else:
                graph_region = {"error": "non-finite losses in the replayed region"}
        else:
            graph_region = {"error": err or "the capture failed on another rank"}
        graphed = batch2 = None
    strict = None
    if want_graph and world == 1 and dgf.hidden_storage() != "f32":
        prev_mode = dgf.hidden_storage()
        dgf.set_hidden_storage("f32")
        try:
            k = min(args.steps, 30)
            for _ in range(2):
                stepper.step(disc_edge, disc_node, gen_edge, gen_node)
            sync()
            ts = time.perf_counter()
            for _ in range(k):
                sl = stepper.step(disc_edge, disc_node, gen_edge, gen_node)
            sync()
            ts = time.perf_counter() - ts
            strict = {"value": B * k / ts, "unit": "molecules/s", "ms_per_step": 1e3 * ts / k, "steps": k,
                      "what": "the same eager steps with the feed-forward's [R,384] hidden tensors in plain float32 (hidden "
                              "storage f32: no fp16 plane for dh, two-launch forward)",
                      "finite_losses": all(bool(torch.isfinite(v)) for v in sl)}
        finally:
            dgf.set_hidden_storage(prev_mode)
    if world > 1:
        both = [elapsed, graph_region["elapsed"] if graph_region and "elapsed" in graph_region else 0.0]
        t = torch.tensor(both, device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)      # the slowest rank's time of each region
        elapsed = float(t[0].item())
        if graph_region and "elapsed" in graph_region:
            graph_region["elapsed"] = float(t[1].item())
    replicas_identical = None
    allreduce = None
    if world > 1:
        # what an N-GPU line needs to explain itself: the time between the events around the two all-reduces of a step
        # on every rank (includes waiting for the slowest rank)
        mine = torch.tensor([ms_ar / max(1, args.steps)], device=dev, dtype=torch.float64)
        gathered = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        per_rank = [float(g.item()) for g in gathered]
        allreduce = {"per_rank_ms_per_step": per_rank, "max_ms_per_step": max(per_rank), "collectives_per_step": n_ar / max(1, args.steps),
                     "backend": backend, "what": "HIP events around the D- and G-gradient flat-bucket all-reduces (6.3 + 4.9 MB fp32) of "
                                                 "every timed step" + ("; gloo: host-side copy time, not a device collective" if backend != "nccl" else "")}
    if world > 1 and (args.full or args.check_replicas):      # whether the replicas still hold identical weights
        sums = torch.stack([p.detach().double().sum() for p in list(G.parameters()) + list(D.parameters())] +
                           [p.detach().double().abs().sum() for p in list(G.parameters()) + list(D.parameters())])
        lo, hi = sums.clone(), sums.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        replicas_identical = bool(torch.equal(lo, hi))
        if not replicas_identical and args.check_replicas:
            raise SystemExit("bench.py --check-replicas: parameters differ across ranks after the timed steps")
    d_loss, g_loss = (float(v.item()) for v in losses)
    if not (d_loss == d_loss and g_loss == g_loss):
        raise SystemExit(f"non-finite losses d={d_loss} g={g_loss}")

    if rank == 0:
        bf16 = act_dtype == "bf16"
        # MFMA ceiling of the GEMM-shaped kernels by arithmetic: fp32 activations run a power-of-two scaled fp16
        # two-plane split in the row GEMMs AND the weight gradients (3 fp16 MFMAs per product: ceiling = 16-bit peak / 3);
        # bf16 activations one MFMA per product
        gemm_peak = MFMA_BF16_PEAK_TFLOPS if bf16 else MFMA_BF16_PEAK_TFLOPS / 3.0
        gemm_how = ("1x v_mfma_f32_*_bf16 per product (bf16 operands, fp32 accumulate)" if bf16 else
                    "3x v_mfma_f32_16x16x32_f16 per product (fp32 operands scaled by a power of two and split hi + lo "
                    "into fp16, fp32 accumulate: fp32-class accuracy, tests/test_hip_kernels.py)")

        def mfma_how(name):
            if name.startswith("linear_wgrad") and not bf16:
                return ("3x v_mfma_f32_16x16x32_f16 per product (fp32 operands split hi + lo into fp16 under running "
                        "power-of-two column scales, fp32 accumulate)")
            return gemm_how

        kernels = {}
        step_bytes = step_floor = 0.0
        for name in (_lib.KERNEL_IDS if args.full else ()):      # the two instrumented steps' table
            n, ms = _lib.prof_read(name)
            nbytes, floor, _ = detail_traffic[name]
            step_bytes += float(nbytes)
            step_floor += float(floor)
            if n:
                gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
                kernels[name] = {"launches_per_step": n / detail_steps, "avg_us": 1e3 * ms / n,
                                 "algorithmic_MB_per_launch": nbytes / n / 1e6, "floor_MB_per_launch": floor / n / 1e6,
                                 "achieved_GBps": gbs, "frac_of_hbm_peak": gbs / HBM_PEAK_GBS,
                                 "frac_of_floor": (floor / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if ms > 0 else 0.0,
                                 "share_of_step": ms * 1e-3 / detail_elapsed}
                fl = detail_traffic[name][2]
                if fl:          # GEMM-shaped kernels: flop rate against the MFMA ceiling of their arithmetic
                    tf = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
                    peak = gemm_peak
                    kernels[name].update({"achieved_TFLOPs": tf, "mfma_peak_TFLOPs": peak,
                                          "frac_of_mfma_peak": tf / peak, "mfma": mfma_how(name)})
                    kernels[name]["bound"] = "hbm" if kernels[name]["frac_of_hbm_peak"] >= tf / peak else "mfma"
                else:
                    kernels[name]["bound"] = "hbm"
        # ---- roofline blocks, measured INSIDE the timed region (HIP events on the launch stream)
        SHAPES = {"row_gemm_e128": "row GEMM 128->128 (+bias / residual / LayerNorm epilogues), edge-level launches",
                  "row_gemm_e_n384": "row GEMM 128->384 (fc1 + ReLU; dh = dz W2), edge-level launches",
                  "row_gemm_e_k384": "row GEMM 384->128 (fc2 + residual + LayerNorm; dx = dh W1), edge-level launches",
                  "attn_fwd": "attention core forward", "attn_bwd": "attention core backward",
                  "attn_bwd2": "attention core second order", "attn_half_fwd": "fused attention half forward "
                  "(e-proj + score/softmax/AV + out_e + residual + LN4)", "attn_half_bwd": "fused attention half backward",
                  "linear_wgrad_e128": "weight gradient dW[128,128] = dy^T x over the edge rows",
                  "linear_wgrad_e_n384": "weight gradient dW[384,128] (fc1) over the edge rows",
                  "linear_wgrad_e_k384": "weight gradient dW[128,384] (fc2) over the edge rows",
                  "ffn_f32": "fused float32 feed-forward forward (fc1 + ReLU + fc2 + residual + LayerNorm, hidden tensor on chip), edge-level launches",
                  "ffn": "fused bf16 feed-forward (forward, dx), edge-level launches",
                  "ffn_wgrad": "fused bf16 feed-forward weight gradients, edge-level launches"}

        # kernel symbols as rocprofv3 --kernel-trace prints them (profiles/*_kernel_stats.txt)
        SYMBOLS = {"row_gemm_e128": "dg::row_gemm_h3_kernel<1,1,...> (plain / +LayerNorm / LayerNorm-backward variants)"
                                    if not bf16 else "dg::row_gemm_bf16_kernel<1,1>",
                   "row_gemm_e_n384": "dg::row_gemm_n384_kernel" if not bf16 else "dg::row_gemm_bf16_kernel<1,3>",
                   "row_gemm_e_k384": "dg::row_gemm_k384_kernel<*>" if not bf16 else "dg::row_gemm_bf16_kernel<3,1>",
                   "attn_fwd": "dg::attn_fwd_kernel", "attn_bwd": "dg::attn_bwd_kernel", "attn_bwd2": "dg::attn_bwd2_kernel",
                   "attn_half_fwd": "dg::attn_half_fwd_kernel (bf16)" if bf16 else "dg::attn_half_f32_fwd_kernel",
                   "attn_half_bwd": "dg::attn_half_bwd_kernel (bf16)" if bf16 else "dg::attn_half_f32_bwd1_kernel",
                   "linear_wgrad_e128": "dg::wgrad_stream_kernel<4,4,*>" if not bf16 else "dg::wgrad_kernel<bf16,...>",
                   "linear_wgrad_e_n384": "dg::wgrad_stream_kernel<12,4,*>" if not bf16 else "dg::wgrad_kernel<bf16,...>",
                   "linear_wgrad_e_k384": "dg::wgrad_stream_kernel<4,12,*>" if not bf16 else "dg::wgrad_kernel<bf16,...>",
                   "ffn_f32": "dg::ffn_fused_f32_kernel<KEEP>",
                   "ffn": "dg::ffn_fwd_bf16_v2_kernel / dg::ffn_bwd_dx_bf16_kernel",
                   "ffn_wgrad": "dg::ffn_bwd_dw2_bf16_kernel / dg::ffn_bwd_dw1_bf16_kernel"}

        def timed_block(name):
            (n, ms), nbytes, floor = attn_stats[name]
            if not n or ms <= 0:
                return None
            gbs = floor / (ms * 1e-3) / 1e9
            # `achieved` / `frac` = the launch's ALGORITHMIC bytes -- its inputs + outputs only, nothing it writes for a
            # backward pass (bytes_floor_per_launch) -- over its average HIP-event duration; what the launch is asked to move
            # including the tensors it saves (moved_bytes_per_launch) is reported beside it as frac_of_moved
            blk = {"kernel": name, "kernel_symbol": SYMBOLS.get(name, name), "what": SHAPES[name], "bound": "hbm",
                   "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "launches_timed": n,
                   "avg_us": 1e3 * ms / n, "bytes_floor_per_launch": floor / n,
                   "moved_bytes_per_launch": nbytes / n, "frac_of_moved": nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                   "share_of_step": ms * 1e-3 / elapsed}
            fl = traffic_flops.get(name, 0)
            if fl:      # GEMM-shaped: the MFMA side from the SAME events; the block reports the roof the kernel is closer to
                tf = fl / (ms * 1e-3) / 1e12
                peak = gemm_peak
                blk.update({"frac_of_mfma_peak": tf / peak, "mfma_peak_TFLOPs": peak, "achieved_TFLOPs": tf,
                            "mfma": mfma_how(name)})
                if tf / peak > blk["frac"]:
                    blk.update({"bound": "mfma", "frac_of_hbm_floor": blk["frac"], "achieved_GBps_of_floor": blk["achieved"],
                                "achieved": tf, "peak": peak, "unit": "TFLOP/s", "frac": tf / peak})
            return blk

        blocks = [b for b in (timed_block(k) for k in attn_kernels) if b]
        # every edge-level kernel from the two extra instrumented steps (not the timed region)
        all_blocks = [dict(kernel=k, kernel_symbol=SYMBOLS.get(k, k), what=SHAPES.get(k, k), bound="hbm",
                           achieved=v["frac_of_floor"] * HBM_PEAK_GBS, peak=HBM_PEAK_GBS, unit="GB/s", frac=v["frac_of_floor"],
                           launches_timed=None, avg_us=v["avg_us"], bytes_floor_per_launch=v["floor_MB_per_launch"] * 1e6,
                           moved_bytes_per_launch=v["algorithmic_MB_per_launch"] * 1e6, frac_of_moved=v["frac_of_hbm_peak"],
                           share_of_step=v["share_of_step"], measured="instrumented steps after the timed region")
                      for k, v in kernels.items() if k in SHAPES]
        if args.graph or not blocks:        # --graph: events cannot sit inside a replayed graph (without --full: no block)
            blocks = all_blocks
        # the block of the kernel the pre-pass ranked first; the instrumented steps after the timed region rank again
        top_all = max(all_blocks, key=lambda b: b["share_of_step"])["kernel"] if all_blocks else None
        dominant = next((b for b in blocks if b["kernel"] == top_key), None) or (
            max(blocks, key=lambda b: b["share_of_step"]) if blocks else {})
        if dominant and top_all is not None:
            dominant["is_time_dominant_edge_kernel"] = bool(top_all == dominant["kernel"])
        if dominant:
            dominant["chosen_by"] = "largest total HIP-event time among the edge-level profiler keys in one instrumented step before the timed region"
        attention = next((b for b in blocks if b["kernel"] == attn_key), None)
        # HBM bytes per launch from PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in their own runs,
        # scripts/pmc_traffic.py): only reported when the pass was taken on THIS workload, dtype and batch; the record
        # names the commit it was measured at
        side = os.path.join(ROOT, "profiles", "traffic.json")
        traffic_rec = {}
        if os.path.exists(side):
            try:
                for rec in json.load(open(side)).get("records", []):
                    if rec.get("config") == args.config and rec.get("dtype") == act_dtype and rec.get("batch") == B:
                        traffic_rec = rec
            except Exception:
                traffic_rec = {}
        for blk in blocks + [b for b in all_blocks if b not in blocks]:
            t = traffic_rec.get("kernels", {}).get(blk["kernel"])
            blk["traffic"] = None if not t else t["bytes_per_launch"]
            blk["traffic_commit"] = None if not t else traffic_rec.get("commit")
        captured = bool(graph_region and "elapsed" in graph_region)
        replayed = False      # `value` is the eager region, always (--graph: the replayed steps ARE the timed region above)
        timed = elapsed
        out = {
            "metric": "molecules/sec GAN step (G+D fwd+bwd), N=45 graphs" if w["vertexes"] == 45 else
                      f"molecules/sec GAN step (G+D fwd+bwd), N={w['vertexes']} graphs",
            "value": B * world * args.steps / timed,
            "unit": "molecules/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * timed / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": act_dtype, "data": "synthetic",
            "config": {"workload": cfg_text + "; full WGAN-GP step (train.py:351-384) incl. gradient penalty + 2x AdamW",
                       "baseline_config": args.config,
                       "batch_per_gpu": B, "global_batch": B * world, "parallelism": f"dp{world}",
                       "vertexes": w["vertexes"], "edges": w["edges"], "depth": w["depth"],
                       "hip_graph_replay": bool(args.graph or replayed),
                       "gemm_arithmetic": gemm_how,
                       "hidden_storage": dgf.hidden_storage(), "feed_forward_forward": dg_options.ffn_f32,
                       "activations": "bf16 in HBM; fp32 parameters, optimizer state, weight gradients, softmax and "
                                      "LayerNorm statistics" if bf16 else "fp32"},
            # the time-dominant kernel AND shape of the step (largest share of the timed region among the edge-level
            # kernels), then the attention kernel north_star names
            "roofline": dominant or None,
            "roofline_attention": attention,
            "losses": {"d_loss": d_loss, "g_loss": g_loss},
            "replicas_identical": replicas_identical,
            "allreduce": allreduce,
            "peak_memory_GB": torch.cuda.max_memory_allocated(dev) / 1e9,
            "step_memory_mode": (("low (D terms differentiated one at a time; " +
                                  ("one generator forward for both steps)" if stepper._low_memory_shares_generator(gen_edge)
                                   else "the generator runs once per step)"))
                                 if stepper._low_memory(gen_edge) else "fast"),
        }
        if args.full:
            # the whole step against the HBM roof: algorithmic bytes of every HIP kernel launch of a step (the per-kernel
            # formulas of DESIGN.md section 3, accumulated by functional._account) / wall time of two fully instrumented
            # steps after the timed region
            out["step_hbm"] = {"algorithmic_GB_per_step": step_bytes / detail_steps / 1e9,
                               "floor_GB_per_step": step_floor / detail_steps / 1e9,
                               "achieved_GBps": step_bytes / detail_elapsed / 1e9,
                               "frac_of_hbm_peak": step_bytes / detail_elapsed / 1e9 / HBM_PEAK_GBS}
        detail = {"kernels": kernels, "roofline_all": all_blocks}
        if captured:
            # two regions of exactly K steps each, `value` = the faster launch mode on this box: K steps launched eagerly (HIP
            # events around the roofline kernels), then K steps replayed from the captured hipGraph, every step copying its batch
            # into the graph's static buffers
            tg = graph_region["elapsed"]
            how = ("hipGraph replay of the whole step (trainer.GraphedGANStep)" if world == 1 else
                   "three hipGraphs per step, cut at the two gradient all-reduces (trainer.GraphedGANStep under the process group)")
            out["timed_region"] = ("eager launches (`value`, `roofline*`); hip_graph_replay_same_step = the same steps (K; at most 10 for N > 1) as " + how +
                                   ", the batch copied into the static buffers every step (secondary, never `value`)")
            gk = graph_region["steps"]
            out["hip_graph_replay_same_step"] = {"value": B * world * gk / tg, "unit": "molecules/s", "ms_per_step": 1e3 * tg / gk,
                                                 "steps": gk, "losses": graph_region["losses"]}
        elif graph_region:
            out["timed_region"] = "eager launches (the hipGraph capture failed: see hip_graph_replay_same_step)"
            out["hip_graph_replay_same_step"] = graph_region
        else:
            out["timed_region"] = (("hipGraph replay (--graph)" if world == 1 else
                                    "three hipGraphs per step, cut at the two gradient all-reduces (--graph)") if args.graph
                                   else "eager launches")
        if strict is not None:
            out["strict_f32_hidden"] = strict
        if args.full:
            out["parity_margin"] = parity_margin(dgf.hidden_storage() if not bf16 else "bf16")
        if args.full and world == 1 and args.config == "c2" and act_dtype == "f32" and not args.no_extra and not args.graph:
            out["bf16_configs2"] = secondary_bf16_line(dev, G, D, synth, dgf, GANStep, w)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(w, args.cpu_batch, args.cpu_threads)
        if args.full:
            # per-kernel detail: a file in profiles/, not stdout (round 4's 21 KB line could not be parsed by the driver)
            detail.update({k: out[k] for k in ("metric", "value", "ms_per_step", "dtype", "config")})
            name = f"bench_detail_{args.config}_{act_dtype}" + ("" if B == cfg_batch else f"_b{B}") + ".json"
            out["detail_file"] = None
            try:
                with open(os.path.join(ROOT, "profiles", name), "w") as f:
                    json.dump(detail, f, indent=1)
                out["detail_file"] = os.path.join("profiles", name)
            except OSError:
                pass
        if dumped is not None:
            dump_outputs(dumped, args.dump_outputs)

        def rnd(v):      # 6 significant digits: the line must stay under 6 KB
            if isinstance(v, float):
                return float(f"{v:.6g}")
            if isinstance(v, dict):
                return {k: rnd(x) for k, x in v.items()}
            if isinstance(v, (list, tuple)):
                return [rnd(x) for x in v]
            return v
        line = json.dumps(rnd(out), separators=(",", ":"))
        if len(line) >= 6144:      # never again an unparseable record: drop the optional blocks, largest first
            for k in ("cpu_baseline", "bf16_configs2", "roofline_attention", "step_hbm"):
                slim = dict(out)
                slim[k] = {kk: vv for kk, vv in out[k].items() if kk in ("value", "unit", "cores", "kind", "frac", "kernel")} if isinstance(out.get(k), dict) else out.get(k)
                out = slim
                line = json.dumps(rnd(out), separators=(",", ":"))
                if len(line) < 6144:
                    break
        print(line, flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
