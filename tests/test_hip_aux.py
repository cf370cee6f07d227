"""GPU parity of the kernels either side of the hot path (densify, AdamW, argmax
decode) and of the reference-format checkpoint helpers."""
import numpy as np
import pytest
import torch

from oracle import aux_oracle as aux

pytestmark = pytest.mark.gpu


def _coo_batch(B, N, E, seed):
    """Padded PyG-style batch from the synthetic molecule generator."""
    from druggen_amd import synth
    a, x, bonds, atoms = synth.molecule_batch(B, N, E, 7, seed=seed)
    src, dst, attr = [], [], []
    for b in range(B):
        i, j = np.nonzero(bonds[b])
        src.append(b * N + i); dst.append(b * N + j); attr.append(bonds[b][i, j])
    edge_index = np.stack([np.concatenate(src), np.concatenate(dst)])
    return edge_index, np.concatenate(attr), x.reshape(B * N, -1), np.repeat(np.arange(B), N), a, x


@pytest.mark.parametrize("B,N,E", [(3, 6, 4), (32, 9, 5), (256, 45, 5), (1, 90, 10), (3, 97, 5), (2, 256, 5)])
def test_densify_matches_to_dense_adj_plus_onehot(B, N, E):
    from druggen_amd import data

    class Batch:      # the four attributes load_molecules touches on a PyG Batch
        pass
    ei, ea, x, batch, a_want, x_want = _coo_batch(B, N, E, seed=B + N)
    d = Batch()
    d.edge_index, d.edge_attr = torch.from_numpy(ei).cuda(), torch.from_numpy(ea).cuda()
    d.x, d.batch = torch.from_numpy(x).cuda(), torch.from_numpy(batch).cuda()
    graphs, a, xt = data.load_molecules(data=d, b_dim=E, m_dim=7, device=None, batch_size=B)
    g_ref, a_ref, x_ref = aux.load_molecules(ei, ea, x, batch, B, E)
    assert np.array_equal(a_ref, a_want)                       # the oracle reproduces the generator's graphs
    assert np.array_equal(a.cpu().numpy(), a_ref)              # bit-exact one-hot
    assert np.array_equal(xt.cpu().numpy(), x_ref) and np.array_equal(graphs.cpu().numpy(), g_ref)


def test_densify_reproduces_pyg_docstring_examples():
    """dg_densify on the vectors of PyG's own to_dense_adj docstring (tests/test_host.py: PYG_*; batches padded to N = 2 nodes
    per graph are the ones the loader produces): the dense labels, incl. the edge that leaves its graph, then one-hot."""
    from druggen_amd import data
    import test_host as th
    ei = torch.tensor(th.PYG_EDGE_INDEX, device="cuda")
    for attr, want in ((torch.ones(5, dtype=torch.long), th.PYG_DENSE), (torch.tensor(th.PYG_EDGE_ATTR), th.PYG_DENSE_ATTR)):
        a = data.dense_one_hot_adjacency(ei, attr.cuda(), 2, 2, 6)
        assert a.shape == (2, 2, 2, 6) and bool((a.sum(-1) == 1).all())
        assert a.argmax(-1).cpu().tolist() == want
        from druggen_amd.functional import one_hot_labels
        assert one_hot_labels(a).cpu().tolist() == want      # the labels the loader attaches for the table-gather embedding


def test_densify_edge_cases():
    from druggen_amd import data
    # no edges at all -> every entry is class 0
    ei = torch.zeros(2, 0, dtype=torch.long, device="cuda")
    ea = torch.zeros(0, dtype=torch.long, device="cuda")
    a = data.dense_one_hot_adjacency(ei, ea, 2, 4, 3)
    assert a.shape == (2, 4, 4, 3) and bool((a[..., 0] == 1).all()) and float(a.sum()) == 2 * 16
    # duplicate edges are ADDED by to_dense_adj (1 + 1 = label 2); out-of-range sums are reported
    ei = torch.tensor([[0, 0, 5], [1, 1, 6]], device="cuda")
    ea = torch.tensor([1, 1, 2], device="cuda")
    a = data.dense_one_hot_adjacency(ei, ea, 2, 4, 3)
    ref = aux.label2onehot(aux.to_dense_adj(ei.cpu().numpy(), np.repeat(np.arange(2), 4), ea.cpu().numpy(), 4), 3)
    assert np.array_equal(a.cpu().numpy(), ref)
    with pytest.raises(RuntimeError, match="outside"):
        data.dense_one_hot_adjacency(ei, torch.tensor([2, 2, 2], device="cuda"), 2, 4, 3, check=True)
    # an edge that leaves its graph (node 1 of graph 0 -> node 2 of graph 1): to_dense_adj indexes
    # (batch[src], src - ptr, dst - ptr[batch[dst]]) -> graph 0, row 1, column 2; node ids outside the batch are ignored
    ei = torch.tensor([[1, 2, 7, 99], [6, 3, 0, 1]], device="cuda")
    ea = torch.tensor([2, 1, 1, 1], device="cuda")
    a = data.dense_one_hot_adjacency(ei, ea, 2, 4, 3)
    ref = aux.label2onehot(aux.to_dense_adj(ei.cpu().numpy()[:, :3], np.repeat(np.arange(2), 4), ea.cpu().numpy()[:3], 4), 3)
    assert np.array_equal(a.cpu().numpy(), ref) and a[0, 1, 2, 2] == 1 and a[1, 3, 0, 1] == 1


def test_densify_deferred_check_never_syncs_and_raises_later():
    """check="deferred": the labels are attached without a device->host read (out-of-range labels are clamped to a valid class
    on the device, so the table gather stays memory-safe) and the error surfaces at a LATER call, once the counter's kernel
    has finished."""
    from druggen_amd import data, functional as dgf
    data.raise_deferred_checks(wait=True)
    ei = torch.tensor([[0, 0, 5], [1, 1, 6]], device="cuda")
    good = data.dense_one_hot_adjacency(ei, torch.tensor([1, 1, 2], device="cuda"), 2, 4, 3, check="deferred")
    assert dgf.one_hot_labels(good) is not None
    assert torch.equal(good, data.dense_one_hot_adjacency(ei, torch.tensor([1, 1, 2], device="cuda"), 2, 4, 3))
    bad = data.dense_one_hot_adjacency(ei, torch.tensor([2, 2, 2], device="cuda"), 2, 4, 3, check="deferred")      # 2 + 2 = label 4
    lab = dgf.one_hot_labels(bad)
    assert lab is not None and int(lab.max()) <= 2 and int(lab.min()) >= 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="EARLIER batch"):
        data.dense_one_hot_adjacency(ei, torch.tensor([1, 1, 2], device="cuda"), 2, 4, 3, check="deferred")
    data.raise_deferred_checks(wait=True)      # the queue is clean again
    # the polling must not read the counter on the compute stream (a .item() there waits for everything queued before
    # it, i.e. the previous training step).  With ~0.1 s of work queued in front, a deferred densify AND a poll return while
    # that work is still running.
    attr = torch.tensor([1, 1, 2], device="cuda")      # (made BEFORE the queued work: a host -> device copy of a list synchronises)
    torch.cuda.synchronize()
    torch.cuda._sleep(int(4e8))
    marker = torch.cuda.Event()
    marker.record()
    assert not marker.query()                          # the device is busy for a while
    data.dense_one_hot_adjacency(ei, attr, 2, 4, 3, check="deferred")
    data.raise_deferred_checks()
    assert not marker.query(), "the deferred check synchronised with the compute stream"
    torch.cuda.synchronize()
    data.raise_deferred_checks(wait=True)


def test_loader_attaches_labels_and_the_model_takes_the_table_path_without_a_sync():
    """data.dense_one_hot_adjacency hands its int32 labels to the model: Generator / Discriminator then embed the batch
    by table gather with NO validation pass (as_one_hot synced once per new tensor, i.e. every step with a
    real DataLoader)."""
    from druggen_amd import data, functional as dgf
    ei, ea, x, batch, a_want, x_want = _coo_batch(4, 9, 5, seed=3)
    a = data.dense_one_hot_adjacency(torch.from_numpy(ei).cuda(), torch.from_numpy(ea).cuda(), 4, 9, 5)
    lab = dgf.one_hot_labels(a)
    assert lab is not None and lab.dtype == torch.int32 and torch.equal(lab.long(), a.argmax(-1))
    calls = []
    real_argmax = torch.Tensor.argmax
    try:
        torch.Tensor.argmax = lambda self, *a_, **k_: (calls.append(1), real_argmax(self, *a_, **k_))[1]
        assert dgf.as_one_hot(a) is a and not calls                 # trusted labels: no re-validation
        dgf.as_one_hot(a.clone())
        assert calls                                                # unknown origin: validated (one sync)
    finally:
        torch.Tensor.argmax = real_argmax
    a.mul_(1.0)                                                     # an in-place write invalidates the declaration
    assert dgf.one_hot_labels(a) is None
    with pytest.raises(ValueError):
        dgf.attach_one_hot_labels(a, lab.long())


def test_flat_adamw_matches_torch_and_oracle_and_skips_dead_parameters():
    from druggen_amd.optim import FlatAdamW
    torch.manual_seed(0)
    shapes = [(128, 128), (128,), (384, 128), (5,), (7, 3)]
    ps = [torch.nn.Parameter(torch.randn(*s, device="cuda")) for s in shapes]
    dead = torch.nn.Parameter(torch.randn(9, device="cuda"))
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    dead0 = dead.detach().clone()
    mine = FlatAdamW(ps + [dead], lr=1e-3)
    theirs = torch.optim.AdamW(ref, lr=1e-3, betas=(0.9, 0.999))
    p_np = [p.detach().double().cpu().numpy() for p in ps]
    m_np = [np.zeros_like(v) for v in p_np]
    v_np = [np.zeros_like(v) for v in p_np]
    for step in range(1, 4):
        grads = [torch.randn_like(p) for p in ps]
        for p, r, g in zip(ps, ref, grads):
            p.grad, r.grad = g.clone(), g.clone()
        mine.step()
        theirs.step()
        for k, g in enumerate(grads):
            p_np[k], m_np[k], v_np[k] = aux.adamw_step(p_np[k], g.double().cpu().numpy(), m_np[k], v_np[k], step, 1e-3)
        for p, r, q in zip(ps, ref, p_np):
            assert torch.allclose(p, r, rtol=1e-6, atol=1e-7)
            assert np.allclose(p.detach().cpu().numpy(), q, rtol=1e-5, atol=1e-6)
    assert torch.equal(dead, dead0) and dead.grad is None       # never touched, not even weight decay
    assert all(p.data_ptr() >= mine.flat_param.data_ptr() for p in ps)


@pytest.mark.parametrize("B,N", [(64, 45), (2, 256)])
def test_argmax_decode_matches_torch_max(B, N):
    from druggen_amd import decode
    g = torch.Generator(device="cuda").manual_seed(0)
    node = torch.randn(B, N, 13, device="cuda", generator=g)
    edge = torch.randn(B, N, N, 5, device="cuda", generator=g)
    edge[0, 0, 0] = 1.0                                          # ties -> first maximum
    # ties on the last row and the last column of the last molecule: every class, and two late classes above the rest
    edge[-1, -1, :, :] = 0.5
    edge[-1, :, -1, :] = 0.5
    edge[-1, -1, : N // 2, 2:5:2] = 3.0
    edge[-1, : N // 2, -1, 3:5] = 3.0
    node[-1, -1, :] = 0.25
    node[-1, -2, 7:13:5] = 9.0
    n_lab, e_lab = decode.decode_molecule_labels(node, edge)
    assert n_lab.dtype == torch.uint8 and e_lab.shape == (B, N, N)
    assert int(n_lab[-1, -1]) == 0 and int(n_lab[-1, -2]) == 7
    assert (e_lab[-1, -1, : N // 2] == 2).all() and (e_lab[-1, -1, N // 2:] == 0).all()
    assert (e_lab[-1, : N // 2, -1] == 3).all() and (e_lab[-1, N // 2:, -1] == 0).all()
    assert np.array_equal(n_lab.cpu().numpy(), aux.argmax_last(node.cpu().numpy()))
    assert np.array_equal(e_lab.cpu().numpy(), aux.argmax_last(edge.cpu().numpy()))
    assert torch.equal(e_lab.long(), torch.max(edge, -1)[1])


def test_trainer_with_flat_adamw_matches_torch_adamw():
    """GANStep(optimizer='flat') == GANStep(optimizer='torch') after two iterations."""
    import cases
    import harness
    from druggen_amd.model import Discriminator, Generator
    from druggen_amd.trainer import GANStep
    case = cases.CASES["tiny_relu"]
    cfg = cases.net_config(case)
    gp, dp = cases.build_params(case)
    inp = harness.torch_inputs(case, torch.float32, "cuda")
    results = []
    for kind in ("flat", "torch"):
        args = (cfg.act, cfg.vertexes, cfg.edges, cfg.nodes, cfg.dropout)
        kw = dict(dim=cfg.dim, depth=cfg.depth, heads=cfg.heads, mlp_ratio=cfg.mlp_ratio)
        G, D = Generator(*args, **kw), Discriminator(*args, **kw)
        G.load_state_dict({k: torch.from_numpy(v) for k, v in gp.items()})
        D.load_state_dict({k: torch.from_numpy(v) for k, v in dp.items()})
        G, D = G.cuda(), D.cuda()
        st = GANStep(G, D, lambda_gp=case["lambda_gp"], optimizer=kind)
        for _ in range(2):
            st.step(inp["disc_edge"], inp["disc_node"], inp["gen_edge"], inp["gen_node"],
                    eps=(inp["eps_edge"], inp["eps_node"]))
        results.append([p.detach().clone() for p in list(G.parameters()) + list(D.parameters())])
    for a, b in zip(*results):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)


def test_shared_generator_forward_is_exact():
    """One G forward serving both the D step and the G step (possible because G is only updated at
    the end of the iteration) gives bit-identical parameters to running it twice like the reference."""
    import cases
    import harness
    from druggen_amd.model import Discriminator, Generator
    from druggen_amd.trainer import GANStep
    case = cases.CASES["tiny_leaky"]
    cfg = cases.net_config(case)
    gp, dp = cases.build_params(case)
    inp = harness.torch_inputs(case, torch.float32, "cuda")
    results = []
    for share in (True, False):
        args = (cfg.act, cfg.vertexes, cfg.edges, cfg.nodes, cfg.dropout)
        kw = dict(dim=cfg.dim, depth=cfg.depth, heads=cfg.heads, mlp_ratio=cfg.mlp_ratio)
        G, D = Generator(*args, **kw), Discriminator(*args, **kw)
        G.load_state_dict({k: torch.from_numpy(v) for k, v in gp.items()})
        D.load_state_dict({k: torch.from_numpy(v) for k, v in dp.items()})
        G, D = G.cuda(), D.cuda()
        st = GANStep(G, D, lambda_gp=case["lambda_gp"], share_generator_forward=share)
        for _ in range(2):
            losses = st.step(inp["disc_edge"], inp["disc_node"], inp["gen_edge"], inp["gen_node"],
                             eps=(inp["eps_edge"], inp["eps_node"]))
        results.append([p.detach().clone() for p in list(G.parameters()) + list(D.parameters())] + list(losses))
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_graphed_step_equals_eager_step():
    """Replaying the captured iteration gives the same parameters as running it eagerly."""
    import cases
    import harness
    from druggen_amd.model import Discriminator, Generator, discriminator_loss
    from druggen_amd.trainer import GANStep, GraphedGANStep
    case = cases.CASES["c1_b4"]
    cfg = cases.net_config(case)
    gp, dp = cases.build_params(case)
    inp = harness.torch_inputs(case, torch.float32, "cuda")
    eps = (inp["eps_edge"], inp["eps_node"])
    fixed_eps = lambda *a, **k: discriminator_loss(*a, **{**k, "eps": eps})   # deterministic eps in both
    outs = []
    for graphed in (False, True):
        args = (cfg.act, cfg.vertexes, cfg.edges, cfg.nodes, cfg.dropout)
        kw = dict(dim=cfg.dim, depth=cfg.depth, heads=cfg.heads, mlp_ratio=cfg.mlp_ratio)
        G, D = Generator(*args, **kw), Discriminator(*args, **kw)
        G.load_state_dict({k: torch.from_numpy(v) for k, v in gp.items()})
        D.load_state_dict({k: torch.from_numpy(v) for k, v in dp.items()})
        G, D = G.cuda(), D.cuda()
        st = GANStep(G, D, lambda_gp=case["lambda_gp"], d_loss_fn=fixed_eps, share_generator_forward=False)
        batch = (inp["disc_edge"], inp["disc_node"], inp["gen_edge"], inp["gen_node"])
        if graphed:
            gs = GraphedGANStep(st, *batch, warmup=2)       # 2 warm-up + 1 captured(not run) ...
            for _ in range(2):
                gs.step(*batch)
        else:
            for _ in range(4):
                st.step(*batch)
        torch.cuda.synchronize()
        outs.append([p.detach().clone() for p in list(G.parameters()) + list(D.parameters())])
    # 4 AdamW steps of size lr = 1e-5: a first-step Adam update is ~ lr * sign(g), so an element whose
    # gradient is rounding noise may differ by a few lr between two runs that pick different BLAS
    # kernels (capture vs eager); everything else must agree to rounding.
    worst, mean = 0.0, 0.0
    for a, b in zip(*outs):
        d = (a - b).abs()
        worst, mean = max(worst, d.max().item()), mean + d.mean().item() / len(outs[0])
    assert worst <= 8.5e-5 and mean <= 2e-6, (worst, mean)


def test_smiles_to_device_batch_end_to_end():
    """Real molecules (the reference's result SMILES) -> druggen_amd.smiles -> collate ->
    load_molecules (dg_densify on the GPU) reproduce the dense one-hot batches the real-graph golden
    case was generated from, bit for bit."""
    import os
    import cases
    from druggen_amd import smiles as sm
    from druggen_amd.data import load_molecules
    case = cases.CASES["chembl_b4"]
    (a, x), (da, dx) = cases.smiles_batches(case)
    rows = [ln.strip().split(",") for ln in open(os.path.join(os.path.dirname(cases.__file__), "chembl_like_smiles.csv"))
            if ln.strip() and not ln.startswith("#")][1:]
    for role, want_a, want_x in (("mol", a, x), ("drug", da, dx)):
        graphs = [sm.molecule_graph(r[2], cases.CHEMBL_ATOM_ENCODER, cases.CHEMBL_BOND_ENCODER, 45)
                  for r in rows if r[0] == role]
        real, a_t, x_t = load_molecules(data=sm.collate(graphs), b_dim=5, m_dim=9, device="cuda", batch_size=4)
        assert torch.equal(a_t.cpu(), torch.from_numpy(want_a))
        assert torch.equal(x_t.cpu(), torch.from_numpy(want_x))
        assert real.shape == (4, 45 * 9 + 45 * 45 * 5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N,E,act", [(3, 45, 5, "relu"), (2, 9, 5, "tanh"), (1, 90, 10, "leaky"),
                                       (2, 128, 5, "relu"), (1, 256, 10, "leaky")])
def test_onehot_embedding_matches_the_dense_kernel(B, N, E, act, dtype):
    """dg_onehot_embed_fwd/bwd (table gather / segmented sum for one-hot graphs, reference utils.py:15-23 +
    models.py:57-61,92-94) == dg_embed_sym_fwd/bwd on the same one-hot input: output, exact i<->j symmetry and all
    four parameter gradients.  A tensor that is not one-hot is not declared one-hot."""
    from druggen_amd import functional as dgf, synth
    a, _, bonds, _ = synth.molecule_batch(B, N, E, 7, seed=B * 100 + N)
    a = torch.from_numpy(a).cuda()
    g = torch.Generator().manual_seed(1)
    ps = [(torch.randn(64, E, generator=g) * 0.4).cuda().requires_grad_(True), (torch.randn(64, generator=g) * 0.1).cuda().requires_grad_(True),
          (torch.randn(128, 64, generator=g) * 0.2).cuda().requires_grad_(True), (torch.randn(128, generator=g) * 0.1).cuda().requires_grad_(True)]
    assert dgf.one_hot_labels(a) is None
    dgf.as_one_hot(a)
    labels = dgf.one_hot_labels(a)
    assert labels is not None and torch.equal(labels.cpu(), torch.from_numpy(bonds).to(torch.int32))
    dense = dgf.embed_sym(a, *ps, act, dtype)
    fast = dgf.embed_sym_onehot(labels, *ps, act, dtype)
    tol = 1e-5 if dtype == torch.float32 else 4e-3
    assert fast.dtype == dtype
    assert float((fast.double() - dense.double()).norm() / dense.double().norm()) < tol
    assert torch.equal(fast, fast.permute(0, 2, 1, 3))
    up = torch.randn(B, N, N, 128, generator=g).to(dtype).cuda()
    gd = torch.autograd.grad(dense, ps, up)
    gf = torch.autograd.grad(fast, ps, up)
    for x, y in zip(gf, gd):
        # float32: the dense kernel's two gradient stages leave out the 2^-16-sized cross products (measured 3e-5 here);
        # bf16: the dense backward is csrc/embed_bf16.hip (bf16 MFMA products)
        assert float((x.double() - y.double()).norm() / y.double().norm()) < (1e-4 if dtype == torch.float32 else 6e-3)
    soft = torch.softmax(torch.randn(B, N, N, E, generator=g), -1).cuda()
    assert dgf.one_hot_labels(dgf.as_one_hot(soft)) is None
    # a batch buffer that is refilled in place must not keep its old labels: the cache is tied to the version counter
    a2, _, bonds2, _ = synth.molecule_batch(B, N, E, 7, seed=B * 100 + N + 1)
    a.copy_(torch.from_numpy(a2))
    assert dgf.one_hot_labels(a) is None
    assert torch.equal(dgf.one_hot_labels(dgf.as_one_hot(a)).cpu(), torch.from_numpy(bonds2).to(torch.int32))
    a.copy_(soft)
    assert dgf.one_hot_labels(dgf.as_one_hot(a)) is None


def test_launch_reports_the_entry_and_keeps_the_current_device():
    """``_lib.launch``: the entry's status comes back as ``check``'s RuntimeError under the entry's name (the entry returns from
    its argument check: nothing is launched), and a ``ref`` on another device leaves the caller's device current."""
    import re
    from druggen_amd import _lib
    args = (None, None, None, None, None, None, 1, 9, 128, 0.25, 0)
    refs = [torch.zeros(4, device="cuda:0")]
    if torch.cuda.device_count() >= 2:
        refs.append(torch.zeros(4, device="cuda:1"))
    torch.cuda.set_device(0)
    for ref in refs:
        with pytest.raises(RuntimeError, match=r"dg_attn_core_fwd failed \(-2\)") as err:
            _lib.launch("dg_attn_core_fwd", ref, *args)
        assert re.search("null pointer", str(err.value))
        assert torch.cuda.current_device() == 0
