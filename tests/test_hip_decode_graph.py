"""GPU tests of the graph decode (`dg_decode_graph` through `decode.decode_molecule_graphs`) against the numpy restatement
of tests/decode_graph_ref.py, and of `sampling.MoleculeSampler` against the eager forward + decode.  Every output is an
integer function of the labels: every comparison is exact."""
import numpy as np
import pytest
import torch

import cases
import decode_graph_ref as ref

pytestmark = pytest.mark.gpu

ORDER2 = [0, 2, 4, 6, 3]


def _order2(E):
    return [(3 * k) % 7 for k in range(E)]      # any byte table does: the sum is checked, not chemistry


def _decode_and_compare(node, edge, order2, cap=None):
    """node / edge: numpy float32 logits.  Decode on the GPU into a sentinel-filled buffer, compare with the restatement."""
    from druggen_amd import decode
    B, N = node.shape[:2]
    c = N * (N - 1) // 2 if cap is None else cap
    out = decode.MoleculeBatch.empty(B, N, c, order2 is not None, "cuda")
    out.buffer.fill_(0xEE)
    got = decode.decode_molecule_graphs(torch.from_numpy(node).cuda(), torch.from_numpy(edge).cuda(), bond_order2=order2,
                                        bond_cap=cap, out=out)
    assert got is out
    host = got.cpu()
    want = ref.decode_graph(node, edge, order2)
    ref.assert_batch_equals(host, want, cap=cap, sentinel=0xEE)
    return host, want


SHAPES = [  # (B, N, M, E): every N, E, M and B the kernel's tiling distinguishes
    (1, 1, 1, 1), (3, 1, 13, 5), (3, 2, 13, 2), (257, 2, 1, 1), (257, 9, 13, 5), (3, 45, 13, 5), (257, 45, 1, 5),
    (3, 63, 13, 10), (1, 64, 13, 1), (257, 64, 13, 2), (3, 65, 1, 2), (3, 90, 13, 10), (1, 96, 13, 5), (3, 97, 13, 2),
    (3, 128, 13, 5), (1, 128, 1, 10), (1, 255, 13, 10), (3, 255, 13, 5), (3, 256, 13, 5), (1, 256, 1, 1), (3, 256, 13, 10),
    (1, 256, 13, 2),
]


@pytest.mark.parametrize("B,N,M,E", SHAPES)
def test_decode_matches_restatement_on_dense_and_sparse_logits(B, N, M, E):
    rng = np.random.default_rng(1000 * N + 10 * E + M + B)
    node = rng.standard_normal((B, N, M)).astype(np.float32)
    edge = rng.standard_normal((B, N, N, E)).astype(np.float32)
    _, want = _decode_and_compare(node, edge, _order2(E))      # dense: a random label per pair
    # sparse, the trained-model regime: label 0 wins ~95 % of the pairs
    edge[..., 0] += np.where(rng.random((B, N, N)) < 0.95, 20.0, 0.0).astype(np.float32)
    _, sparse = _decode_and_compare(node, edge, _order2(E))
    if E > 1 and N >= 45:
        pairs = B * N * (N - 1) // 2
        assert sum(w["n_bonds"] for w in want) > 0.4 * pairs      # (E - 1) / E of the pairs
        assert 0 < sum(w["n_bonds"] for w in sparse) < 0.2 * pairs


def test_decode_without_valence_table():
    rng = np.random.default_rng(7)
    host, _ = _decode_and_compare(rng.standard_normal((2, 45, 13)).astype(np.float32),
                                  rng.standard_normal((2, 45, 45, 5)).astype(np.float32), None)
    assert host.valence2 is None


def test_structured_graphs_at_256_atoms():
    N, M, E = 256, 13, 5
    graphs = [ref.empty_graph(N), ref.path(N), ref.far_end_path(N), ref.zigzag_path(N), ref.star(N, 0), ref.star(N, 255),
              ref.star(N, 100), ref.complete(N, E), ref.two_equal_components(N), ref.upper_only(N)]
    labels = np.stack(graphs)
    atoms = (np.arange(len(graphs) * N).reshape(len(graphs), N) * 7) % M
    node, edge = ref.one_hot_logits(atoms, labels, M, E)
    host, want = _decode_and_compare(node, edge, ORDER2)
    assert [w["n_components"] for w in want] == [256, 1, 1, 1, 1, 1, 1, 1, 2, 256]
    assert [w["n_bonds"] for w in want] == [0, 255, 255, 255, 255, 255, 255, 32640, 254, 0]
    assert (want[8]["largest"], want[8]["largest_size"]) == (0, 128)
    for b in range(len(graphs)):      # the dense matrix rebuilt from the list gives the reference's walk the same bonds
        assert np.array_equal(host.edge_labels(b), np.tril(labels[b], -1))
    assert ref.reference_bond_walk(host.edge_labels(7)) == [tuple(t) for t in want[7]["bonds"].tolist()]


@pytest.mark.parametrize("B,N,M,E", [(3, 45, 13, 5), (2, 97, 4, 3), (1, 256, 13, 2)])
def test_ties_and_nans_follow_the_first_maximum_rule(B, N, M, E):
    """Constructed, not hoped for: logits drawn from {0, 1, 2} tie in most rows, a tenth of them are NaN, and whole rows are
    made constant / all-NaN / -inf.  The restatement alone decides; `argmax_labels` on the same tensors has to agree."""
    from druggen_amd import decode
    rng = np.random.default_rng(N)
    node = rng.integers(0, 3, (B, N, M)).astype(np.float32)
    edge = rng.integers(0, 3, (B, N, N, E)).astype(np.float32)
    node[rng.random(node.shape) < 0.1] = np.nan
    edge[rng.random(edge.shape) < 0.1] = np.nan
    edge[:, 1:, 0, :] = 1.0                      # constant rows: label 0
    edge[:, N - 1, : N // 2, :] = np.nan         # all-NaN rows: label 0
    edge[:, N // 2, : N // 4, :] = -np.inf       # all -inf: label 0
    if E > 1:
        edge[:, N - 1, N // 2: N - 1, 0] = 5.0
        edge[:, N - 1, N // 2: N - 1, E - 1] = np.nan      # a NaN behind a larger finite value still wins: a bond
    host, want = _decode_and_compare(node, edge, _order2(E))
    if E > 1:
        for w in want:
            last = w["bonds"][(w["bonds"][:, 0] == N - 1) & (w["bonds"][:, 1] >= N // 2)]
            assert len(last) == N - 1 - N // 2 and (E > 2 or (last[:, 2] == 1).all())
    n_lab, e_lab = decode.decode_molecule_labels(torch.from_numpy(node).cuda(), torch.from_numpy(edge).cuda())
    assert np.array_equal(n_lab.cpu().numpy(), host.atoms)
    e_lab = e_lab.cpu().numpy()
    for b in range(B):
        assert np.array_equal(host.edge_labels(b), np.tril(e_lab[b], -1))


@pytest.mark.parametrize("cap", [0, 1, 7, 100])
def test_bond_cap_writes_a_prefix_and_leaves_the_rest_untouched(cap):
    rng = np.random.default_rng(11)
    node = rng.standard_normal((5, 45, 13)).astype(np.float32)
    edge = rng.standard_normal((5, 45, 45, 5)).astype(np.float32)
    edge[1, ..., 0] += 20.0                          # molecule 1: no bonds at all
    edge[2, :, :, 0] += 20.0
    edge[2, 3, 1, 0] = edge[2, 9, 4, 0] = -20.0      # molecule 2: exactly two bonds
    host, want = _decode_and_compare(node, edge, ORDER2, cap=cap)
    assert [w["n_bonds"] for w in want][1:3] == [0, 2] and want[0]["n_bonds"] > 100
    assert host.truncated.tolist() == [True, False, cap < 2, True, True]


def test_decode_on_a_side_stream_and_twice_gives_the_same_bytes():
    from druggen_amd import decode
    rng = np.random.default_rng(3)
    node_h = rng.standard_normal((6, 90, 13)).astype(np.float32)
    edge_h = rng.standard_normal((6, 90, 90, 10)).astype(np.float32)
    want = ref.decode_graph(node_h, edge_h, _order2(10))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    bufs = []
    with torch.cuda.stream(stream):
        node, edge = torch.from_numpy(node_h).cuda(), torch.from_numpy(edge_h).cuda()
        for _ in range(2):
            out = decode.MoleculeBatch.empty(6, 90, 90 * 89 // 2, True, "cuda")
            out.buffer.fill_(0x5A)
            bufs.append(decode.decode_molecule_graphs(node, edge, bond_order2=_order2(10), out=out))
        stream.synchronize()
        hosts = [b.cpu() for b in bufs]
    torch.cuda.current_stream().wait_stream(stream)
    assert np.array_equal(hosts[0].buffer, hosts[1].buffer)
    ref.assert_batch_equals(hosts[0], want, sentinel=0x5A)


def test_a_molecule_does_not_depend_on_its_batch():
    from druggen_amd import decode
    rng = np.random.default_rng(4)
    B, N = 9, 45
    node = torch.from_numpy(rng.standard_normal((B, N, 13)).astype(np.float32)).cuda()
    edge = torch.from_numpy(rng.standard_normal((B, N, N, 5)).astype(np.float32)).cuda()
    whole = decode.decode_molecule_graphs(node, edge, bond_order2=ORDER2).cpu()
    perm = [4, 0, 8, 2, 7, 1, 6, 3, 5]
    idx = torch.tensor(perm, device="cuda")
    moved = decode.decode_molecule_graphs(node[idx].contiguous(), edge[idx].contiguous(), bond_order2=ORDER2).cpu()
    alone = decode.decode_molecule_graphs(node[3:4], edge[3:4], bond_order2=ORDER2).cpu()      # a view at an odd offset
    for k, b in enumerate(perm):
        _same_molecule(moved, k, whole, b)
    _same_molecule(alone, 0, whole, 3)


def _same_molecule(h1, b1, h2, b2):
    assert np.array_equal(h1.edge_list(b1), h2.edge_list(b2))
    for name in ("atoms", "component", "valence2", "n_bonds", "n_components", "largest", "largest_size"):
        assert np.array_equal(getattr(h1, name)[b1], getattr(h2, name)[b2]), name


def _same_batch(h1, h2):
    assert (h1.B, h1.N, h1.cap) == (h2.B, h2.N, h2.cap)
    for b in range(h1.B):
        _same_molecule(h1, b, h2, b)


def test_cpu_is_one_transfer_for_the_batch():
    from druggen_amd import decode
    rng = np.random.default_rng(6)
    node = torch.from_numpy(rng.standard_normal((16, 45, 13)).astype(np.float32)).cuda()
    edge = torch.from_numpy(rng.standard_normal((16, 45, 45, 5)).astype(np.float32)).cuda()
    batch = decode.decode_molecule_graphs(node, edge, bond_order2=ORDER2)
    calls = []
    real = {n: getattr(torch.Tensor, n) for n in ("cpu", "to", "copy_", "numpy", "tolist", "item")}
    try:
        for n, f in real.items():
            setattr(torch.Tensor, n, (lambda n_, f_: lambda self, *a, **k: (calls.append(n_), f_(self, *a, **k))[1])(n, f))
        host = batch.cpu()
        lists = [host.edge_list(b) for b in range(16)]
        dense = [host.edge_labels(b) for b in range(16)]
    finally:
        for n, f in real.items():
            setattr(torch.Tensor, n, f)
    assert calls.count("cpu") == 1 and not [c for c in calls if c in ("to", "copy_", "tolist", "item")], calls
    assert len(lists) == len(dense) == 16 and host.is_host and host.cpu() is host
    for name in ("atoms", "bonds", "n_bonds", "component", "n_components", "largest", "largest_size", "valence2"):
        arr = getattr(host, name)
        assert isinstance(arr, np.ndarray) and np.shares_memory(arr, host.buffer), name
    with pytest.raises(RuntimeError, match=r"\.cpu\(\)"):
        batch.edge_list(0)


# ---- MoleculeSampler ---------------------------------------------------------------------------------------------------
def _generator(case, seed_shift=0):
    from druggen_amd.model import Generator
    cfg = cases.net_config(case)
    G = Generator(cfg.act, cfg.vertexes, cfg.edges, cfg.nodes, cfg.dropout, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                  mlp_ratio=cfg.mlp_ratio)
    gp, _ = cases.build_params(dict(case, seed=case["seed"] + seed_shift))
    G.load_state_dict({k: torch.from_numpy(v) for k, v in gp.items()})
    return cfg, G.cuda()


def _batches(cfg, B, n, one_hot, seed):
    from druggen_amd import synth
    out = []
    for k in range(n):
        a, x, _, _ = synth.molecule_batch(B, cfg.vertexes, cfg.edges, cfg.nodes, seed=seed + k)
        a, x = torch.from_numpy(a).cuda(), torch.from_numpy(x).cuda()
        if not one_hot:      # a dense edge tensor, as a generator's output fed back would be
            g = torch.Generator(device="cuda").manual_seed(seed + k)
            a = torch.softmax(torch.randn(a.shape, device="cuda", generator=g) + 2.0 * a, -1)
        out.append((a, x))
    return out


def _eager(G, a, x, one_hot):
    """The eager route the sampler has to reproduce bit for bit: G.eval() under inference_mode, then the decode."""
    from druggen_amd import decode
    from druggen_amd.functional import as_one_hot
    was = G.training
    G.eval()
    a = a.clone()
    if one_hot:
        as_one_hot(a)
    with torch.inference_mode():
        _, _, ns, es = G(a, x)
        batch = decode.decode_molecule_graphs(ns, es, bond_order2=ORDER2)
    G.train(was)
    return batch.cpu(), ns.clone(), es.clone()


def _check_sampler(sampler, G, batches, one_hot, seen):
    for a, x in batches:
        got, ns, es = sampler.sample(a, x, keep_logits=True)
        want, wns, wes = _eager(G, a, x, one_hot)
        assert torch.equal(ns, wns) and torch.equal(es, wes)
        _same_batch(got.cpu(), want)
        seen.append(es.clone())
        assert G.training and all(m.training for m in G.modules())


SAMPLER_CASES = {"n9_depth1": dict(cases.CASES["c1_b4"]),
                 "n45_depth2": dict(cases.CASES["c2_b2"], cfg=dict(cases.CASES["c2_b2"]["cfg"], depth=2))}


@pytest.mark.parametrize("one_hot", [True, False], ids=["onehot", "dense"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(SAMPLER_CASES))
def test_graphed_sampler_equals_eager_forward_and_decode(name, dtype, one_hot):
    from druggen_amd import functional as dgf
    from druggen_amd.optim import FlatAdamW
    from druggen_amd.sampling import MoleculeSampler
    case = SAMPLER_CASES[name]
    cfg, G = _generator(case)
    G.train()
    B = 3
    batches = _batches(cfg, B, 6, one_hot, seed=500)
    with dgf.activations(dtype):
        sampler = MoleculeSampler(G, *batches[0], bond_order2=ORDER2, warmup=2)
        assert G.training
        seen = []
        _check_sampler(sampler, G, batches[1:], one_hot, seen)                 # five new batches after the capture
        assert not torch.equal(seen[0], seen[1])
        # weights overwritten in place: a replay has to see them
        _, other = _generator(case, seed_shift=7)
        G.load_state_dict(other.state_dict())
        after = []
        _check_sampler(sampler, G, batches[1:3], one_hot, after)
        assert not torch.equal(after[0], seen[0])
        # torch's AdamW steps in place; FlatAdamW's first step MOVES the parameters into its flat buffer (the sampler captures
        # again), its second one is in place
        flat = FlatAdamW(G.parameters(), lr=1e-2)
        for opt in (torch.optim.AdamW(G.parameters(), lr=1e-2), flat, flat):
            g = torch.Generator(device="cuda").manual_seed(9)
            for p in G.parameters():
                p.grad = torch.randn(p.shape, device="cuda", generator=g)
            opt.step()
            stepped = []
            _check_sampler(sampler, G, batches[1:3], one_hot, stepped)
            assert not torch.equal(stepped[0], after[0])
            after = stepped
        if one_hot:
            dense = torch.softmax(torch.randn_like(batches[1][0]), -1)
            with pytest.raises(RuntimeError, match="one-hot"):
                sampler.sample(dense, batches[1][1])
            _check_sampler(sampler, G, batches[3:4], one_hot, [])              # the rejected batch left the buffers intact
        with pytest.raises(RuntimeError, match="batch shape"):
            sampler.sample(batches[1][0][:2], batches[1][1][:2])


def test_eager_sampler_and_eval_mode_are_restored():
    from druggen_amd.sampling import MoleculeSampler
    case = SAMPLER_CASES["n9_depth1"]
    cfg, G = _generator(case)
    batches = _batches(cfg, 4, 2, True, seed=900)
    sampler = MoleculeSampler(G, *batches[0], graph=False, bond_order2=ORDER2, bond_cap=5)
    G.train()
    G.readout_e.eval()      # mixed flags come back as they were
    got = sampler.sample(*batches[1])
    assert G.training and not G.readout_e.training and got.cap == 5
    G.train()
    want, _, _ = _eager(G, *batches[1], True)
    host = got.cpu()
    for b in range(4):
        assert np.array_equal(host.edge_list(b), want.edge_list(b)[:5]) and int(host.n_bonds[b]) == int(want.n_bonds[b])
        assert np.array_equal(host.component[b], want.component[b])
