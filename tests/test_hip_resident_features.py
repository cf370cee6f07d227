"""GPU tests of the feature plane of the resident molecule set (`dg_mol_gather_features` through
`druggen_amd.resident.ResidentMolecules(..., bits=, atom_dim=)`): node matrices that are a one-hot atom type followed by F
columns of 0 / 1 (the reference's --features).  A batch built by index equals, bit for bit, the dense tensors built on the host
from the same graphs -- the outputs are exact 0 / 1 floats and integers, so every comparison of a batch is `torch.equal` --
nothing is written outside the batch or read outside the store, and the trainer and the sampler run on such stores as they do
on one-hot ones."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 5
# (N, atom_dim, F, B): the smallest store; N M = 315, so molecule bases 1 and 2 are not 16-byte aligned; the reference's layout
# at the headline N; atom_dim and the word boundary inside one 16-byte store (M = 36); M = 255; N = 256 (64 KiB of LDS)
SHAPES = [(1, 1, 1, 1), (5, 9, 54, 3), (45, 13, 54, 4), (7, 3, 33, 5), (6, 9, 246, 2), (256, 13, 54, 2)]
BLOCKS = (5, 9, 6, 9, 1, 1, 5, 5, 5, 1, 7)      # the reference's descriptor blocks (dataset.py:161-185)


@functools.lru_cache(maxsize=None)
def _molecules(n, N, A, F, seed=0):
    """(bond labels [n, N, N] symmetric, density ~0.1, zero diagonal, molecule 0 without a bond and molecule 1 with every
    off-diagonal one -- as tests/test_hip_resident.py makes them; x [n, N, A + F] float32: a one-hot atom type, then F = 54 in
    the reference's blocks (one-hot inside each multi-column block) or coins, the last atom position of every molecule with ALL
    features set; graphs)."""
    rng = np.random.default_rng([n, N, A, F, seed])
    upper = np.triu((rng.random((n, N, N)) < 0.1) * rng.integers(1, E, size=(n, N, N)), 1)
    bonds = upper + upper.transpose(0, 2, 1)
    bonds[0] = 0
    if n > 1:
        full = np.triu(rng.integers(1, E, size=(N, N)), 1)
        bonds[1] = full + full.T
    x = np.zeros((n, N, A + F), dtype=np.float32)
    np.put_along_axis(x, rng.integers(0, A, size=(n, N, 1)), 1.0, axis=-1)
    if F == sum(BLOCKS):
        start = A
        for width in BLOCKS:
            if width == 1:
                x[..., start] = rng.integers(0, 2, size=(n, N))
            else:
                np.put_along_axis(x[..., start:start + width], rng.integers(0, width, size=(n, N, 1)), 1.0, axis=-1)
            start += width
    else:
        x[..., A:] = rng.integers(0, 2, size=(n, N, F))
    x[:, -1, A:] = 1.0
    graphs = []
    for i in range(n):
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x[i], edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    bonds.setflags(write=False)
    x.setflags(write=False)
    return bonds, x, tuple(graphs)


@functools.lru_cache(maxsize=None)
def _store(n, N, A, F, seed=0):
    from druggen_amd.resident import ResidentMolecules
    store = ResidentMolecules.from_graphs(_molecules(n, N, A, F, seed)[2], device="cuda", b_dim=E, atom_dim=A)
    assert (len(store), store.vertexes, store.m_dim, store.b_dim, store.atom_dim) == (n, N, A + F, E, A)
    assert store.bits.shape == (n, N, (F + 31) // 32) and store.bits.dtype == torch.int32
    return store


def _indices(n, B):
    """Index lists of length B over n = B + 3 molecules that are not sorted and hold a repeat (B >= 3: both in one list; B = 2
    cannot have both at once, so two lists; B = 1: the last molecule)."""
    if B == 1:
        return [[n - 1]]
    if B == 2:
        return [[n - 1, 0], [1, 1]]
    return [[n - 1, 0, n - 1] + [(3 * k + 1) % n for k in range(B - 3)]]


def _want(bonds, x, idx):
    """(real_graphs, a, labels, x) of the molecules idx, built on the host."""
    idx = list(idx)
    B = len(idx)
    a = np.eye(E, dtype=np.float32)[bonds[idx]]
    dense = np.ascontiguousarray(x[idx])
    real = np.concatenate([dense.reshape(B, -1), a.reshape(B, -1)], axis=1)
    return tuple(torch.from_numpy(t).cuda() for t in (real, a, bonds[idx].astype(np.int32), dense))


def _loaded(graphs, idx, M):
    """The only route on the parent commit: collate on the host, upload the dense node matrix, dg_densify."""
    from druggen_amd import smiles as sm
    from druggen_amd.data import load_molecules
    return load_molecules(sm.collate([graphs[i] for i in idx]), b_dim=E, m_dim=M, device="cuda", batch_size=len(idx))


@pytest.mark.parametrize("N,A,F,B", SHAPES)
def test_batch_is_bit_identical_to_the_dense_tensors(N, A, F, B):
    from druggen_amd import functional as dgf
    n, M = B + 3, A + F
    bonds, x_host, graphs = _molecules(n, N, A, F)
    store = _store(n, N, A, F)
    for idx in _indices(n, B):
        real, a, x = store.batch(torch.tensor(idx, device="cuda"))
        want_real, want_a, want_labels, want_x = _want(bonds, x_host, idx)
        assert a.shape == (B, N, N, E) and x.shape == (B, N, M) and real.shape == (B, N * M + N * N * E)
        assert a.dtype == x.dtype == real.dtype == torch.float32
        assert torch.equal(x, want_x) and torch.equal(a, want_a) and torch.equal(real, want_real)
        labels = dgf.one_hot_labels(a)
        assert labels is not None and labels.dtype == torch.int32 and torch.equal(labels, want_labels)
    if (N, A, F) == (45, 13, 54):      # ... which is what load_molecules makes of the collated batch
        for got, want in zip(store.batch(idx), _loaded(graphs, idx, M)):
            assert torch.equal(got, want)
    store.raise_bad_indices(wait=True)


def _cut_out(shape, dtype, sentinel, pad=65):
    """A contiguous buffer of `shape` cut from the middle of a larger allocation filled with `sentinel`, `pad` elements from
    its start: 65 elements = 260 bytes, so the buffer is 4-byte but not 16-byte aligned.  (whole allocation, buffer)"""
    numel = int(np.prod(shape))
    whole = torch.full((pad + numel + 64,), sentinel, dtype=dtype, device="cuda")
    return whole, whole[pad:pad + numel].view(shape)


@pytest.mark.parametrize("N,A,F,B", [(5, 9, 54, 3), (7, 3, 33, 5), (6, 9, 246, 2)])
def test_nothing_is_written_outside_the_batch_or_read_outside_the_plane(N, A, F, B):
    from druggen_amd.resident import ResidentMolecules
    n, M, W = B + 3, A + F, (F + 31) // 32
    bonds, x_host, graphs = _molecules(n, N, A, F)
    atoms, ptr, entries, bits = ResidentMolecules.pack_features(graphs, A, b_dim=E)
    # the plane in the middle of an allocation of all-ones words: a load past either end would put ones into x
    whole_bits, plane = _cut_out((n, N, W), torch.int32, -1)
    plane.copy_(torch.from_numpy(bits.view(np.int32)))
    inner = ResidentMolecules.from_arrays(atoms, ptr, entries, M, E, "cuda")
    store = ResidentMolecules(inner.atoms, inner.ptr, inner.entries, M, E, bits=plane, atom_dim=A)
    assert store.nbytes() == inner.nbytes() + 4 * n * N * W
    idx = [n - 1, 0, n - 1][:B] + [2] * max(B - 3, 0)      # the first and the last molecule of the plane
    whole_a, a = _cut_out((B, N, N, E), torch.float32, 7.0)
    whole_l, labels = _cut_out((B, N, N), torch.int32, -7)
    whole_x, x = _cut_out((B, N, M), torch.float32, 7.0)
    assert x.data_ptr() % 16 == 4
    real, a2, x2 = store.batch(torch.tensor(idx, device="cuda"), out=(a, labels, x))
    assert real is None and a2 is a and x2 is x
    _, want_a, want_labels, want_x = _want(bonds, x_host, idx)
    assert torch.equal(x, want_x) and torch.equal(a, want_a) and torch.equal(labels, want_labels)      # every element, no sentinel left
    for whole, buf, sentinel in ((whole_a, a, 7.0), (whole_l, labels, -7), (whole_x, x, 7.0)):
        assert (whole[1:65] == sentinel).all() and (whole[65 + buf.numel():] == sentinel).all()
        assert whole[65 + buf.numel():].numel() == 64
    assert (whole_bits[:65] == -1).all() and (whole_bits[65 + plane.numel():] == -1).all()
    store.raise_bad_indices(wait=True)


def test_index_handling():
    N, A, F, n = 5, 9, 54, 6
    M = A + F
    bonds, x_host, _ = _molecules(n, N, A, F)
    store = _store(n, N, A, F)
    real, a, x = store.batch(torch.empty(0, dtype=torch.int64, device="cuda"))      # B = 0: no launch
    assert real.shape == (0, N * M + N * N * E) and a.shape == (0, N, N, E) and x.shape == (0, N, M)
    assert x.is_cuda and x.dtype == torch.float32
    store.raise_bad_indices(wait=True)
    real, a, x = store.batch(torch.tensor([2, -1, n], device="cuda"))      # clamped: -1 -> 0, n -> n - 1
    want_real, want_a, _, want_x = _want(bonds, x_host, [2, 0, n - 1])
    assert torch.equal(x, want_x) and torch.equal(a, want_a) and torch.equal(real, want_real)
    with pytest.raises(RuntimeError, match=r"2 bad indices in an EARLIER ResidentMolecules.batch call: outside \[0, 6\)"):
        store.raise_bad_indices(wait=True)
    store.batch([1, 2])      # a clean call (a CPU list): nothing left to report
    store.raise_bad_indices(wait=True)


def test_batch_is_capturable():
    from druggen_amd import functional as dgf
    N, A, F, B = 45, 13, 54, 4
    n, M = B + 3, A + F
    bonds, x_host, _ = _molecules(n, N, A, F)
    store = _store(n, N, A, F)
    idx_static = torch.tensor([0, 1, 2, 3], device="cuda")
    bufs = (torch.full((B, N, N, E), float("nan"), device="cuda"), torch.full((B, N, N), -1, dtype=torch.int32, device="cuda"),
            torch.full((B, N, M), float("nan"), device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        store.batch(idx_static, out=bufs)      # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        store.batch(idx_static, out=bufs)
    for content in ([6, 1, 1, 5], [3, 0, 4, 2]):
        idx_static.copy_(torch.tensor(content, device="cuda"))      # in place: the graph reads this tensor
        bufs[0].fill_(float("nan"))
        bufs[2].fill_(float("nan"))
        graph.replay()
        _, eager_a, eager_x = store.batch(torch.tensor(content, device="cuda"))
        _, want_a, want_labels, want_x = _want(bonds, x_host, content)
        assert torch.equal(bufs[0], eager_a) and torch.equal(bufs[2], eager_x) and torch.equal(bufs[1], dgf.one_hot_labels(eager_a))
        assert torch.equal(bufs[0], want_a) and torch.equal(bufs[2], want_x) and torch.equal(bufs[1], want_labels)
    store.raise_bad_indices(wait=True)
    del graph


def test_a_store_without_a_plane_is_todays_store():
    from druggen_amd import functional as dgf
    from druggen_amd.resident import ResidentMolecules
    n, N, M = 7, 5, 13
    rng = np.random.default_rng(5)
    bonds = _molecules(n, N, 9, 54)[0]
    graphs = []
    for i in range(n):
        x = np.zeros((N, M), dtype=np.float32)
        x[np.arange(N), rng.integers(0, M, size=N)] = 1.0
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x, edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    today = ResidentMolecules.from_graphs(graphs, device="cuda", m_dim=M, b_dim=E)
    atoms, ptr, entries = ResidentMolecules.pack(graphs, m_dim=M, b_dim=E)
    split = SimpleNamespace(x=np.concatenate([g.x for g in graphs]), batch=np.arange(n).repeat(N),
                            edge_index=np.concatenate([g.edge_index + i * N for i, g in enumerate(graphs)], 1),
                            edge_attr=np.concatenate([g.edge_attr for g in graphs]))
    idx = torch.tensor([6, 0, 6, 3], device="cuda")
    want = today.batch(idx)
    for store in (ResidentMolecules.from_graphs(graphs, device="cuda", m_dim=M, b_dim=E, atom_dim=None),
                  ResidentMolecules.from_arrays(atoms, ptr, entries, M, E, "cuda", bits=None, atom_dim=None),
                  ResidentMolecules.from_batch(split, n, device="cuda", m_dim=M, b_dim=E, atom_dim=None),
                  ResidentMolecules(today.atoms, today.ptr, today.entries, M, E, bits=None, atom_dim=None),
                  ResidentMolecules.from_graphs(graphs, device="cuda", b_dim=E, atom_dim=M)):      # F = 0: no plane either
        assert store.bits is None and store.atom_dim == M and store.nbytes() == today.nbytes()
        got = store.batch(idx)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        assert torch.equal(dgf.one_hot_labels(got[1]), dgf.one_hot_labels(want[1]))
        store.raise_bad_indices(wait=True)
    assert all(torch.equal(g, w) for g, w in zip(want, _loaded(graphs, idx.tolist(), M)))
    # from_batch with atom_dim: the feature store of the same split
    bonds9, x9, graphs9 = _molecules(6, 5, 9, 54)
    whole = SimpleNamespace(x=np.concatenate([g.x for g in graphs9]), batch=np.arange(6).repeat(5),
                            edge_index=np.concatenate([g.edge_index + i * 5 for i, g in enumerate(graphs9)], 1),
                            edge_attr=np.concatenate([g.edge_attr for g in graphs9]))
    store = ResidentMolecules.from_batch(whole, 6, device="cuda", b_dim=E, atom_dim=9)
    assert torch.equal(store.bits, _store(6, 5, 9, 54).bits) and torch.equal(store.batch([4, 1])[2], _want(bonds9, x9, [4, 1])[3])


def test_the_constructor_checks_the_plane():
    from druggen_amd.resident import ResidentMolecules
    good = _store(6, 5, 9, 54)
    parts = (good.atoms, good.ptr, good.entries, 63, E)
    ResidentMolecules(*parts, bits=good.bits, atom_dim=9)
    wider = torch.zeros(6, 5, 4, dtype=torch.int32, device="cuda")
    for bits, atom_dim, error, match in (
            (good.bits.long(), 9, ValueError, "bits must be a contiguous torch.int32"),
            (wider[:, :, :2], 9, ValueError, "bits must be a contiguous torch.int32"),
            (good.bits.cpu(), 9, RuntimeError, "bits is not a GPU tensor"),
            (good.bits[:5], 9, ValueError, r"bits \[n, N, ceil"),
            (good.bits, 31, ValueError, r"bits \[n, N, ceil"),            # F = 32: one word
            (good.bits, None, ValueError, "needs 1 <= atom_dim < m_dim"),
            (good.bits, 0, ValueError, "needs 1 <= atom_dim < m_dim"),
            (good.bits, 63, ValueError, "needs 1 <= atom_dim < m_dim"),
            (None, 9, ValueError, "needs the feature plane")):
        with pytest.raises(error, match=match):
            ResidentMolecules(*parts, bits=bits, atom_dim=atom_dim)


# ---- the trainer and the sampler on feature stores -------------------------------------------------------------------------------
T_N, T_A, T_F, T_B, T_MOL, T_DRUG, T_SEED, T_LR = 9, 5, 54, 4, 11, 6, 3, 2e-3
T_M = T_A + T_F


def _nets():
    from druggen_amd import synth
    from druggen_amd.model import Discriminator, Generator
    from druggen_amd.trainer import GANStep
    nets = []
    for cls, seed in ((Generator, 11), (Discriminator, 12)):
        net = cls("relu", T_N, E, T_M, 0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
        params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=seed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        nets.append(net.cuda())
    G, D = nets
    return G, D, GANStep(G, D, g_lr=T_LR, d_lr=T_LR)


def _flat(G, D):
    torch.cuda.synchronize()
    return torch.cat([p.detach().reshape(-1) for p in list(G.parameters()) + list(D.parameters())]).clone()


@functools.lru_cache(maxsize=None)
def _eps():
    from druggen_amd import synth
    return tuple(torch.from_numpy(t).cuda() for t in synth.interpolation_eps(T_B, 9))


@functools.lru_cache(maxsize=None)
def _dense_fed(submodel):
    """Two steps of an eager GANStep fed the DENSE batches (load_molecules with the node matrix uploaded from the host) of the
    indices the trainer's schedule draws: (start, parameters, losses [2, 2])."""
    from druggen_amd.schedule import epoch_schedule
    mols, drugs = _molecules(T_MOL, T_N, T_A, T_F, 1)[2], _molecules(T_DRUG, T_N, T_A, T_F, 2)[2]
    G, D, st = _nets()
    start = _flat(G, D)
    g = torch.Generator(device="cuda").manual_seed(T_SEED)
    history = []
    for mi, di in epoch_schedule(T_MOL, T_DRUG if submodel == "DrugGEN" else None, T_B, generator=g, device="cuda"):
        _, ma, mx = _loaded(mols, mi.tolist(), T_M)
        _, da, dx = _loaded(drugs, di.tolist(), T_M) if submodel == "DrugGEN" else (None, ma, mx)
        history.append(torch.stack(st.step(da, dx, ma, mx, eps=_eps())))
    assert len(history) == 2
    return start, _flat(G, D), torch.stack(history)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("submodel", ["NoTarget", "DrugGEN"])
def test_trainer_on_feature_stores_equals_the_step_fed_dense_batches(submodel, graph):
    """The comparisons tests/test_hip_loop.py makes on one-hot stores, with its tolerances.  graph=False is its
    `_same_step_twice` (the same eager steps on the same inputs, held to test_hip_step.py's criterion for that):
    |p - q| <= 1e-6 |q - start| over all parameters and |h - k| <= 1e-6 |k| over the loss history.  graph=True is its `_tracks`
    (the captured step against the eager one): |p - q| <= 0.05 |q - start|.  `_tracks` sets no bound on the losses; they get the
    bound every comparison of one step's losses through two routes has in this suite (tests/test_hip_step.py: the step against
    the fp64 reference, the low-memory step against the default one): |a - b| <= 1e-3 max(1, |b|) per loss."""
    from druggen_amd.loop import ResidentTrainer
    mols, drugs = _store(T_MOL, T_N, T_A, T_F, 1), _store(T_DRUG, T_N, T_A, T_F, 2)
    G, D, st = _nets()
    tr = ResidentTrainer(st, mols, drugs if submodel == "DrugGEN" else None, batch_size=T_B, submodel=submodel, graph=graph,
                         seed=T_SEED, eps=_eps())
    assert tr.steps_per_epoch == 2 and (tr.graphed is not None) == graph
    start, want, want_losses = _dense_fed(submodel)
    assert torch.equal(_flat(G, D), start)
    losses = torch.stack([torch.stack(tr.step(mi, di)).clone() for mi, di in tr.schedule()])
    got = _flat(G, D)
    for s in tr.stores:
        s.raise_bad_indices(wait=True)
    moved = (want - start).norm()
    print(submodel, "graph" if graph else "eager", "parameters", float((got - want).norm()), "moved", float(moved),
          "losses", losses.tolist(), want_losses.tolist())
    assert losses.shape == (2, 2) and torch.isfinite(want).all() and float(moved) > 0
    if graph:
        assert (got - want).norm() <= 0.05 * moved
        assert ((losses - want_losses).abs() <= 1e-3 * want_losses.abs().clamp(min=1.0)).all()
    else:
        assert (got - want).norm() <= 1e-6 * moved
        assert (losses - want_losses).norm() <= 1e-6 * want_losses.norm()


def test_trainer_refuses_stores_that_split_the_node_row_differently():
    from druggen_amd.loop import ResidentTrainer
    from druggen_amd.resident import ResidentMolecules
    mols = _store(T_MOL, T_N, T_A, T_F, 1)
    drugs = _store(T_DRUG, T_N, T_A + 1, T_F - 1, 2)      # the same N, m_dim, b_dim and plane width
    assert (drugs.vertexes, drugs.m_dim, drugs.b_dim, drugs.bits.shape[2]) == (mols.vertexes, mols.m_dim, mols.b_dim, mols.bits.shape[2])
    _, _, st = _nets()
    for graph in (False, True):
        with pytest.raises(ValueError, match="must share N, m_dim, b_dim, atom_dim"):
            ResidentTrainer(st, mols, drugs, batch_size=T_B, graph=graph, seed=T_SEED, eps=_eps())
    assert isinstance(mols, ResidentMolecules)


@pytest.mark.parametrize("graph", [True, False])
def test_sample_from_a_feature_store_equals_sample_on_the_dense_batch(graph):
    from druggen_amd.decode import _FIELDS
    from druggen_amd.sampling import MoleculeSampler
    graphs, mols = _molecules(T_MOL, T_N, T_A, T_F, 1)[2], _store(T_MOL, T_N, T_A, T_F, 1)
    G, _, _ = _nets()
    _, a0, x0 = _loaded(graphs, list(range(T_B)), T_M)
    sampler = MoleculeSampler(G, a0, x0, graph=graph, bond_order2=[0, 2, 4, 6, 3], warmup=1)
    decoded = []
    for idx in ([7, 1, 10, 0], [2, 2, 9, 5]):
        got, got_nodes, got_edges = sampler.sample_from(mols, torch.tensor(idx, device="cuda"), keep_logits=True)
        got, got_nodes, got_edges = got.cpu(), got_nodes.clone(), got_edges.clone()
        _, a, x = _loaded(graphs, idx, T_M)
        want, want_nodes, want_edges = sampler.sample(a, x, keep_logits=True)
        want = want.cpu()
        assert torch.equal(got_nodes, want_nodes) and torch.equal(got_edges, want_edges)
        for name in _FIELDS:
            if name == "bonds":      # rows past n_bonds are unwritten memory
                assert all(np.array_equal(got.edge_list(b), want.edge_list(b)) for b in range(T_B))
            else:
                assert np.array_equal(getattr(got, name), getattr(want, name)), name
        decoded.append(want.atoms.copy())
    assert not np.array_equal(decoded[0], decoded[1])
    mols.raise_bad_indices(wait=True)
