"""GPU tests of the loop over resident molecule sets (`druggen_amd.loop.ResidentTrainer`, `MoleculeSampler.sample_from`, the
static inputs of the captured step and sampler): the trainer equals the loop fed by hand from the same index schedule, the
captured route tracks the eager one, and a replay never reads the dense buffers or labels of an older batch.

Shapes: dim 128, 8 heads, mlp_ratio 3, depth 1; N = 5, E = 5, M = 13 (N N E = 125 is odd: the misaligned-base case of the
gather); batch 4 of 11 molecules (2 steps per epoch, 3 molecules dropped) and 6 drugs (one drug batch per permutation: the drug
permutation restarts at every step after an epoch's first); 2 epochs."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, E, M, B, N_MOL, N_DRUG = 5, 5, 13, 4, 11, 6
EPOCHS, SEED, LR = 2, 3, 2e-3      # (the learning rate of tests/test_hip_step.py's replay tests: stale inputs show as O(1) differences)


@functools.lru_cache(maxsize=None)
def _graphs(n, seed):
    """Synthetic molecules as tests/test_hip_resident.py::_molecules makes them: symmetric bond labels of density ~0.1 with a
    zero diagonal, molecule 0 without a bond, molecule 1 with every off-diagonal one."""
    rng = np.random.default_rng([n, N, M, E, seed])
    upper = np.triu((rng.random((n, N, N)) < 0.1) * rng.integers(1, E, size=(n, N, N)), 1)
    bonds = upper + upper.transpose(0, 2, 1)
    bonds[0] = 0
    full = np.triu(rng.integers(1, E, size=(N, N)), 1)
    bonds[1] = full + full.T
    atoms = rng.integers(0, M, size=(n, N))
    graphs = []
    for i in range(n):
        x = np.zeros((N, M), dtype=np.float32)
        x[np.arange(N), atoms[i]] = 1.0
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x, edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    return tuple(graphs)


def _new_stores():
    from druggen_amd.resident import ResidentMolecules
    return (ResidentMolecules.from_graphs(_graphs(N_MOL, 1), device="cuda", m_dim=M, b_dim=E),
            ResidentMolecules.from_graphs(_graphs(N_DRUG, 2), device="cuda", m_dim=M, b_dim=E))


_stores = functools.lru_cache(maxsize=None)(_new_stores)


@functools.lru_cache(maxsize=None)
def _eps():
    from druggen_amd import synth
    return tuple(torch.from_numpy(t).cuda() for t in synth.interpolation_eps(B, 9))


def _nets(dropout=0.0, **step_kw):
    from druggen_amd import synth
    from druggen_amd.model import Discriminator, Generator
    from druggen_amd.trainer import GANStep
    nets = []
    for cls, seed in ((Generator, 11), (Discriminator, 12)):
        net = cls("relu", N, E, M, dropout, dim=128, depth=1, heads=8, mlp_ratio=3)
        params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=seed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        nets.append(net.cuda())
    G, D = nets
    return G, D, GANStep(G, D, g_lr=LR, d_lr=LR, **step_kw)


def _flat(G, D):
    torch.cuda.synchronize()
    return torch.cat([p.detach().reshape(-1) for p in list(G.parameters()) + list(D.parameters())]).clone()


@functools.lru_cache(maxsize=None)
def _start():
    G, D, _ = _nets()
    return _flat(G, D)


@functools.lru_cache(maxsize=None)
def _trainer_run(submodel, graph):
    """Two epochs of ResidentTrainer, stepped by hand so that the static inputs can be looked at after every step:
    (parameters, loss history [4, 2], per step: inputs == store.batch(idx)?, per step: D's inputs == the generator's?)."""
    from druggen_amd import functional as dgf
    from druggen_amd.loop import ResidentTrainer
    mols, drugs = _stores()
    G, D, st = _nets()
    tr = ResidentTrainer(st, mols, drugs if submodel == "DrugGEN" else None, batch_size=B, submodel=submodel, graph=graph,
                         seed=SEED, eps=_eps())
    assert tr.steps_per_epoch == 2 and (tr.world, tr.rank) == (1, 0) and (tr.graphed is not None) == graph
    if graph:      # the capture's warm-up iterations were undone: the loop starts from the weights it was given
        assert torch.equal(_flat(G, D), _start())
    history, fresh, aliased = [], [], []
    for _ in range(EPOCHS):
        for mi, di in tr.schedule():
            history.append(torch.stack(tr.step(mi, di)).clone())
            if graph:
                disc, gen = tr.graphed.inputs()
                want = [drugs.batch(di) if submodel == "DrugGEN" else mols.batch(mi), mols.batch(mi)]
                fresh.append(all(torch.equal(a, w[1]) and torch.equal(lab, dgf.one_hot_labels(w[1])) and torch.equal(x, w[2])
                                 and dgf.one_hot_labels(a) is lab for (a, lab, x), w in zip((disc, gen), want)))
                aliased.append(all(torch.equal(p, q) for p, q in zip(disc, gen)))
    for s in (mols, drugs):
        s.raise_bad_indices(wait=True)
    return _flat(G, D), torch.stack(history), fresh, aliased


@functools.lru_cache(maxsize=None)
def _hand_fed(submodel):
    """The same two epochs, fed by hand: epoch_schedule -> store.batch -> GANStep.step."""
    from druggen_amd.schedule import epoch_schedule
    mols, drugs = _stores()
    G, D, st = _nets()
    g = torch.Generator(device="cuda").manual_seed(SEED)
    history = []
    for _ in range(EPOCHS):
        for mi, di in epoch_schedule(N_MOL, N_DRUG if submodel == "DrugGEN" else None, B, generator=g, device="cuda"):
            _, ma, mx = mols.batch(mi)
            _, da, dx = drugs.batch(di) if submodel == "DrugGEN" else (None, ma, mx)
            history.append(torch.stack(st.step(da, dx, ma, mx, eps=_eps())))
    return _flat(G, D), torch.stack(history)


def _same_step_twice(got, want, what):
    """Two runs of the same steps on the same inputs.  tests/test_hip_step.py does not hold the step bit-reproducible; its
    criterion for this is test_graphed_step_with_static_interpolation_weights_equals_the_eager_step's:
    |a - b| <= 1e-6 |a - start| over all parameters of G and D.  The loss history has no start to move from: the same 1e-6,
    relative to its own norm (losses are O(1) float32 means; 1e-6 is ~16 ulp of them)."""
    p, h = got[0], got[1]
    q, k = want[0], want[1]
    moved = (q - _start()).norm()
    print(what, "parameters", float((p - q).norm()), "moved", float(moved), "losses", float((h - k).norm()), float(k.norm()))
    assert torch.isfinite(q).all() and float(moved) > 0
    assert (p - q).norm() <= 1e-6 * moved
    assert (h - k).norm() <= 1e-6 * k.norm()


def _tracks(got, want, what):
    """test_graphed_step_replays_on_new_batches_like_the_eager_step's criterion: |a - b| <= 0.05 |a - start|."""
    moved = (want[0] - _start()).norm()
    print(what, "parameters", float((got[0] - want[0]).norm()), "moved", float(moved), "losses", (got[1] - want[1]).abs().max().item())
    assert (got[0] - want[0]).norm() <= 0.05 * moved


def test_eager_trainer_equals_the_hand_fed_loop():
    got, want = _trainer_run("DrugGEN", False), _hand_fed("DrugGEN")
    assert got[1].shape == (EPOCHS * 2, 2)
    _same_step_twice(got, want, "DrugGEN eager")


def test_run_epoch_returns_the_loss_history_and_logs_at_the_boundaries(tmp_path):
    """run_epoch / fit drive the same steps as the hand-stepped trainer above; on_log sees host tensors at every log_every-th
    step and at the end of an epoch, and checkpoints land at the same boundaries."""
    import os
    from druggen_amd.loop import ResidentTrainer
    mols, drugs = _stores()
    G, D, st = _nets()
    tr = ResidentTrainer(st, mols, drugs, batch_size=B, graph=False, seed=SEED, eps=_eps(), log_every=1)
    seen = []
    first = tr.run_epoch()
    second, = tr.fit(1, on_log=lambda e, i, losses: seen.append((e, i, losses)), save_dir=str(tmp_path))
    assert first.is_cuda and first.shape == second.shape == (2, 2) and first.dtype == torch.float32
    _same_step_twice((_flat(G, D), torch.cat([first, second])), _trainer_run("DrugGEN", False), "run_epoch")
    assert [(e, i) for e, i, _ in seen] == [(1, 0), (1, 1)]
    assert all(not l.is_cuda and l.shape == (i + 1, 2) and torch.equal(l, second[:i + 1].cpu()) for _, i, l in seen)
    assert sorted(os.listdir(tmp_path)) == ["2-1-D.ckpt", "2-1-G.ckpt", "2-2-D.ckpt", "2-2-G.ckpt"]


def test_graphed_trainer_tracks_the_eager_trainer():
    _tracks(_trainer_run("DrugGEN", True), _trainer_run("DrugGEN", False), "DrugGEN graphed")


def test_static_inputs_after_every_graphed_step_are_the_batch_of_that_step():
    fresh = _trainer_run("DrugGEN", True)[2]
    assert len(fresh) == EPOCHS * 2 and all(fresh), fresh      # dense buffers AND labels: a stale label buffer shows here


def test_no_target_feeds_the_discriminator_the_molecule_batch():
    eager, graphed, hand = _trainer_run("NoTarget", False), _trainer_run("NoTarget", True), _hand_fed("NoTarget")
    _same_step_twice(eager, hand, "NoTarget eager")
    _tracks(graphed, eager, "NoTarget graphed")
    assert len(graphed[3]) == EPOCHS * 2 and all(graphed[3]) and all(graphed[2])      # D's static inputs == the generator's
    assert not torch.equal(hand[0], _hand_fed("DrugGEN")[0])


@pytest.mark.parametrize("graph", [False, True])
def test_bad_index_surfaces_as_the_stores_error_by_the_end_of_the_epoch(graph):
    from druggen_amd.loop import ResidentTrainer
    mols, drugs = _new_stores()
    G, D, st = _nets()
    tr = ResidentTrainer(st, mols, drugs, batch_size=B, graph=graph, seed=SEED, eps=_eps())
    real = tr.schedule

    def poisoned():
        for k, (mi, di) in enumerate(real()):
            if k == 0:
                mi = mi.clone()
                mi[1] = N_MOL + 3
            yield mi, di
    tr.schedule = poisoned
    with pytest.raises(RuntimeError, match=r"1 bad indices.*outside \[0, 11\)"):
        tr.run_epoch()
    tr.schedule = real
    assert torch.isfinite(_flat(G, D)).all() and not torch.equal(_flat(G, D), _start())      # the step ran on the clamped index
    losses = tr.run_epoch()                                                                 # and the loop goes on, clean
    assert torch.isfinite(losses).all()


@pytest.mark.parametrize("graph", [True, False])
def test_sample_from_equals_sample_on_the_gathered_batch(graph):
    from druggen_amd.decode import _FIELDS
    from druggen_amd.resident import ResidentMolecules
    from druggen_amd.sampling import MoleculeSampler
    mols, _ = _stores()
    G, _, _ = _nets()
    _, a0, x0 = mols.batch(torch.arange(B, device="cuda"))
    sampler = MoleculeSampler(G, a0, x0, graph=graph, bond_order2=[0, 2, 4, 6, 3], warmup=1)
    decoded = []
    for idx in ([7, 1, 10, 0], [2, 2, 9, 5]):      # two in a row: the second replay must not see the first one's labels
        idx = torch.tensor(idx, device="cuda")
        got, got_nodes, got_edges = sampler.sample_from(mols, idx, keep_logits=True)
        got, got_nodes, got_edges = got.cpu(), got_nodes.clone(), got_edges.clone()
        _, a, x = mols.batch(idx)
        want, want_nodes, want_edges = sampler.sample(a, x, keep_logits=True)
        want = want.cpu()
        assert torch.equal(got_nodes, want_nodes) and torch.equal(got_edges, want_edges)
        for name in _FIELDS:
            if name == "bonds":      # rows past n_bonds are unwritten memory
                assert all(np.array_equal(got.edge_list(b), want.edge_list(b)) for b in range(B))
            else:
                assert np.array_equal(getattr(got, name), getattr(want, name)), name
        decoded.append(sampler.sample_from(mols, idx).cpu().atoms.copy())
        assert np.array_equal(decoded[-1], want.atoms)
    assert not np.array_equal(decoded[0], decoded[1])
    other = ResidentMolecules.from_graphs(_graphs(N_MOL, 1), device="cuda", m_dim=M, b_dim=E + 1)
    with pytest.raises(ValueError, match="b_dim=6"):
        sampler.sample_from(other, torch.arange(B, device="cuda"))
    if graph:
        with pytest.raises(ValueError, match="3 indices"):
            sampler.sample_from(mols, torch.arange(3, device="cuda"))
        a, labels, x = sampler.inputs()
        assert a.shape == (B, N, N, E) and labels.dtype == torch.int32 and x.shape == (B, N, M)
    mols.raise_bad_indices(wait=True)


def test_dense_captures_have_no_label_buffer_and_live_dropout_is_refused():
    from druggen_amd.loop import ResidentTrainer
    from druggen_amd.sampling import MoleculeSampler
    from druggen_amd.trainer import GraphedGANStep
    mols, drugs = _stores()
    _, a, x = mols.batch(torch.arange(B, device="cuda"))
    dense = torch.softmax(torch.randn(B, N, N, E, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)), -1)
    G, D, st = _nets()
    with pytest.raises(RuntimeError, match="not one-hot"):
        MoleculeSampler(G, dense, x, warmup=1).inputs()
    with pytest.raises(RuntimeError, match="not one-hot"):
        GraphedGANStep(st, dense, x, dense.clone(), x, warmup=1, eps=_eps()).inputs()
    G, D, st = _nets(dropout=0.1)
    assert G.training and D.training
    with pytest.raises(RuntimeError, match="dropout"):
        ResidentTrainer(st, mols, drugs, batch_size=B, seed=SEED)
    G.eval(), D.eval()      # dropout that is not live captures
    assert ResidentTrainer(st, mols, drugs, batch_size=B, seed=SEED).graphed is not None
