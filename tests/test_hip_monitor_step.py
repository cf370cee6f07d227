"""GPU tests of the step monitor (`monitor.StepMonitor` inside `GANStep`, `GraphedGANStep` and `ResidentTrainer`): the counters
of a step are those of the generated batch the D step sees, watching changes nothing the step computes, a captured step
replays them, and the trainer files one row per step and hands the last batch to `on_monitor`.

Shapes: dim 128, 8 heads, mlp_ratio 3, depth 1; N = 9, E = 5, M = 13; batch 4 of 11 molecules (2 steps per epoch) and 6 drugs."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mol_stats_ref as ref

pytestmark = pytest.mark.gpu

N, E, M, B, N_MOL, N_DRUG = 9, 5, 13, 4, 11, 6
SEED, LR = 3, 2e-3
ORDER2 = (0, 2, 4, 6, 3)
TABLE = (0xFFFF, 2, 4, 6, 8, 2, 4, 6, 8, 2, 4, 6, 8)


@functools.lru_cache(maxsize=None)
def _graphs(n, seed):
    """Synthetic molecules as tests/test_hip_loop.py::_graphs makes them."""
    rng = np.random.default_rng([n, N, M, E, seed])
    upper = np.triu((rng.random((n, N, N)) < 0.1) * rng.integers(1, E, size=(n, N, N)), 1)
    bonds = upper + upper.transpose(0, 2, 1)
    atoms = rng.integers(0, M, size=(n, N))
    graphs = []
    for i in range(n):
        x = np.zeros((N, M), dtype=np.float32)
        x[np.arange(N), atoms[i]] = 1.0
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x, edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    return tuple(graphs)


@functools.lru_cache(maxsize=None)
def _stores():
    from druggen_amd.resident import ResidentMolecules
    return (ResidentMolecules.from_graphs(_graphs(N_MOL, 1), device="cuda", m_dim=M, b_dim=E),
            ResidentMolecules.from_graphs(_graphs(N_DRUG, 2), device="cuda", m_dim=M, b_dim=E))


@functools.lru_cache(maxsize=None)
def _eps():
    from druggen_amd import synth
    return tuple(torch.from_numpy(t).cuda() for t in synth.interpolation_eps(B, 9))


def _generator(dropout=0.0):
    from druggen_amd import synth
    from druggen_amd.model import Generator
    net = Generator("relu", N, E, M, dropout, dim=128, depth=1, heads=8, mlp_ratio=3)
    params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=11)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return net.cuda()


def _nets(dropout=0.0, **step_kw):
    from druggen_amd import synth
    from druggen_amd.model import Discriminator
    from druggen_amd.trainer import GANStep
    G = _generator(dropout)
    D = Discriminator("relu", N, E, M, dropout, dim=128, depth=1, heads=8, mlp_ratio=3)
    params = synth.fill_parameters([(k, v.shape) for k, v in D.state_dict().items()], seed=12)
    D.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    D = D.cuda()
    return G, D, GANStep(G, D, g_lr=LR, d_lr=LR, **step_kw)


def _monitor():
    from druggen_amd.monitor import StepMonitor
    return StepMonitor(bond_order2=ORDER2, max_valence2=TABLE)


def _flat(G, D):
    return torch.cat([p.detach().reshape(-1) for p in list(G.parameters()) + list(D.parameters())]).clone()


def _watch(state, a, x, with_inputs=True, **kw):
    """The counters by hand: a generator of its own with the weights `state`, one forward, the decode, the statistics."""
    from druggen_amd import decode, monitor
    from druggen_amd.functional import as_one_hot, one_hot_labels
    G = _generator()
    G.load_state_dict(state)
    a = as_one_hot(a.clone())
    _, _, ns, es = G(a, x)
    batch = decode.decode_molecule_graphs(ns.detach(), es.detach(), bond_order2=kw.get("bond_order2", ORDER2))
    stats = monitor.molecule_statistics(batch, in_atoms=x.argmax(-1).to(torch.uint8) if with_inputs else None,
                                        in_labels=one_hot_labels(a) if with_inputs else None,
                                        max_valence2=kw.get("max_valence2", TABLE))
    return batch.cpu(), stats.cpu()


def _state(G):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in G.state_dict().items()}


def _fixed_batches():
    mols, drugs = _stores()
    out = []
    for mi, di in (([7, 1, 10, 0], [2, 5, 0, 3]), ([2, 2, 9, 5], [1, 1, 4, 0])):
        _, ma, mx = mols.batch(torch.tensor(mi, device="cuda"))
        _, da, dx = drugs.batch(torch.tensor(di, device="cuda"))
        out.append((da, dx, ma, mx))
    return out


def _same_decode(got, want):
    for b in range(got.B):
        assert np.array_equal(got.edge_list(b), want.edge_list(b))
    for name in ("atoms", "n_bonds", "n_components", "largest_size", "valence2"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


@pytest.mark.parametrize("memory", ["fast", "low"])
def test_monitored_step_counts_the_generated_batch_and_changes_nothing(memory):
    """After a step, `monitor.stats` is `molecule_statistics` of a separate G forward on the PRE-step weights; losses and all
    parameters after two steps are bit-identical to those of a twin without a monitor."""
    mon = _monitor()
    G, D, st = _nets(memory=memory, monitor=mon)
    G2, D2, twin = _nets(memory=memory)
    assert st.monitor is mon and twin.monitor is None
    rows = []
    for da, dx, ma, mx in _fixed_batches():
        decoded, want = _watch(_state(G), ma, mx)
        losses = st.step(da, dx, ma, mx, eps=_eps())
        plain = twin.step(da, dx, ma, mx, eps=_eps())
        assert mon.stats.cpu().tot[0] == B
        got = mon.stats.cpu()
        assert np.array_equal(got.buffer, want.buffer), (got.mol, want.mol)
        _same_decode(mon.decoded.cpu(), decoded)
        mol, tot = ref.mol_stats(ref.molecules_of(mon.decoded.cpu()), in_atoms=mx.argmax(-1).cpu().numpy(),
                                 in_labels=ma.argmax(-1).cpu().numpy(), max_valence2=TABLE)
        assert np.array_equal(got.mol, mol) and np.array_equal(got.tot, tot)
        assert (got.mol[:, 4:7] >= 0).all()      # valence and both inputs were handed over
        assert torch.equal(losses[0], plain[0]) and torch.equal(losses[1], plain[1])
        rows.append(got.tot.copy())
    assert torch.equal(_flat(G, D), _flat(G2, D2))
    assert not torch.equal(_flat(G, D), _flat(*_nets()[:2]))
    # a dense edge batch has no labels: the step runs, the two changed_* columns are not answered
    da, dx, ma, mx = _fixed_batches()[0]
    st.step(da, dx, torch.softmax(3.0 * ma, -1), mx, eps=_eps())
    got = mon.stats.cpu()
    assert got.B == B and (got.mol[:, 5:7] == -1).all() and (got.mol[:, 4] >= 0).all() and got.total("n_copies") == 0


def test_graphed_step_replays_the_counters_of_the_eager_monitored_step():
    """The decode and the statistics are part of the captured step: every replay rewrites `monitor.stats` with the counters
    the eager route gives for that batch and those weights -- one graph, no side stream."""
    from druggen_amd.trainer import GraphedGANStep
    batches = _fixed_batches()
    mon = _monitor()
    G, D, st = _nets(monitor=mon)
    graphed = GraphedGANStep(st, *batches[0], warmup=2, eps=_eps())
    assert graphed.segments is None      # one process: ONE graph, the two calls are in it
    seen = []
    for da, dx, ma, mx in batches[1:] + batches:
        state = _state(G)
        mon.stats.buffer.fill_(0xFF)
        mon.decoded.buffer.fill_(0xEE)
        graphed.step(da, dx, ma, mx, eps=_eps())
        got = mon.stats.cpu()
        decoded, want = _watch(state, ma, mx)
        assert np.array_equal(got.buffer, want.buffer), (got.mol, want.mol)
        _same_decode(mon.decoded.cpu(), decoded)
        # ... and of an eager monitored step from the same weights on the same batch
        other = _monitor()
        G2, D2, eager = _nets(monitor=other)
        G2.load_state_dict(state)
        eager.step(da, dx, ma, mx, eps=_eps())
        assert np.array_equal(other.stats.cpu().buffer, got.buffer)
        seen.append(got.mol.copy())
    assert not np.array_equal(seen[0], seen[1])


def test_segmented_capture_counts_inside_its_first_graph():
    """Captured as under a process group (three graphs cut at the two gradient all-reduces): the decode and the statistics are
    nodes of the FIRST graph -- replaying it alone rewrites the counters -- and a whole replay gives the eager counters."""
    from druggen_amd.trainer import GraphedGANStep
    batches = _fixed_batches()
    mon = _monitor()
    G, D, st = _nets(monitor=mon)
    graphed = GraphedGANStep(st, *batches[0], warmup=2, eps=_eps(), segmented=True)
    graphs, flats = graphed.segments
    assert len(graphs) == 3 and len(flats) == 2
    da, dx, ma, mx = batches[1]
    state = _state(G)
    graphed.step(da, dx, ma, mx, eps=_eps())
    _, want = _watch(state, ma, mx)
    assert np.array_equal(mon.stats.cpu().buffer, want.buffer)
    state = _state(G)
    mon.stats.buffer.fill_(0xFF)
    graphs[0].replay()                      # generator forward, D loss and backward: the monitor's two calls are in here
    got = mon.stats.cpu()
    graphs[1].replay()                      # the rest of the iteration (no process group: nothing to reduce in between)
    graphs[2].replay()
    from druggen_amd.functional import bump_weights_epoch
    bump_weights_epoch()                    # as GraphedGANStep.replay does: the graphs rewrote the weights in place
    _, want = _watch(state, ma, mx)
    assert np.array_equal(got.buffer, want.buffer) and np.array_equal(mon.stats.cpu().buffer, got.buffer)


@functools.lru_cache(maxsize=None)
def _trainer_run(submodel, graph):
    """Two epochs of ResidentTrainer(monitor=True) with log_every=1: what on_log and on_monitor saw, the per-epoch totals."""
    from druggen_amd.loop import ResidentTrainer
    mols, drugs = _stores()
    G, D, st = _nets()
    tr = ResidentTrainer(st, mols, drugs if submodel == "DrugGEN" else None, batch_size=B, submodel=submodel, graph=graph,
                         seed=SEED, eps=_eps(), log_every=1, monitor=True)
    assert st.monitor is tr.monitor and tr.monitor is not None and tr.steps_per_epoch == 2
    logs, seen, totals = [], [], []
    for _ in range(2):
        tr.run_epoch(on_log=lambda e, i, losses: logs.append((e, i, tuple(losses.shape))),
                     on_monitor=lambda e, i, t, d: seen.append((e, i, t, d)))
        totals.append(tr.monitor_totals.cpu().clone())
    return logs, seen, totals


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
@pytest.mark.parametrize("submodel", ["DrugGEN", "NoTarget"])
def test_trainer_files_one_row_per_step_and_hands_over_the_last_batch(submodel, graph):
    from druggen_amd.decode import MoleculeBatch
    from druggen_amd.schedule import epoch_schedule
    logs, seen, totals = _trainer_run(submodel, graph)
    # on_monitor fires at exactly the boundaries where on_log fires
    assert [(e, i) for e, i, _ in logs] == [(e, i) for e, i, _, _ in seen] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    mols, _ = _stores()
    g = torch.Generator(device="cuda").manual_seed(SEED)
    schedule = [mi for _ in range(2) for mi, _ in epoch_schedule(N_MOL, N_DRUG if submodel == "DrugGEN" else None, B,
                                                                 generator=g, device="cuda")]
    for k, (e, i, rows, decoded) in enumerate(seen):
        assert not rows.is_cuda and rows.dtype == torch.int64 and rows.shape == (i + 1, 16)
        assert torch.equal(rows, totals[e][:i + 1])              # each history row is that step's counters
        assert isinstance(decoded, MoleculeBatch) and decoded.is_host and (decoded.B, decoded.N) == (B, N)
        # the host batch of the last step reproduces the last row through the numpy restatement, inputs included
        _, a, x = mols.batch(schedule[k])
        _, tot = ref.mol_stats(ref.molecules_of(decoded), in_atoms=x.argmax(-1).cpu().numpy(),
                               in_labels=a.argmax(-1).cpu().numpy())
        assert rows[i].tolist() == tot.tolist(), (k, rows[i].tolist(), tot.tolist())
        assert int(rows[i, 0]) == B and int(rows[i, 6]) >= 0 and int(rows[i, 7]) >= 0 and int(rows[i, 5]) == 0      # no tables: -1s
    assert all(t.shape == (2, 16) for t in totals)


def test_first_step_counters_agree_between_the_graphed_and_the_eager_trainer():
    """Both routes start from the same weights (the capture's warm-up is undone) and draw the same schedule."""
    for submodel in ("DrugGEN", "NoTarget"):
        assert torch.equal(_trainer_run(submodel, True)[2][0][0], _trainer_run(submodel, False)[2][0][0])


def test_monitor_off_allocates_and_files_nothing():
    from druggen_amd.loop import ResidentTrainer
    mols, drugs = _stores()
    G, D, st = _nets()
    tr = ResidentTrainer(st, mols, drugs, batch_size=B, graph=False, seed=SEED, eps=_eps())
    called = []
    tr.run_epoch(on_monitor=lambda *a: called.append(a))
    assert st.monitor is None and tr.monitor is None and tr.monitor_totals is None and not called


def test_steps_that_cannot_hand_over_the_logits_refuse_a_monitor():
    from druggen_amd.loop import ResidentTrainer
    from druggen_amd.model.loss import discriminator_loss, generator_loss
    mols, drugs = _stores()
    with pytest.raises(ValueError, match="custom d_loss_fn / g_loss_fn"):
        _nets(monitor=_monitor(), d_loss_fn=lambda *a, **k: discriminator_loss(*a, **k))
    with pytest.raises(ValueError, match="custom d_loss_fn / g_loss_fn"):
        _nets(monitor=_monitor(), g_loss_fn=lambda *a, **k: generator_loss(*a, **k))
    with pytest.raises(ValueError, match="dropout > 0"):
        _nets(dropout=0.1, monitor=_monitor())
    with pytest.raises(ValueError, match="share_generator_forward"):
        _nets(monitor=_monitor(), share_generator_forward=False)
    G, D, st = _nets(dropout=0.1)
    with pytest.raises(ValueError, match="dropout > 0"):
        ResidentTrainer(st, mols, drugs, batch_size=B, graph=False, seed=SEED, monitor=True)
    assert st.monitor is None
    G.eval()      # dropout that is not live: watched
    mon = _monitor()
    st.set_monitor(mon)
    da, dx, ma, mx = _fixed_batches()[0]
    st.step(da, dx, ma, mx, eps=_eps())
    assert mon.stats.cpu().total("B") == B
    G.train()     # switched on after the monitor was attached: the step says so
    with pytest.raises(RuntimeError, match="no shared forward to watch"):
        st.step(da, dx, ma, mx, eps=_eps())
