"""The training loop over GPU-resident molecule sets: the reference's ``train.py:302-397`` without its host feed.

Every step of the reference collates two PyG batches on the host, sends eight tensors over PCIe, densifies them and calls
``.item()`` twice.  ``ResidentTrainer`` draws the same index schedule (``schedule.epoch_schedule``), builds both batches on the
device with one ``dg_mol_gather`` each (``resident.ResidentMolecules.batch``) and keeps the losses on the device:

    mols, drugs = ResidentMolecules.from_graphs(mol_graphs), ResidentMolecules.from_graphs(drug_graphs)
    trainer = ResidentTrainer(GANStep(G, D), mols, drugs, batch_size=128, log_every=100)
    trainer.fit(epochs, on_log=lambda epoch, step, losses: print(epoch, step, losses[-1]), save_dir="models")

``graph=True`` (the default) captures the step once (``trainer.GraphedGANStep``); a step is then the gathers, written straight
into the static inputs of the capture, and a replay -- the gathers sit on the replay's stream, in front of the graph.
``graph=False`` runs ``GANStep.step`` on the gathered batches.  GPU only, no CPU fallback."""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import checkpoint
from .functional import attach_one_hot_labels, bump_weights_epoch
from .optim import FlatAdamW
from .schedule import epoch_schedule
from .trainer import GANStep, GraphedGANStep

__all__ = ["ResidentTrainer"]


def _live_dropout(module) -> bool:
    return bool(module.training) and float(getattr(module, "dropout", 0.0) or 0.0) > 0.0


class _TrainingState:
    """Parameters and AdamW state of a ``GANStep`` as they are NOW, to put back after ``GraphedGANStep``'s warm-up: its
    warm-up iterations are real optimizer steps on the capture batch, and a loop must start from the weights it was given."""

    def __init__(self, stepper: GANStep):
        self.stepper = stepper
        self.params = [(p, p.detach().clone()) for net in (stepper.G, stepper.D) for p in net.parameters()]
        self.opts = []
        for opt in (stepper.d_optimizer, stepper.g_optimizer):
            built = opt.flat_param is not None
            self.opts.append((opt, opt.step_count, list(opt._live) if built else None,
                              (opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.device_step.clone()) if built else None))

    def restore(self):
        with torch.no_grad():
            for p, saved in self.params:
                p.copy_(saved)      # in place: FlatAdamW has re-pointed the parameters into its flat buffer by now
            for opt, count, live, saved in self.opts:
                opt.step_count = count
                if saved is None:      # first built during the warm-up: a fresh AdamW
                    opt.exp_avg.zero_()
                    opt.exp_avg_sq.zero_()
                    opt.device_step.zero_()
                elif live == opt._live:
                    for dst, src in zip((opt.exp_avg, opt.exp_avg_sq, opt.device_step), saved):
                        dst.copy_(src)
                else:
                    raise RuntimeError("ResidentTrainer: the set of parameters that receive a gradient changed during the "
                                       "capture warm-up; build the trainer on a fresh GANStep")
        self.stepper.reset_grad()
        bump_weights_epoch()      # the parameters were rewritten in place: no pack of the warm-up's weights is reused


class ResidentTrainer:
    """``ResidentTrainer(stepper, molecules, drugs=None, *, batch_size, submodel="DrugGEN", graph=True, seed=0, eps=None,
    log_every=None)`` -- ``molecules`` / ``drugs``: ``ResidentMolecules`` on the stepper's device with the same ``(N, m_dim,
    b_dim, atom_dim)``.  ``submodel="DrugGEN"`` feeds the discriminator drug batches, ``"NoTarget"`` the molecule batch (one gather
    serves both sides, ``train.py:340-345``).

    ``batch_size`` is the GLOBAL batch: under a process group (``stepper.group``) every rank holds the whole set, draws the
    same schedule from ``seed`` and gathers its ``batch_size // world`` rows.  ``eps=(eps_edge [b,1,1,1], eps_node [b,1,1])``
    fixes the gradient penalty's interpolation weights (reproducible runs, tests).

    Losses are written into a ``[steps, 2]`` device tensor per epoch (``d_loss``, ``g_loss`` per row) and read on the host only
    every ``log_every`` steps and at the end of an epoch; nothing in a step synchronises with the host.  An index outside a
    store is clamped on the device by the gather and raised as the store's ``RuntimeError`` at the next such boundary.

    The graphed route refuses live dropout (the captured step shares one generator forward between the D and the G step) and
    restores the weights and the AdamW state after the capture's warm-up iterations, so both routes start from the weights
    they were given.

    ``monitor=`` a ``monitor.StepMonitor`` or ``True`` (a default one; the stepper's own if it has one): every step decodes the
    generated batch and counts its statistics on the device (``GANStep.set_monitor``), and one device-side copy per step files
    ``MolStats.tot`` into an ``[steps, 16]`` int64 device tensor per epoch (``monitor_totals``: the running epoch's, then the last
    one's) beside the loss history.  ``fit`` / ``run_epoch`` hand it to ``on_monitor`` at the boundaries where ``on_log`` fires.
    Under a process group each rank watches its own shard: duplicates are counted within the shard and no collective is added.
    ``monitor=None``: nothing is allocated or launched."""

    def __init__(self, stepper: GANStep, molecules, drugs=None, *, batch_size: int, submodel: str = "DrugGEN",
                 graph: bool = True, seed: int = 0, eps=None, log_every=None, monitor=None):
        if submodel not in ("DrugGEN", "NoTarget"):
            raise ValueError(f"submodel must be 'DrugGEN' or 'NoTarget', got {submodel!r}")
        if submodel == "DrugGEN" and drugs is None:
            raise ValueError("submodel='DrugGEN' trains the discriminator on drug batches: pass drugs= (or submodel='NoTarget')")
        if submodel == "NoTarget":
            drugs = None
        if log_every is not None and int(log_every) < 1:
            raise ValueError(f"log_every must be positive, got {log_every}")
        self.stepper, self.molecules, self.drugs = stepper, molecules, drugs
        self.submodel, self.eps = submodel, eps
        self.log_every = None if log_every is None else int(log_every)
        self.device = molecules.device
        for store in self.stores[1:]:
            if any(getattr(store, k) != getattr(molecules, k) for k in ("vertexes", "m_dim", "b_dim", "atom_dim", "device")):
                raise ValueError("ResidentTrainer: molecules and drugs must share N, m_dim, b_dim, atom_dim and the device")
        group = stepper.group
        on = dist.is_available() and dist.is_initialized()
        self.world, self.rank = (dist.get_world_size(group), dist.get_rank(group)) if on else (1, 0)
        self.batch_size = int(batch_size)
        n_drug = None if drugs is None else len(drugs)
        epoch_schedule(len(molecules), n_drug, self.batch_size, generator=None, device=self.device, world=self.world,
                       rank=self.rank)      # its ValueErrors, now (an iterator that is never started draws nothing)
        self.steps_per_epoch = len(molecules) // self.batch_size
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))
        self.epoch = 0
        b, N, M, E = self.batch_size // self.world, molecules.vertexes, molecules.m_dim, molecules.b_dim
        self.graphed = None
        if monitor is True:
            from .monitor import StepMonitor
            monitor = stepper.monitor if stepper.monitor is not None else StepMonitor()
        if monitor is not None and monitor is not stepper.monitor:
            stepper.set_monitor(monitor)      # before the capture: the decode and the statistics are part of the graph
        self.monitor = monitor
        self.monitor_totals = None
        if graph:
            if _live_dropout(stepper.G) or _live_dropout(stepper.D):
                raise RuntimeError("ResidentTrainer(graph=True): a model is training with dropout > 0 and the captured step "
                                   "shares one generator forward between the D and the G step; use graph=False")
            if not (isinstance(stepper.d_optimizer, FlatAdamW) and isinstance(stepper.g_optimizer, FlatAdamW)):
                raise RuntimeError("ResidentTrainer(graph=True) needs GANStep's flat optimizer (optimizer='auto' or 'flat')")
            first = torch.arange(b, device=self.device)      # batch 0: the shapes to capture at (both sets hold >= b)
            _, gen_a, gen_x = molecules.batch(first)
            _, disc_a, disc_x = (None, gen_a, gen_x) if drugs is None else drugs.batch(first)
            state = _TrainingState(stepper)
            self.graphed = GraphedGANStep(stepper, disc_a, disc_x, gen_a, gen_x, eps=eps)
            state.restore()
            self._disc, self._gen = self.graphed.inputs()
        else:
            def triple():
                return (torch.empty(b, N, N, E, device=self.device), torch.empty(b, N, N, dtype=torch.int32, device=self.device),
                        torch.empty(b, N, M, device=self.device))
            self._gen = triple()
            self._disc = self._gen if drugs is None else triple()

    @property
    def stores(self):
        return (self.molecules,) if self.drugs is None else (self.molecules, self.drugs)

    def schedule(self):
        """This rank's ``(mol_idx, drug_idx)`` of the next epoch (``schedule.epoch_schedule`` on the trainer's generator)."""
        return epoch_schedule(len(self.molecules), None if self.drugs is None else len(self.drugs), self.batch_size,
                              generator=self.generator, device=self.device, world=self.world, rank=self.rank)

    def step(self, mol_idx, drug_idx=None):
        """One iteration on the molecules ``mol_idx`` (and the drugs ``drug_idx``): ``(d_loss, g_loss)`` device scalars."""
        self.molecules.batch(mol_idx, out=self._gen)
        if self.drugs is not None:
            self.drugs.batch(drug_idx, out=self._disc)
        elif self._disc is not self._gen:      # NoTarget, graphed: the capture owns two sets of buffers
            for dst, src in zip(self._disc, self._gen):
                dst.copy_(src)
            attach_one_hot_labels(self._disc[0], self._disc[1])
        if self.graphed is not None:
            return self.graphed.replay()
        return self.stepper.step(self._disc[0], self._disc[2], self._gen[0], self._gen[2], eps=self.eps)

    def _raise_bad_indices(self, wait=False):
        for store in self.stores:
            store.raise_bad_indices(wait=wait)

    def run_epoch(self, on_log=None, save_dir=None, on_monitor=None):
        """One epoch; returns its ``[steps, 2]`` float32 device tensor of ``(d_loss, g_loss)``.  ``on_log`` / ``save_dir`` /
        ``on_monitor``: see ``fit``."""
        epoch, steps = self.epoch, self.steps_per_epoch
        history = torch.zeros(steps, 2, dtype=torch.float32, device=self.device)
        if self.monitor is not None:
            self.monitor_totals = torch.zeros(steps, 16, dtype=torch.int64, device=self.device)
        for i, (mol_idx, drug_idx) in enumerate(self.schedule()):
            torch.stack(self.step(mol_idx, drug_idx), out=history[i])
            if self.monitor is not None:
                self.monitor_totals[i].copy_(self.monitor.stats.tot)
            if self.log_every is not None and (i + 1) % self.log_every == 0 and i + 1 < steps:
                self._boundary(epoch, i, history, on_log, save_dir, on_monitor)
        self.epoch += 1
        self._raise_bad_indices(wait=True)
        self._boundary(epoch, steps - 1, history, on_log, save_dir, on_monitor)
        return history

    def _boundary(self, epoch, i, history, on_log, save_dir, on_monitor=None):
        self._raise_bad_indices()
        if on_log is not None:
            on_log(epoch, i, history[:i + 1].cpu())
        if on_monitor is not None and self.monitor is not None:
            on_monitor(epoch, i, self.monitor_totals[:i + 1].cpu(), self.monitor.decoded.cpu())
        if save_dir is not None and self.rank == 0:
            checkpoint.save_model(self.stepper.G, self.stepper.D, save_dir, epoch, i)

    def fit(self, epochs: int, on_log=None, save_dir=None, on_monitor=None):
        """``epochs`` epochs.  Every ``log_every`` steps and at the end of each epoch: ``on_log(epoch, step, losses_so_far)``
        with the epoch's losses so far as a host tensor ``[step + 1, 2]``, and with ``save_dir`` a checkpoint in the
        reference's format (``checkpoint.save_model``, rank 0; ``train.py:386-397``).  With ``monitor=``, at the same boundaries:
        ``on_monitor(epoch, step, totals_host, decoded_host)`` -- the epoch's ``MolStats.tot`` rows so far as a host tensor
        ``[step + 1, 16]`` (``monitor.TOT_FIELDS``, ``monitor.fractions_of``) and the host ``MoleculeBatch`` of step ``step``, the
        batch the last row counts (for RDKit on exactly those molecules).  Returns the per-epoch loss tensors."""
        return [self.run_epoch(on_log, save_dir, on_monitor) for _ in range(int(epochs))]
