"""Which molecules enter which step: the index schedule of the reference's training loop (``train.py:302-345``) as int64
index tensors, for stores that are addressed by index (``resident.ResidentMolecules``).

The reference iterates a molecule ``DataLoader`` and a drug ``DataLoader``, both ``shuffle=True, drop_last=True``
(``train.py:97-115``):

* molecules: one permutation per epoch, ``n_mol // batch_size`` steps, the remainder dropped;
* drugs: a new iterator -- a new permutation -- at the start of every epoch (``train.py:307``) and again whenever the
  current one is exhausted (``train.py:312-316``), i.e. when fewer than ``batch_size`` indices of it remain;
* ``NoTarget`` has no drug set: the discriminator sees the molecule batch (``train.py:343-345``).

Pure index arithmetic on ``torch.randperm``: runs on the CPU and on the GPU, no kernel, no host synchronisation."""
from __future__ import annotations

import torch

from .resident import epoch_batches

__all__ = ["epoch_schedule"]


def epoch_schedule(n_mol: int, n_drug, batch_size: int, *, generator, device, world: int = 1, rank: int = 0):
    """Iterator over ONE epoch: ``(mol_idx, drug_idx)`` int64 tensors ``[batch_size // world]`` on ``device``, ``n_mol //
    batch_size`` of them.  Call it once per epoch with the same ``generator``; the draws of an epoch are, in the reference's
    order, the drug permutation, the molecule permutation, then one drug permutation per restart.

    ``n_drug=None`` (``NoTarget``): ``drug_idx is mol_idx``.  Data parallel: every rank passes the same seed and device
    type, draws the same permutations and takes rows ``[rank * b, (rank + 1) * b)``, ``b = batch_size // world``, of each
    global batch.  ``ValueError`` -- before anything is drawn -- when ``batch_size`` is not a multiple of ``world`` or a set
    is smaller than one batch."""
    n_mol, batch_size, world, rank = int(n_mol), int(batch_size), int(world), int(rank)
    n_drug = None if n_drug is None else int(n_drug)
    if batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_schedule: batch_size {batch_size}, world {world}, rank {rank}")
    if batch_size % world:
        raise ValueError(f"epoch_schedule: batch_size {batch_size} is not a multiple of the {world} ranks")
    if n_mol < batch_size:
        raise ValueError(f"epoch_schedule: {n_mol} molecules do not fill one batch of {batch_size}")
    if n_drug is not None and n_drug < batch_size:
        raise ValueError(f"epoch_schedule: {n_drug} drugs do not fill one batch of {batch_size}")
    return _epoch(n_mol, n_drug, batch_size, generator, device, batch_size // world, rank)


def _epoch(n_mol, n_drug, batch_size, generator, device, per_rank, rank):
    def permutation(n):
        return torch.randperm(n, generator=generator, device=device)

    rows = slice(rank * per_rank, (rank + 1) * per_rank)
    drugs = None if n_drug is None else epoch_batches(permutation(n_drug), batch_size)      # train.py:307
    for mol in epoch_batches(permutation(n_mol), batch_size):
        mol = mol[rows]
        if drugs is None:
            yield mol, mol
            continue
        drug = next(drugs, None)
        if drug is None:                                                                     # train.py:314-316
            drugs = epoch_batches(permutation(n_drug), batch_size)
            drug = next(drugs)
        yield mol, drug[rows]
