"""Per-step statistics of the generated batch on the GPU: the part of the reference's ``logging()`` (``src/util/utils.py:241-355``)
that is integer arithmetic on the decoded labels, so that it can run inside every training step instead of every
``log_sample_step``-th.

``molecule_statistics`` turns a device ``decode.MoleculeBatch`` into ``MolStats`` with one call of ``dg_mol_stats``
(``include/druggen_hip.h``); ``StepMonitor`` owns the static buffers ``GANStep(monitor=...)`` decodes and counts into.
Canonical SMILES, RDKit validity and fingerprints stay with the caller (``smiles.py``, ``metrics.py``).  GPU only, no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._packed import PackedRecord, check_key_bits, uploaded
from .decode import MoleculeBatch, decode_molecule_graphs, device_batch
from .functional import _c

__all__ = ["molecule_statistics", "MolStats", "StepMonitor", "fractions_of", "MOL_COLUMNS", "TOT_FIELDS"]

MOL_COLUMNS = ("atom_types", "largest_size", "n_components", "n_bonds", "over_valent", "changed_atoms", "changed_bonds",
               "duplicate_of")
TOT_FIELDS = ("B", "atom_types", "largest_size", "n_components", "n_bonds", "over_valent", "changed_atoms", "changed_bonds",
              "n_over_valent", "n_copies", "n_distinct", "n_truncated", "n_connected")


class MolStats(PackedRecord):
    """Statistics of one decoded batch: typed views of one packed byte buffer (``tot`` first, then ``mol``).

    ``mol`` [B,8] int32, one row per molecule (``MOL_COLUMNS``); a column is -1 where the input it needs was not given:

    ===  =================  ============================================================================================
    0    ``atom_types``     distinct values in ``atoms[b, :]``; the pad label counts, as ``i.unique()`` does in the
                            reference's ``Metrics.mean_atom_type`` (``utils.py:112-127``)
    1-3  ``largest_size``, ``n_components``, ``n_bonds``   copied from the decode
    4    ``over_valent``    positions with ``valence2[b,i] > max_valence2[atoms[b,i]]``
    5    ``changed_atoms``  positions with ``atoms[b,i] != in_atoms[b,i]``
    6    ``changed_bonds``  pairs ``i > j`` whose decoded bond label (0: not in the list) differs from ``in_labels[b,i,j]``
    7    ``duplicate_of``   smallest ``j < b`` with the same atoms row, ``n_bonds`` and bond list; -1: none
    ===  =================  ============================================================================================

    A truncated molecule (``n_bonds > cap``) has ``changed_bonds = -1`` and ``duplicate_of = -2`` and is nobody's duplicate.

    ``tot`` [16] int64 (``TOT_FIELDS``): B; the sums of columns 0-6 over their entries >= 0; the molecules with ``over_valent >
    0``; ``n_copies`` (both ``changed_*`` are 0); ``n_distinct`` (``duplicate_of == -1``); ``n_truncated``; ``n_connected``
    (``n_components == 1``); zeros.

    How the fractions below relate to the reference's curves:

    * ``atom_types_mean`` IS the reference's ``Atom_types``.
    * ``main_fragment_fraction`` is the analogue of ``MaxLen``: it counts the ATOMS of the largest fragment over N, where the
      reference counts the LETTERS of the largest fragment's SMILES string over a fixed length.  Same trend, different unit.
    * Identity here is positional: two identical decoded graphs are certainly the same molecule, but the same molecule with its
      atoms in another order is not recognised.  So ``1 - distinct_fraction`` is a LOWER BOUND on the duplication RDKit's
      ``Uniqueness`` would report, and ``copy_fraction`` is a LOWER BOUND on the share of molecules that are not novel with
      respect to their own input.  Both are alarms for the two failures of this GAN (collapse to a few outputs; the generator
      returning its input); neither replaces RDKit's Uniqueness or Novelty.  Identity up to the atom order, within the batch
      and against a stock of molecules, is ``druggen_amd.canon``'s, on the same ``MoleculeBatch``.

    ``cpu()`` moves the packed buffer with ONE device->host copy; the fractions read the host copy."""

    TOT_FIELDS = TOT_FIELDS

    def __init__(self, buffer, B, N):
        self.B, self.N, self._workspace = B, N, None
        super().__init__(buffer, B, N)

    @staticmethod
    def _fields(B, N):
        return ("tot", 8, (16,)), ("mol", 4, (B, 8))

    @staticmethod
    def empty(B, N, device):
        """Device statistics over an uninitialised buffer (``molecule_statistics(..., out=)`` fills it), with the key workspace
        of ``dg_mol_stats``."""
        stats = MolStats._empty(device, B, N)
        stats._workspace = torch.empty(max(B, 1), dtype=torch.int64, device=device)
        return stats

    def cpu(self):
        host = super().cpu()
        if host is not self:
            host._workspace = None      # the key workspace stays on the device
        return host

    def column(self, name):
        return self.mol[:, MOL_COLUMNS.index(name)]

    def _over_b(self, name):
        return self.total(name) / self.B if self.B else float("nan")

    @property
    def atom_types_mean(self):
        """``sum(atom_types) / B - 1``: exactly the reference's ``Atom_types``."""
        return self._over_b("atom_types") - 1

    @property
    def main_fragment_fraction(self):
        """``sum(largest_size) / (B N)``: atoms of the main fragment (the reference's ``MaxLen`` counts SMILES letters)."""
        return self._over_b("largest_size") / self.N

    @property
    def distinct_fraction(self):
        return self._over_b("n_distinct")

    @property
    def copy_fraction(self):
        return self._over_b("n_copies")

    @property
    def over_valent_fraction(self):
        return self._over_b("n_over_valent")


def fractions_of(totals, N):
    """The five fractions from a row of ``tot`` (e.g. a row of ``ResidentTrainer``'s per-step history) as a dict."""
    t = [int(v) for v in totals]
    B = t[0]
    if B == 0:
        return dict.fromkeys(("atom_types_mean", "main_fragment_fraction", "distinct_fraction", "copy_fraction",
                              "over_valent_fraction"), float("nan"))
    return {"atom_types_mean": t[1] / B - 1, "main_fragment_fraction": t[2] / (B * N), "distinct_fraction": t[10] / B,
            "copy_fraction": t[9] / B, "over_valent_fraction": t[8] / B}


def _valence_table(max_valence2, device):
    """``max_valence2`` as a contiguous uint16 device tensor (a host sequence is uploaded once)."""
    if max_valence2 is None:
        return None
    if torch.is_tensor(max_valence2):
        t = max_valence2
        if t.dtype != torch.uint16:
            raise ValueError(f"max_valence2 must be a uint16 tensor (0xFFFF: no limit), got {t.dtype}")
        if t.device != device:
            t = t.to(device)
    else:
        vals = tuple(int(v) for v in max_valence2)
        if any(v < 0 or v > 0xFFFF for v in vals):
            raise ValueError("max_valence2 holds twice the largest allowed valence per atom label as uint16 (0xFFFF: no limit)")
        t = uploaded(vals, np.uint16, device)
    if t.dim() != 1 or not 1 <= t.shape[0] <= 256:
        raise ValueError(f"max_valence2 needs one entry per atom label (1..256), got shape {tuple(t.shape)}")
    return _c(t)


def molecule_statistics(batch, *, in_atoms=None, in_labels=None, max_valence2=None, key_bits=64, out=None):
    """``MolStats`` of a device ``MoleculeBatch`` (``decode.decode_molecule_graphs``), on its device and the current stream.

    ``in_atoms`` [B,N] uint8 and ``in_labels`` [B,N,N] int32: the graph the batch was generated from (the static label buffer of
    ``ResidentMolecules.batch`` / ``GraphedGANStep``) -- ask for ``changed_atoms`` / ``changed_bonds``.  ``max_valence2``: twice
    the largest allowed valence per atom label (sequence or uint16 tensor; 0xFFFF = no limit, which the caller sets for the pad
    label 0) -- with a batch decoded with ``bond_order2`` asks for ``over_valent``.  ``key_bits`` (1..64): width of the keys that
    select candidate duplicates; every key match is verified byte by byte, so the result does not depend on it.  ``out``: a
    ``MolStats.empty(B, N, device)`` to write into.  Every element of ``mol`` and ``tot`` is written by every call; nothing is
    allocated with ``out=`` and nothing synchronises, so the call can be captured into a hipGraph."""
    device_batch(batch, "molecule_statistics", "monitor")
    check_key_bits(key_bits)
    B, N, cap = batch.B, batch.N, batch.cap
    dev = batch.buffer.device
    for name, t, shape, dtype in (("in_atoms", in_atoms, (B, N), torch.uint8), ("in_labels", in_labels, (B, N, N), torch.int32)):
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"druggen_amd.monitor runs on the GPU (no CPU fallback): {name} is not a device tensor")
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev:
            raise ValueError(f"{name} must be a {dtype} tensor of shape {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on "
                             f"{t.device}")
    in_atoms = None if in_atoms is None else _c(in_atoms)
    in_labels = None if in_labels is None else _c(in_labels)
    table = _valence_table(max_valence2, dev)
    if out is None:
        out = MolStats.empty(B, N, dev)
    elif (not isinstance(out, MolStats) or out.is_host or (out.B, out.N) != (B, N) or out.buffer.device != dev
            or out._workspace is None):
        raise ValueError("out= must be a device MolStats of this batch's B and N (MolStats.empty)")
    work = out._workspace
    _lib.launch("dg_mol_stats", batch.buffer, batch.atoms.data_ptr(), batch.bonds.data_ptr() if cap > 0 else None,
                batch.n_bonds.data_ptr(), batch.n_components.data_ptr(), batch.largest_size.data_ptr(),
                None if batch.valence2 is None else batch.valence2.data_ptr(),
                None if in_atoms is None else in_atoms.data_ptr(), None if in_labels is None else in_labels.data_ptr(),
                None if table is None else table.data_ptr(), B, N, cap, 0 if table is None else table.shape[0],
                key_bits, out.mol.data_ptr(), out.tot.data_ptr(), work.data_ptr(), work.numel() * 8)
    return out


class StepMonitor:
    """What ``GANStep(monitor=...)`` needs to watch the generated batch of every step: the decode's options and two static
    buffers, ``decoded`` (``MoleculeBatch``) and ``stats`` (``MolStats``), allocated at the first step for its (B, N) and written in
    place by every later one -- a captured step (``GraphedGANStep``) replays into them.

    ``bond_order2`` / ``bond_cap``: as for ``decode_molecule_graphs``; ``max_valence2``: as for ``molecule_statistics`` (the
    ``over_valent`` column needs both tables)."""

    def __init__(self, bond_order2=None, max_valence2=None, bond_cap=None):
        self.bond_order2 = None if bond_order2 is None else tuple(int(v) for v in bond_order2)
        self.max_valence2 = max_valence2 if max_valence2 is None or torch.is_tensor(max_valence2) else tuple(
            int(v) for v in max_valence2)
        self.bond_cap = None if bond_cap is None else int(bond_cap)
        self.decoded = None
        self.stats = None
        self._in_atoms = None

    def _buffers(self, B, N, device):
        cap = N * (N - 1) // 2 if self.bond_cap is None else self.bond_cap
        d = self.decoded
        if d is None or (d.B, d.N, d.cap) != (B, N, cap) or d.buffer.device != device:
            self.decoded = MoleculeBatch.empty(B, N, cap, self.bond_order2 is not None, device)
            self.stats = MolStats.empty(B, N, device)
            self._in_atoms = torch.empty(B, N, dtype=torch.uint8, device=device)

    def observe(self, node_sample, edge_sample, in_node=None, in_labels=None):
        """Decode the generator's logits into ``decoded`` and count into ``stats``: two calls on the current stream.  ``in_node``
        [B,N,M] (one-hot atom matrix of the input graph) and ``in_labels`` [B,N,N] int32: both or neither."""
        B, N, M = node_sample.shape
        self._buffers(B, N, node_sample.device)
        decode_molecule_graphs(node_sample, edge_sample, bond_order2=self.bond_order2, bond_cap=self.bond_cap, out=self.decoded)
        in_atoms = None
        if in_node is not None and in_labels is not None and tuple(in_node.shape) == (B, N, M) and B > 0:
            x = _c(in_node.detach())
            if x.dtype != torch.float32:
                x = x.float()
            in_atoms = self._in_atoms      # gen_node.argmax(-1) as uint8 (first maximum)
            _lib.launch("dg_argmax_decode", x, _lib.ptr(x), B * N, M, in_atoms.data_ptr())
        else:
            in_labels = None
        return molecule_statistics(self.decoded, in_atoms=in_atoms, in_labels=in_labels, max_valence2=self.max_valence2,
                                   out=self.stats)
