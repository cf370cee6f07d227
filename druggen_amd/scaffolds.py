"""Murcko-style scaffolds and ring systems of decoded molecules, cut out on the GPU (``dg_mol_scaffold``,
``include/druggen_hip_scaf.h``), and the scaffold similarity of two sets of molecules (the reference's
``compute_scaffolds`` / ``ScafMetric`` / ``cos_similarity``, ``src/util/utils.py``) without a device->host copy of the molecules and
without RDKit.  The consumer of ``descriptors.describe_molecules``' ``atom_key`` and ``bond_class``.

The scaffold of a molecule comes back as a second device ``decode.MoleculeBatch`` (``MoleculeScaffolds.batch``), so every tool
that reads a decoded batch -- ``canon.canonical_forms``, ``smiles_out.write_smiles``, ``fingerprint`` ... -- works on scaffolds
unchanged; the similarity is integer arithmetic on ``canon.match_forms``' output.

The header states the definition in full.  It is the project's own: written after what RDKit's
``MurckoScaffold.GetScaffoldForMol`` is understood to do (rings, the linkers between them, and the atoms double-bonded to either)
and NOT RDKit's bit for bit -- RDKit is not available where this was built, so nothing here was compared with it.  A scaffold is
a labelled graph, not a canonical SMILES after sanitisation: two Kekule drawings of one scaffold are two scaffolds.  No SSSR is
computed and no ring is enumerated: ring sizes are per ring BOND (the smallest cycle through it), ``n_rings`` is the cyclomatic
number.  How far ``scaffold_similarity`` sits from the reference's ``ScafMetric`` on a trained model's samples has not been
measured.  GPU only, no CPU fallback."""
from __future__ import annotations

import math

import torch

from . import _lib
from ._packed import PackedRecord
from ._packed import check_key_bits as _check_key_bits
from .canon import CanonicalSet, _scope_code, canonical_forms, match_forms
from .decode import MoleculeBatch, decode_molecule_graphs, device_batch
from .descriptors import DescriptorTables, MoleculeDescriptors
from .descriptors import _launch as _describe
from .validity import MoleculeValidity, ValenceTables
from .validity import _launch as _check

__all__ = ["MoleculeScaffolds", "murcko_scaffolds", "scaffold_store", "ScaffoldStock", "scaffold_similarity", "counts",
           "MOL_FIELDS", "HIST_BINS", "MAX_RING", "NO_SYSTEM", "ROLES"]

MOL_FIELDS = ("status", "n_heavy", "n_scaffold_atoms", "n_scaffold_bonds", "n_exo", "n_linker_atoms", "n_ring_atoms", "n_ring_bonds",
              "n_rings", "n_ring_systems", "largest_system_atoms", "min_ring", "max_ring")      # the named columns of `mol`
_MOL_COLUMNS = 16                # DG_SCAF_MOL_FIELDS: the named columns, then zeros
HIST_BINS = ("3", "4", "5", "6", "7", "8", "9-12", "13+")      # the columns of `ring_hist`
MAX_RING, NO_SYSTEM = 255, 255   # DG_SCAF_MAX_RING, DG_SCAF_NO_SYSTEM
ROLES = ("none", "side", "exo", "linker", "ring")      # the values of `atom_role`


class MoleculeScaffolds(PackedRecord):
    """The scaffolds of one batch: typed views of one packed byte buffer, and the derived batch.

    ====================  ===============  ===========================================================================
    ``mol``               [B,16] int32     one row per molecule; its columns are the attributes below, then three zeros
    ``status``            [B] int32        the validity status; every other column is 0 unless it is 0
    ``n_heavy``           [B] int32        atoms of the scope
    ``n_scaffold_atoms``, ``n_scaffold_bonds`` [B] int32   atoms and bonds of the scaffold
    ``n_exo``, ``n_linker_atoms``, ``n_ring_atoms`` [B] int32   atoms double-bonded to the core from outside; core atoms
                                           without a ring bond; atoms with a ring bond
    ``n_ring_bonds``, ``n_rings`` [B] int32   bonds that are no bridge; ring bonds - ring atoms + ring systems
    ``n_ring_systems``, ``largest_system_atoms`` [B] int32   connected components of the ring bonds; atoms of the largest
    ``min_ring``, ``max_ring`` [B] int32   smallest and largest ring size of a ring bond; 0 without a ring
    ``ring_hist``         [B,8] int32      ring bonds by ring size: 3, 4, 5, 6, 7, 8, 9-12, 13 and more (``HIST_BINS``)
    ``atom_role``         [B,N] uint8      0 outside the scope, 1 side chain, 2 exo, 3 linker, 4 ring atom (``ROLES``)
    ``atom_system``       [B,N] uint8      smallest atom index of the atom's ring system; 255 where there is none
    ``bond_ring_size``    [B,cap] uint8    per row of the bond list the size of the smallest ring through a ring bond
                                           (at most 255), 0 for any other row; entries past ``min(n_bonds, cap)`` are
                                           unwritten memory
    ``batch``             MoleculeBatch    the scaffolds as a decoded batch of the same B, N and cap (no ``valence2``):
                                           scaffold atoms keep label and position, every other position is an isolated pad
    ====================  ===============  ===========================================================================

    ``cpu()`` moves the record with one device->host copy per buffer: its own and the derived batch's."""

    def __init__(self, buffer, B, N, cap, batch=None):
        self.B, self.N, self.cap = B, N, cap
        super().__init__(buffer, B, N, cap)
        self.batch = batch

    @staticmethod
    def _fields(B, N, cap):
        return (("mol", 4, (B, _MOL_COLUMNS)), ("ring_hist", 4, (B, len(HIST_BINS))), ("atom_role", 1, (B, N)),
                ("atom_system", 1, (B, N)), ("bond_ring_size", 1, (B, cap)))

    @staticmethod
    def empty(B, N, cap, device):
        """A device record and its derived batch over uninitialised buffers (``murcko_scaffolds(..., out=)`` fills them)."""
        rec = MoleculeScaffolds._empty(device, B, N, cap)
        rec.batch = MoleculeBatch.empty(B, N, cap, False, device)
        return rec

    def __len__(self):
        return self.B

    def cpu(self):
        if self.is_host:
            return self
        host = super().cpu()
        host.batch = None if self.batch is None else self.batch.cpu()
        return host


for _k, _name in enumerate(MOL_FIELDS):
    setattr(MoleculeScaffolds, _name, property(lambda self, _k=_k: self.mol[:, _k]))


def _launch(batch, descriptors, tables, out, at=0, seen=0):
    """``dg_mol_scaffold`` of ``batch`` into the rows ``at ..`` of ``out`` and of ``out.batch``, its keys and classes read from
    the rows ``seen ..`` of ``descriptors``."""
    if batch.B == 0:
        return
    cap, to = batch.cap, out.batch
    _lib.launch("dg_mol_scaffold", batch.buffer,
                batch.atoms.data_ptr(), batch.bonds.data_ptr() if cap > 0 else None, batch.n_bonds.data_ptr(),
                descriptors.desc[seen:].data_ptr(), descriptors.atom_key[seen:].data_ptr(),
                descriptors.bond_class[seen:].data_ptr() if cap > 0 else None, tables.bonds.data_ptr(), tables.n_bond_labels,
                batch.B, batch.N, cap, out.mol[at:].data_ptr(), out.ring_hist[at:].data_ptr(), out.atom_role[at:].data_ptr(),
                out.atom_system[at:].data_ptr(), out.bond_ring_size[at:].data_ptr() if cap > 0 else None,
                to.atoms[at:].data_ptr(), to.bonds[at:].data_ptr() if cap > 0 else None, to.n_bonds[at:].data_ptr(),
                to.component[at:].data_ptr(), to.n_components[at:].data_ptr(), to.largest[at:].data_ptr(),
                to.largest_size[at:].data_ptr())


def _check_tables(tables, who, dev):
    if not isinstance(tables, DescriptorTables):
        raise TypeError(f"{who} takes DescriptorTables (DescriptorTables.from_decoders): its bond table is read")
    if tables.device != dev:
        raise ValueError(f"the tables live on {tables.device}, the molecules on {dev}")


def _is_out(out, B, N, cap, dev):
    to = getattr(out, "batch", None)
    return (isinstance(out, MoleculeScaffolds) and not out.is_host and (out.B, out.N, out.cap) == (B, N, cap)
            and out.buffer.device == dev and isinstance(to, MoleculeBatch) and not to.is_host
            and (to.B, to.N, to.cap) == (B, N, cap) and to.valence2 is None and to.buffer.device == dev)


def murcko_scaffolds(batch, descriptors, tables, out=None):
    """``MoleculeScaffolds`` of a device ``MoleculeBatch``, on its device and the current stream.

    ``descriptors``: the ``MoleculeDescriptors`` that ``describe_molecules`` made of THIS batch (its status, ``atom_key`` and
    ``bond_class`` are read on the device, and they carry the scope; another batch's record gives numbers without a meaning).
    ``tables``: the ``DescriptorTables`` in use; only its bond table is read.  ``out``: a ``MoleculeScaffolds.empty(B, N, cap,
    device)`` to write into.  One launch; every element but the rows past the bond counts is written by every call, nothing is
    allocated with ``out=`` and nothing synchronises: capturable."""
    device_batch(batch, "murcko_scaffolds", "scaffolds")
    dev = batch.buffer.device
    _check_tables(tables, "murcko_scaffolds", dev)
    B, N, cap = batch.B, batch.N, batch.cap
    if (not isinstance(descriptors, MoleculeDescriptors) or descriptors.is_host or (descriptors.B, descriptors.N, descriptors.cap) != (B, N, cap)
            or descriptors.buffer.device != dev):
        raise ValueError("descriptors= must be the device MoleculeDescriptors of this batch (descriptors.describe_molecules)")
    if out is None:
        out = MoleculeScaffolds.empty(B, N, cap, dev)
    elif not _is_out(out, B, N, cap, dev):
        raise ValueError("out= must be a device MoleculeScaffolds of this batch's B, N and bond_cap (MoleculeScaffolds.empty)")
    _launch(batch, descriptors, tables, out)
    return out


def scaffold_store(store, valence_tables, descriptor_tables, chunk=1024, scope="largest", bond_cap=None):
    """``(MoleculeValidity, MoleculeDescriptors, MoleculeScaffolds)`` of every molecule of a ``resident.ResidentMolecules`` store,
    ``chunk`` molecules at a time by the route of ``substructure.match_store``: ``store.batch`` -> ``decode_molecule_graphs`` ->
    ``dg_mol_validity`` -> ``dg_mol_descriptors`` -> ``dg_mol_scaffold``, each written at the row offsets of one record.  Nothing
    but the unwritten rows past a molecule's bond counts depends on ``chunk``."""
    code = _scope_code(scope)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    if not isinstance(valence_tables, ValenceTables):
        raise TypeError("scaffold_store takes ValenceTables and DescriptorTables (their from_decoders)")
    _check_tables(descriptor_tables, "scaffold_store", store.device)
    if valence_tables.device != descriptor_tables.device:
        raise ValueError(f"the ValenceTables live on {valence_tables.device}, the molecules on {descriptor_tables.device}")
    n, N = len(store), store.vertexes
    cap = N * (N - 1) // 2 if bond_cap is None else int(bond_cap)
    checked = MoleculeValidity.empty(n, N, cap, store.device)
    described = MoleculeDescriptors.empty(n, N, cap, store.device)
    out = MoleculeScaffolds.empty(n, N, cap, store.device)
    for at in range(0, n, chunk):
        index = torch.arange(at, min(n, at + chunk), device=store.device)
        _, a, x = store.batch(index)
        if store.atom_dim != store.m_dim:
            x = x[..., :store.atom_dim].contiguous()
        batch = decode_molecule_graphs(x, a, bond_cap=cap)
        _check(batch, valence_tables, code, checked, at)
        _describe(batch, checked, descriptor_tables, code, described, at, at)
        _launch(batch, described, descriptor_tables, out, at, at)
    return checked, described, out


def _device_scaffolds(scaffolds, who):
    if not isinstance(scaffolds, MoleculeScaffolds):
        raise TypeError(f"{who} takes MoleculeScaffolds (murcko_scaffolds / scaffold_store)")
    if scaffolds.is_host or not isinstance(scaffolds.batch, MoleculeBatch) or scaffolds.batch.is_host:
        raise RuntimeError("druggen_amd.scaffolds runs on the GPU (no CPU fallback): pass the device MoleculeScaffolds")


def _min_rings(min_rings):
    if not isinstance(min_rings, int) or isinstance(min_rings, bool) or min_rings < 0:
        raise ValueError(f"min_rings must be an integer >= 0, got {min_rings!r}")
    return min_rings


def _kept_counts(scaffolds, min_rings, key_bits):
    """Forms of the scaffolds, the mask of the molecules that count (status 0, ``n_rings >= min_rings``, a scaffold that is not empty, a form) and, at the first
    molecule of every distinct kept form, how many kept molecules share it (0 everywhere else); all on the device.  Equal forms
    are equal labelled graphs, so a form is shared by kept molecules only or by none."""
    forms = canonical_forms(scaffolds.batch, "whole")
    first = match_forms(forms, None, key_bits).duplicate_of.to(torch.int64)
    kept = (scaffolds.status == 0) & (scaffolds.n_rings >= min_rings) & (forms.n_splits >= 0) & (scaffolds.n_scaffold_atoms > 0)
    here = torch.arange(scaffolds.B, device=first.device)
    count = torch.zeros(scaffolds.B, dtype=torch.int64, device=first.device)
    count.index_add_(0, torch.where(first >= 0, first, here), kept.to(torch.int64))
    return forms, kept, count


class ScaffoldStock:
    """A reference set of scaffolds to compare generated ones with: ``set`` -- the ``canon.CanonicalSet`` of the scaffolds'
    forms (scope ``"whole"`` of the derived batch); ``count`` int64 [n] -- at the smallest index of every distinct form of a
    molecule that counts (status 0, ``n_rings >= min_rings``, a form) the number of such molecules with that form, 0 at every
    other index, so a molecule that does not count contributes nothing wherever it is hit; ``sum_squares`` -- ``sum(count^2)``
    as a 0-d int64 device tensor; ``min_rings``, ``key_bits``."""

    def __init__(self, canonical_set, count, sum_squares, min_rings, key_bits):
        self.set, self.count, self.sum_squares, self.min_rings, self.key_bits = canonical_set, count, sum_squares, min_rings, key_bits

    def __len__(self):
        return len(self.set)

    @classmethod
    def from_scaffolds(cls, scaffolds, min_rings=2, key_bits=64):
        """The stock of device ``MoleculeScaffolds`` (``scaffold_store`` of a training or drug store).  ``min_rings``: the
        reference's ``compute_scaffold(min_rings=2)`` -- scaffolds with fewer rings do not count."""
        _device_scaffolds(scaffolds, "ScaffoldStock.from_scaffolds")
        _min_rings(min_rings)
        _check_key_bits(key_bits)
        forms, _, count = _kept_counts(scaffolds, min_rings, key_bits)
        return cls(CanonicalSet.from_forms(forms, key_bits), count, (count * count).sum(), min_rings, key_bits)


def _sums(scaffolds, stock):
    _device_scaffolds(scaffolds, "scaffold_similarity")
    if not isinstance(stock, ScaffoldStock):
        raise TypeError("stock must be a ScaffoldStock (ScaffoldStock.from_scaffolds)")
    forms, kept, count = _kept_counts(scaffolds, stock.min_rings, stock.key_bits)
    hit = match_forms(forms, stock.set, stock.key_bits).stock_hit.to(torch.int64)
    found = kept & (hit >= 0)
    shared = torch.where(found, stock.count[hit.clamp(min=0)], torch.zeros_like(count)) if len(stock) else torch.zeros_like(count)
    return torch.stack([shared.sum(), (count * count).sum(), stock.sum_squares]).cpu().tolist()      # the one transfer


def counts(scaffolds, stock):
    """``(dot, g2, r2)`` as Python ints: the sum over the generated molecules that count of the stock's count of their form;
    the sum of squares of the generated counts per distinct form; the stock's.  One device->host transfer."""
    return tuple(int(v) for v in _sums(scaffolds, stock))


def scaffold_similarity(scaffolds, stock):
    """The reference's ``ScafMetric`` value of generated ``scaffolds`` against a ``ScaffoldStock``: the cosine of the two count
    vectors over distinct scaffolds, ``dot / sqrt(g2 * r2)`` in float64 (``counts``); ``nan`` when either side keeps no
    scaffold, as ``cos_similarity`` returns it.  Molecules count under the stock's ``min_rings``.  Everything before the three
    int64 sums stays on the device, and they cross in one transfer.  Scaffolds are compared as labelled graphs (see the module's
    text for what that is not)."""
    dot, g2, r2 = counts(scaffolds, stock)
    if g2 == 0 or r2 == 0:
        return float("nan")
    return dot / math.sqrt(float(g2) * float(r2))
