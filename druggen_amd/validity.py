"""Validity of decoded molecules, checked on the GPU (``dg_mol_validity``, ``include/druggen_hip_valid.h``): is a
decoded graph a molecule at all -- an allowed valence at every atom, aromatic bonds in rings only, a Kekule structure for them
-- and, for those that are, implicit hydrogens per atom, the molecular mass and the N / O counts, without a device->host copy
of the molecules and RDKit.

The reference's first evaluation number is ``fraction_valid``: what survives ``Chem.SanitizeMol``.  This check is the project's
own, exactly specified one -- the header states it in full -- and NOT ``SanitizeMol``: the decoded graph carries no charges,
radicals or explicit hydrogens, so an aromatic ``[nH]`` drawn with aromatic bonds, a nitro group ``N(=O)=O`` and ``[N+]`` are
invalid here; aromaticity is taken from the bond labels as they are (no perception, no ring-size or Hueckel rule);
``n_donors`` / ``n_acceptors`` are N / O counts, not RDKit's SMARTS-based ``NumHDonors`` / ``NumHAcceptors``.  How far
``valid_fraction`` sits from RDKit's on a trained model's samples has not been measured.  GPU only, no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._packed import PackedRecord
from .canon import SCOPES, _scope_code
from .decode import decode_molecule_graphs, device_batch
from .smiles import AROMATIC, DOUBLE, SINGLE, TRIPLE
from .smiles_out import table_rows as _symbol_rows

__all__ = ["ValenceTables", "MoleculeValidity", "check_molecules", "validity_store", "table_rows", "STATUS", "VALENCES", "H_MASS",
           "VALID", "NO_GRAPH", "EMPTY", "UNKNOWN_LABEL", "OVER_VALENT", "AROMATIC_NOT_IN_RING", "NOT_KEKULISABLE"]

VALID, NO_GRAPH, EMPTY, UNKNOWN_LABEL, OVER_VALENT, AROMATIC_NOT_IN_RING, NOT_KEKULISABLE = 0, -2, 1, 2, 3, 4, 5      # DG_VALID_*
STATUS = {VALID: "valid", NO_GRAPH: "no graph (truncated bond list)", EMPTY: "no atom in the scope",
          UNKNOWN_LABEL: "an atom or bond label without a table row", OVER_VALENT: "an atom above its largest allowed valence",
          AROMATIC_NOT_IN_RING: "an aromatic bond outside every ring", NOT_KEKULISABLE: "the aromatic bonds have no Kekule structure"}
MOL_FIELDS = ("status", "n_atoms", "n_over", "deficiency", "n_h", "mass", "n_donors", "n_acceptors")      # the row of `mol`
H_MASS = 10078      # 1H, in 1e-4 Da
# atomic number -> (allowed valences ascending, monoisotopic mass in 1e-4 Da)
VALENCES = {5: ((3,), 110093), 6: ((4,), 120000), 7: ((3,), 140031), 8: ((2,), 159949), 9: ((1,), 189984), 14: ((4,), 279769),
            15: ((3, 5), 309738), 16: ((2, 4, 6), 319721), 17: ((1,), 349689), 33: ((3, 5), 749216), 34: ((2, 4, 6), 799165),
            35: ((1,), 789183), 53: ((1, 3, 5), 1269045)}
_POLAR = (7, 8)
_ORDER = {SINGLE: 1, DOUBLE: 2, TRIPLE: 3, AROMATIC: 1 | 1 << 8}      # order | aromatic << 8


def table_rows(atom_decoder, bond_decoder, valences=None):
    """The two tables as host arrays: ``[n_atom_labels, 4]`` uint32 -- the allowed valences as four bytes (ascending,
    zero-terminated), the mass in 1e-4 Da, a flag word (bit 0: polar, N and O), 0 -- and ``[n_bond_labels]`` uint32 -- ``order |
    aromatic << 8`` (0 for the no-bond label).  Atomic number 0 gives an empty row: an unknown label.  ``valences``:
    ``{atomic number: (valences, mass)}`` for elements beyond the built-in ``VALENCES``, or to replace one of them.  The
    decoders are those of ``smiles_out.table_rows``, checked by it: the same ``ValueError``s."""
    _symbol_rows(atom_decoder, bond_decoder)
    known = dict(VALENCES)
    for z, (vals, mass) in (valences or {}).items():
        vals = tuple(int(v) for v in vals)
        if not 1 <= len(vals) <= 4 or any(not 1 <= v <= 8 for v in vals) or list(vals) != sorted(set(vals)):
            raise ValueError(f"valences of atomic number {z}: one to four distinct values in 1..8, ascending, got {vals}")
        if not 0 <= int(mass) < 1 << 32:
            raise ValueError(f"mass of atomic number {z}: an unsigned 32-bit count of 1e-4 Da, got {mass}")
        known[int(z)] = (vals, int(mass))
    atom_rows = np.zeros((len(atom_decoder), 4), dtype=np.uint32)
    for l in range(len(atom_decoder)):
        z = int(atom_decoder[l])
        if z == 0:
            continue
        if z not in known:
            raise ValueError(f"atom label {l}: atomic number {z} has no valence row (built in: {sorted(VALENCES)}; pass valences=)")
        vals, mass = known[z]
        atom_rows[l] = sum(v << (8 * k) for k, v in enumerate(vals)), mass, z in _POLAR, 0
    bond_rows = np.array([_ORDER.get(int(bond_decoder[l]), 0) for l in range(len(bond_decoder))], dtype=np.uint32)
    return atom_rows, bond_rows


class ValenceTables:
    """The two tables of ``dg_mol_validity`` on a device (``table_rows``); the kernel itself knows no chemistry."""

    def __init__(self, atom_rows, bond_rows, device):
        self.atom_rows, self.bond_rows = atom_rows, bond_rows
        self.n_atom_labels, self.n_bond_labels = len(atom_rows), len(bond_rows)
        self.atoms = torch.from_numpy(atom_rows.view(np.int32)).to(device).contiguous()      # (the bit patterns)
        self.bonds = torch.from_numpy(bond_rows.view(np.int32)).to(device).contiguous()
        self.device = self.atoms.device      # with its index, as a batch's buffer reports it

    @classmethod
    def from_decoders(cls, atom_decoder, bond_decoder, device, valences=None):
        """Build and upload the tables; ``ValueError`` on an atomic number without a valence row, and
        ``SmilesTables.from_decoders``' errors."""
        return cls(*table_rows(atom_decoder, bond_decoder, valences), device)


class MoleculeValidity(PackedRecord):
    """The verdicts of one batch: typed views of one packed byte buffer.

    ===============  ===============  ================================================================================
    ``mol``          [B,8] int32      one row per molecule; its columns are the attributes below
    ``status``       [B] int32        0 valid, -2 no graph, 1 empty, 2 unknown label, 3 over-valent, 4 aromatic bond
                                      outside a ring, 5 not kekulisable (``STATUS``): the first that applies
    ``n_atoms``      [B] int32        atoms of the scope
    ``n_over``       [B] int32        over-valent atoms (0 for status -2, 1, 2)
    ``deficiency``   [B] int32        candidates a maximum matching leaves without a double bond; -1: not computed
    ``n_h``, ``mass``, ``n_donors``, ``n_acceptors`` [B] int32   status 0 only, else 0: implicit hydrogens, mass in 1e-4
                                      Da (hydrogens included), N / O atoms with a hydrogen, N / O atoms
    ``hcount``       [B,N] uint8      implicit hydrogens per atom; 0xFF outside the scope and unless status is 0
    ``kekule``       [B,cap,4] uint8  ``(hi, lo, label, order)`` per row of the bond list, order 1 / 2 / 3 with the
                                      aromatic bonds drawn single / double; 0: no bond of the scope, or status != 0; rows
                                      past ``min(n_bonds, cap)`` are unwritten memory.  A certificate, not a pinned value
    ===============  ===============  ================================================================================

    ``cpu()`` moves the packed buffer with ONE device->host copy."""

    def __init__(self, buffer, B, N, cap):
        self.B, self.N, self.cap = B, N, cap
        super().__init__(buffer, B, N, cap)

    @staticmethod
    def _fields(B, N, cap):
        return ("mol", 4, (B, len(MOL_FIELDS))), ("hcount", 1, (B, N)), ("kekule", 1, (B, cap, 4))

    @staticmethod
    def empty(B, N, cap, device):
        """A device record over an uninitialised buffer (``check_molecules(..., out=)`` fills it)."""
        return MoleculeValidity._empty(device, B, N, cap)

    def __len__(self):
        return self.B

    @property
    def valid(self):
        """Mask [B]: ``status == 0``."""
        return self.status == VALID

    def valid_fraction(self):
        """The share of valid molecules among all B (truncated ones count as invalid): a 0-d float64 device tensor on the
        device, a float on the host copy; nan for an empty batch."""
        if self.is_host:
            return float(self.valid.mean()) if self.B else float("nan")
        return self.valid.to(torch.float64).mean()


for _k, _name in enumerate(MOL_FIELDS):
    setattr(MoleculeValidity, _name, property(lambda self, _k=_k: self.mol[:, _k]))

_layout = MoleculeValidity.layout      # (B, N, cap) -> (name -> (byte offset, bytes, element bytes, shape), size)


def _launch(batch, tables, code, out, at=0):
    """``dg_mol_validity`` of ``batch`` into the rows ``at ..`` of ``out`` (same N and cap)."""
    if batch.B == 0:
        return
    cap = batch.cap
    largest = code == SCOPES["largest"]
    _lib.launch("dg_mol_validity", batch.buffer,
                batch.atoms.data_ptr(), batch.bonds.data_ptr() if cap > 0 else None, batch.n_bonds.data_ptr(),
                batch.component.data_ptr() if largest else None, batch.largest.data_ptr() if largest else None, None,
                tables.atoms.data_ptr(), tables.n_atom_labels, tables.bonds.data_ptr(), tables.n_bond_labels,
                batch.B, batch.N, cap, code, H_MASS,
                out.mol[at:].data_ptr(), out.hcount[at:].data_ptr(), out.kekule[at:].data_ptr() if cap > 0 else None)


def _check_tables(tables, who, dev):
    if not isinstance(tables, ValenceTables):
        raise TypeError(f"{who} takes ValenceTables (ValenceTables.from_decoders)")
    if tables.device != dev:
        raise ValueError(f"the tables live on {tables.device}, the molecules on {dev}")


def check_molecules(batch, tables, scope="largest", out=None):
    """``MoleculeValidity`` of a device ``MoleculeBatch``, on its device and the current stream.

    ``scope``: ``"largest"`` -- the largest fragment, what the reference evaluates -- or ``"whole"`` -- every atom except
    isolated pads; the membership rule of ``canon.canonical_forms``.  ``out``: a ``MoleculeValidity.empty(B, N, cap, device)``
    to write into.  One launch; every element but the Kekule rows past a molecule's bond count is written by every call,
    nothing is allocated with ``out=`` and nothing synchronises: capturable."""
    device_batch(batch, "check_molecules", "validity")
    code = _scope_code(scope)
    dev = batch.buffer.device
    _check_tables(tables, "check_molecules", dev)
    B, N, cap = batch.B, batch.N, batch.cap
    if out is None:
        out = MoleculeValidity.empty(B, N, cap, dev)
    elif (not isinstance(out, MoleculeValidity) or out.is_host or (out.B, out.N, out.cap) != (B, N, cap)
            or out.buffer.device != dev):
        raise ValueError("out= must be a device MoleculeValidity of this batch's B, N and bond_cap (MoleculeValidity.empty)")
    _launch(batch, tables, code, out)
    return out


def validity_store(store, tables, chunk=1024, scope="largest", bond_cap=None):
    """``MoleculeValidity`` of every molecule of a ``resident.ResidentMolecules`` store, ``chunk`` molecules at a time by the
    route of ``fingerprint_store``: ``store.batch`` -> ``decode_molecule_graphs`` (the one-hots serve as logits) ->
    ``dg_mol_validity``, written at the row offsets of one record.  ``mol`` and ``hcount`` do not depend on ``chunk``; the
    Kekule rows past a molecule's bond count are unwritten memory."""
    code = _scope_code(scope)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    _check_tables(tables, "validity_store", store.device)
    n, N = len(store), store.vertexes
    cap = N * (N - 1) // 2 if bond_cap is None else int(bond_cap)
    out = MoleculeValidity.empty(n, N, cap, store.device)
    for at in range(0, n, chunk):
        index = torch.arange(at, min(n, at + chunk), device=store.device)
        _, a, x = store.batch(index)
        if store.atom_dim != store.m_dim:
            x = x[..., :store.atom_dim].contiguous()
        _launch(decode_molecule_graphs(x, a, bond_cap=cap), tables, code, out, at)
    return out
