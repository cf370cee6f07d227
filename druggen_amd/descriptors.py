"""Drug-likeness descriptors of decoded molecules, made on the GPU (``dg_mol_descriptors``, ``include/druggen_hip_desc.h``,
DESIGN 3.30): rotatable bonds, a topological polar surface area summed from a table of atom environments, ring, aromatic-atom
and carbon counts, and the environment key of every atom -- for the molecules that ``validity.check_molecules`` found valid,
without a device->host copy of the molecules and RDKit.  From these and the validity record's mass and N / O counts come the
rule counts the reference reports per generated molecule (``obey_lipinski``, ``obey_veber``): ``lipinski_rules`` and
``veber_rules`` below.

The header states the definition in full.  It is the project's own and NOT RDKit's: ``n_rot`` is the SIMPLE rotatable-bond
pattern (a single bond outside every ring between two atoms that each have another neighbour, no triple bond at either end),
not ``CalcNumRotatableBonds``' strict one, which also drops amides, esters and the like; ``tpsa`` is the sum of the built-in
table ``TPSA`` -- the N and O rows of Ertl, Rohde and Selzer (2000) that a neutral graph with implicit hydrogens can reach,
written down from memory, no S or P contributions -- not ``CalcTPSA``; donors and acceptors are the validity record's N / O
counts, not ``NumHDonors`` / ``NumHAcceptors``; and there is no logP, so Lipinski's fourth rule is missing.  How far the rule
counts sit from the reference's on a trained model's samples has not been measured.  GPU only, no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._packed import PackedRecord
from .canon import SCOPES, _scope_code
from .decode import decode_molecule_graphs, device_batch
from .smiles_out import table_rows as _symbol_rows
from .validity import _ORDER, _POLAR, VALID, MoleculeValidity, ValenceTables
from .validity import _launch as _check

__all__ = ["DescriptorTables", "MoleculeDescriptors", "describe_molecules", "descriptor_store", "lipinski_rules", "veber_rules",
           "env_key", "env_rows", "TPSA", "DESC_FIELDS", "NO_KEY", "MAX_ENV", "BOND", "RING_BOND", "ROTATABLE"]

DESC_FIELDS = ("status", "n_heavy", "n_rot", "tpsa", "n_untyped", "n_rings", "n_ring_atoms", "n_aromatic_atoms", "n_carbon",
               "n_sp3_carbon", "reserved0", "reserved1")      # the row of `desc`
NO_KEY = 0xFFFFFFFF      # DG_DESC_NO_KEY
MAX_ENV = 4096           # DG_DESC_MAX_ENV
BOND, RING_BOND, ROTATABLE = 1, 2, 4      # the bits of `bond_class`
_CARBON = 6
_MAX_VALUE = (1 << 23) - 1      # 256 atoms of it stay below 2^31

# (atomic number, h, n1, n2, n3, na, r3, 1e-2 A^2): implicit hydrogens, bonds of order 1 (not aromatic) / 2 / 3, aromatic bonds,
# and the three-ring variant -- 0: outside a triangle only, 1: in one only, None: either
TPSA = (
    (7, 0, 3, 0, 0, 0, 0, 324),         # N(-)(-)-
    (7, 0, 3, 0, 0, 0, 1, 301),         # ... in a three-ring
    (7, 0, 1, 1, 0, 0, None, 1236),     # N(-)=
    (7, 0, 0, 0, 1, 0, None, 2379),     # N#
    (7, 1, 2, 0, 0, 0, 0, 1203),        # [NH](-)-
    (7, 1, 2, 0, 0, 0, 1, 2194),        # ... in a three-ring
    (7, 1, 0, 1, 0, 0, None, 2385),     # [NH]=
    (7, 2, 1, 0, 0, 0, None, 2602),     # [NH2]-
    (7, 0, 0, 0, 0, 2, None, 1289),     # n(:):
    (7, 0, 0, 0, 0, 3, None, 441),      # n(:)(:):
    (7, 0, 1, 0, 0, 2, None, 493),      # n(-)(:):
    (8, 0, 2, 0, 0, 0, 0, 923),         # O(-)-
    (8, 0, 2, 0, 0, 0, 1, 1253),        # ... in a three-ring
    (8, 0, 0, 1, 0, 0, None, 1707),     # O=
    (8, 1, 1, 0, 0, 0, None, 2023),     # [OH]-
    (8, 0, 0, 0, 0, 2, None, 1314),     # o(:):
)


def env_key(label, h, n1, n2, n3, na, r3):
    """The environment key of the header: ``label | h << 8 | n1 << 12 | n2 << 16 | n3 << 19 | na << 21 | r3 << 24``."""
    return label | h << 8 | n1 << 12 | n2 << 16 | n3 << 19 | na << 21 | r3 << 24


def env_rows(atom_decoder, tpsa=None):
    """``tpsa`` (rows like ``TPSA``, the default) expanded over the atom labels of ``atom_decoder`` and over ``r3`` -- a pattern
    whose ``r3`` is None gives both keys the same value -- as a ``[n_env, 2]`` uint32 array of ``(key, value)`` with the keys
    strictly ascending.  A pattern of an element no label decodes to gives no row.  ``ValueError`` on a field out of its range
    (h, n1 0..8, n2 0..4, n3 0..2, na 0..7, r3 0 / 1 / None, value 0..2^23 - 1), on two patterns that reach the same key, and
    on more than 4096 rows."""
    rows = {}
    for row in (TPSA if tpsa is None else tpsa):
        try:
            z, h, n1, n2, n3, na, r3, value = row
        except (TypeError, ValueError):
            raise ValueError(f"a tpsa= row is (atomic number, h, n1, n2, n3, na, r3, value), got {row!r}") from None
        if (not 0 <= h <= 8 or not 0 <= n1 <= 8 or not 0 <= n2 <= 4 or not 0 <= n3 <= 2 or not 0 <= na <= 7
                or r3 not in (0, 1, None) or not 0 <= value <= _MAX_VALUE):
            raise ValueError(f"tpsa= row {row!r}: h, n1 in 0..8, n2 in 0..4, n3 in 0..2, na in 0..7, r3 0, 1 or None, "
                             f"value in 0..{_MAX_VALUE}")
        for label in sorted(atom_decoder):
            if int(atom_decoder[label]) != z or z == 0:
                continue
            for r in ((0, 1) if r3 is None else (r3,)):
                key = env_key(int(label), h, n1, n2, n3, na, r)
                if key in rows:
                    raise ValueError(f"tpsa= row {row!r}: the key of (label {label}, r3 {r}) is reached twice")
                rows[key] = value
    if len(rows) > MAX_ENV:
        raise ValueError(f"tpsa= expands to {len(rows)} rows over the atom labels, at most {MAX_ENV} fit")
    return np.array(sorted(rows.items()), dtype=np.uint32).reshape(-1, 2)


class DescriptorTables:
    """The tables of ``dg_mol_descriptors`` on a device; the kernel itself knows no chemistry.  ``atom_class``
    ``[n_atom_labels]`` (bit 0: a carbon), ``atom_flags`` ``[n_atom_labels]`` (the flags column of the validity check's atom
    table; bit 0: polar, N and O), ``bond_rows`` ``[n_bond_labels]`` (``order | aromatic << 8``, the validity check's) and
    ``env`` ``[n_env, 2]`` ``(key, tpsa in 1e-2 A^2)``.  ``ValueError`` unless the keys are strictly ascending -- the kernel
    searches them and does not check -- and ``n_env <= 4096``."""

    def __init__(self, atom_class, atom_flags, bond_rows, env, device):
        atom_class, atom_flags, bond_rows = (np.ascontiguousarray(t, dtype=np.uint32) for t in (atom_class, atom_flags, bond_rows))
        env = np.ascontiguousarray(env, dtype=np.uint32).reshape(-1, 2)
        if atom_class.ndim != 1 or atom_class.shape != atom_flags.shape or not 1 <= len(atom_class) <= 255:
            raise ValueError("atom_class and atom_flags are one word per atom label, 1..255 labels")
        if bond_rows.ndim != 1 or not 1 <= len(bond_rows) <= 256:
            raise ValueError("bond_rows is one word per bond label, 1..256 labels")
        if len(env) > MAX_ENV:
            raise ValueError(f"the environment table has {len(env)} rows, at most {MAX_ENV} fit")
        if len(env) > 1 and not (env[1:, 0] > env[:-1, 0]).all():
            raise ValueError("the keys of the environment table must be strictly ascending (sorted, no key twice)")
        self.atom_class_rows, self.atom_flag_rows, self.bond_rows, self.env_rows = atom_class, atom_flags, bond_rows, env
        self.n_atom_labels, self.n_bond_labels, self.n_env = len(atom_class), len(bond_rows), len(env)
        wide = np.zeros((len(env), 4), dtype=np.uint32)
        wide[:, :2] = env

        def up(a):
            return torch.from_numpy(a.view(np.int32)).to(device).contiguous()      # (the bit patterns)
        self.atom_class, self.atom_flags, self.bonds, self.env = up(atom_class), up(atom_flags), up(bond_rows), up(wide)
        self.device = self.atom_class.device      # with its index, as a batch's buffer reports it

    @classmethod
    def from_decoders(cls, atom_decoder, bond_decoder, device, tpsa=None):
        """Build and upload the tables.  ``tpsa``: None for the built-in ``TPSA``; rows like it, expanded by ``env_rows`` over
        the atom labels and ``r3`` (``ValueError`` on a key reached twice); or a ready ``[n, 2]`` numpy array of ``(key,
        value)`` taken as it is (``ValueError`` unless its keys are strictly ascending).  The decoders are those of
        ``SmilesTables.from_decoders``, checked like them."""
        _symbol_rows(atom_decoder, bond_decoder)
        n = len(atom_decoder)
        z = [int(atom_decoder[l]) for l in range(n)]
        env = tpsa if isinstance(tpsa, np.ndarray) else env_rows(atom_decoder, tpsa)
        return cls([int(a == _CARBON) for a in z], [int(a in _POLAR) for a in z],
                   [_ORDER.get(int(bond_decoder[l]), 0) for l in range(len(bond_decoder))], env, device)


class MoleculeDescriptors(PackedRecord):
    """The descriptors of one batch: typed views of one packed byte buffer.

    ====================  ===============  ===========================================================================
    ``desc``              [B,12] int32     one row per molecule; its columns are the attributes below, then two zeros
    ``status``            [B] int32        the validity status (``validity.STATUS``); every other column is 0 unless it is 0
    ``n_heavy``           [B] int32        atoms of the scope
    ``n_rot``             [B] int32        rotatable bonds (the simple pattern, see the module's text)
    ``tpsa``              [B] int32        polar surface area in 1e-2 A^2: the table values of the atoms' keys, summed
    ``n_untyped``         [B] int32        polar atoms (N, O) whose key has no table row: they contribute 0 to ``tpsa``
    ``n_rings``           [B] int32        bonds - atoms + connected components
    ``n_ring_atoms``, ``n_aromatic_atoms``, ``n_carbon``, ``n_sp3_carbon`` [B] int32   atoms with a ring bond, with an
                                           aromatic bond, carbons, carbons with single bonds only
    ``atom_key``          [B,N] int32      the bit pattern of the environment key (``env_key``); -1 (0xFFFFFFFF) outside
                                           the scope and unless status is 0
    ``bond_class``        [B,cap] uint8    per row of the bond list ``BOND | RING_BOND | ROTATABLE``; 0: no bond of the scope,
                                           or status != 0; entries past ``min(n_bonds, cap)`` are unwritten memory
    ====================  ===============  ===========================================================================

    ``cpu()`` moves the packed buffer with ONE device->host copy."""

    def __init__(self, buffer, B, N, cap):
        self.B, self.N, self.cap = B, N, cap
        super().__init__(buffer, B, N, cap)

    @staticmethod
    def _fields(B, N, cap):
        return ("desc", 4, (B, len(DESC_FIELDS))), ("atom_key", 4, (B, N)), ("bond_class", 1, (B, cap))

    @staticmethod
    def empty(B, N, cap, device):
        """A device record over an uninitialised buffer (``describe_molecules(..., out=)`` fills it)."""
        return MoleculeDescriptors._empty(device, B, N, cap)

    def __len__(self):
        return self.B

    @property
    def tpsa_A2(self):
        """``tpsa`` in A^2, float64 [B]."""
        return self.tpsa.astype(np.float64) / 100.0 if self.is_host else self.tpsa.to(torch.float64) / 100.0

    @property
    def veber_rules(self):
        """``veber_rules(self)``."""
        return veber_rules(self)

    def lipinski_rules(self, validity):
        """``lipinski_rules(validity, self)``."""
        return lipinski_rules(validity, self)


for _k, _name in enumerate(DESC_FIELDS[:10]):
    setattr(MoleculeDescriptors, _name, property(lambda self, _k=_k: self.desc[:, _k]))


def _count(rules, valid, host):
    if host:
        return np.where(valid, sum(r.astype(np.int32) for r in rules), 0).astype(np.int32)
    total = sum(r.to(torch.int32) for r in rules)
    return torch.where(valid, total, torch.zeros_like(total))


def veber_rules(descriptors):
    """How many of Veber's two rules each molecule obeys, int32 [B] in 0..2: ``n_rot <= 10`` and ``tpsa <= 140 A^2``.  0 for a
    molecule whose status is not 0.  ``n_rot`` and ``tpsa`` are this module's, not RDKit's (see the module's text)."""
    d = descriptors
    return _count((d.n_rot <= 10, d.tpsa <= 14000), d.status == VALID, d.is_host)


def lipinski_rules(validity, descriptors):
    """How many of four rules each molecule obeys, int32 [B] in 0..4: mass < 500 Da, donors <= 5, acceptors <= 10, ``n_rot <=
    10`` -- the reference's ``obey_lipinski`` rules 1, 2, 3 and 5.  Its rule 4, the logP range, is MISSING: no logP is computed
    here.  The donor and acceptor counts are the validity record's N / O counts (N or O atoms with a hydrogen; N or O atoms),
    Lipinski's original ones, not RDKit's ``NumHDonors`` / ``NumHAcceptors``; the mass is the monoisotopic one of
    ``validity.VALENCES``.  0 for a molecule whose status is not 0.  ``validity``: the ``MoleculeValidity`` the descriptors
    were made from, on the same side (device or host)."""
    v, d = validity, descriptors
    if not isinstance(v, MoleculeValidity) or not isinstance(d, MoleculeDescriptors) or v.is_host != d.is_host or v.B != d.B:
        raise ValueError("lipinski_rules takes a MoleculeValidity and the MoleculeDescriptors made from it, both on the device or "
                         "both on the host")
    return _count((v.mass < 5000000, v.n_donors <= 5, v.n_acceptors <= 10, d.n_rot <= 10), d.status == VALID, d.is_host)


def _launch(batch, validity, tables, code, out, at=0, seen=0):
    """``dg_mol_descriptors`` of ``batch`` into the rows ``at ..`` of ``out`` (same N and cap), its verdicts read from the rows
    ``seen ..`` of ``validity``."""
    if batch.B == 0:
        return
    cap = batch.cap
    largest = code == SCOPES["largest"]
    _lib.launch("dg_mol_descriptors", batch.buffer,
                batch.atoms.data_ptr(), batch.bonds.data_ptr() if cap > 0 else None, batch.n_bonds.data_ptr(),
                batch.component.data_ptr() if largest else None, batch.largest.data_ptr() if largest else None, None,
                validity.mol[seen:].data_ptr(), validity.hcount[seen:].data_ptr(), tables.bonds.data_ptr(), tables.n_bond_labels,
                tables.atom_flags.data_ptr(), tables.atom_class.data_ptr(), tables.n_atom_labels,
                tables.env.data_ptr() if tables.n_env else None, tables.n_env, batch.B, batch.N, cap, code,
                out.desc[at:].data_ptr(), out.atom_key[at:].data_ptr(), out.bond_class[at:].data_ptr() if cap > 0 else None)


def _check_tables(tables, who, dev):
    if not isinstance(tables, DescriptorTables):
        raise TypeError(f"{who} takes DescriptorTables (DescriptorTables.from_decoders)")
    if tables.device != dev:
        raise ValueError(f"the tables live on {tables.device}, the molecules on {dev}")


def describe_molecules(batch, validity, tables, scope="largest", out=None):
    """``MoleculeDescriptors`` of a device ``MoleculeBatch``, on its device and the current stream.

    ``validity``: the ``MoleculeValidity`` that ``check_molecules`` made of THIS batch under THIS scope (its status and
    ``hcount`` are read on the device; another batch's or scope's record gives numbers without a meaning).  ``scope``:
    ``"largest"`` or ``"whole"``, as there.  ``out``: a ``MoleculeDescriptors.empty(B, N, cap, device)`` to write into.  One
    launch; every element but the bond classes past a molecule's bond count is written by every call, nothing is allocated
    with ``out=`` and nothing synchronises: capturable."""
    device_batch(batch, "describe_molecules", "descriptors")
    code = _scope_code(scope)
    dev = batch.buffer.device
    _check_tables(tables, "describe_molecules", dev)
    B, N, cap = batch.B, batch.N, batch.cap
    if (not isinstance(validity, MoleculeValidity) or validity.is_host or (validity.B, validity.N, validity.cap) != (B, N, cap)
            or validity.buffer.device != dev):
        raise ValueError("validity= must be the device MoleculeValidity of this batch (validity.check_molecules)")
    if out is None:
        out = MoleculeDescriptors.empty(B, N, cap, dev)
    elif (not isinstance(out, MoleculeDescriptors) or out.is_host or (out.B, out.N, out.cap) != (B, N, cap)
            or out.buffer.device != dev):
        raise ValueError("out= must be a device MoleculeDescriptors of this batch's B, N and bond_cap (MoleculeDescriptors.empty)")
    _launch(batch, validity, tables, code, out)
    return out


def descriptor_store(store, valence_tables, tables, chunk=1024, scope="largest", bond_cap=None):
    """``(MoleculeValidity, MoleculeDescriptors)`` of every molecule of a ``resident.ResidentMolecules`` store, ``chunk``
    molecules at a time by the route of ``validity.validity_store``: ``store.batch`` -> ``decode_molecule_graphs`` (the one-hots
    serve as logits) -> ``dg_mol_validity`` -> ``dg_mol_descriptors``, both written at the row offsets of one record each.
    Nothing but the unwritten rows past a molecule's bond count depends on ``chunk``."""
    code = _scope_code(scope)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    if not isinstance(valence_tables, ValenceTables):
        raise TypeError("descriptor_store takes ValenceTables (ValenceTables.from_decoders) and DescriptorTables")
    _check_tables(tables, "descriptor_store", store.device)
    if valence_tables.device != tables.device:
        raise ValueError(f"the valence tables live on {valence_tables.device}, the molecules on {tables.device}")
    n, N = len(store), store.vertexes
    cap = N * (N - 1) // 2 if bond_cap is None else int(bond_cap)
    checked = MoleculeValidity.empty(n, N, cap, store.device)
    out = MoleculeDescriptors.empty(n, N, cap, store.device)
    for at in range(0, n, chunk):
        index = torch.arange(at, min(n, at + chunk), device=store.device)
        _, a, x = store.batch(index)
        if store.atom_dim != store.m_dim:
            x = x[..., :store.atom_dim].contiguous()
        batch = decode_molecule_graphs(x, a, bond_cap=cap)
        _check(batch, valence_tables, code, checked, at)
        _launch(batch, checked, tables, code, out, at, at)
    return checked, out
