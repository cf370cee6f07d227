"""Circular fingerprints of decoded molecules, made on the GPU (``dg_mol_fingerprint``, ``include/druggen_hip_fp.h``,
DESIGN 3.27): the hop from a device ``decode.MoleculeBatch`` to the ``metrics.PackedFingerprints`` that SNN and internal
diversity start from, without a device->host copy of the molecules, RDKit and an upload.

The fingerprint is an ECFP-style circular fingerprint (Rogers & Hahn 2010, the algorithm Morgan fingerprints implement) in the
project's own, exactly specified sense -- the header states it down to the last bit.  It is NOT RDKit's bit vector: the hash
is the project's ``mix64``, and the atom invariant is (atomic number, degree, twice the valence, in-ring) where Morgan has
(atomic number, degree, total hydrogens, charge, isotope, in-ring).  Stock and generated molecules pass through the same
function, so Tanimoto similarities, SNN and IntDiv computed from these fingerprints are self-consistent; how far they move
against an RDKit run has not been measured.  GPU only, no CPU fallback."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .canon import SCOPES, _scope_code
from .decode import decode_molecule_graphs, device_batch
from .metrics import PackedFingerprints, _check_nbits
from .smiles import AROMATIC, DOUBLE, SINGLE, TRIPLE
from .smiles_out import table_rows as _symbol_rows

__all__ = ["FingerprintTables", "CircularFingerprints", "circular_fingerprints", "fingerprint_store", "table_words", "NO_GRAPH",
           "MAX_RADIUS"]

NO_GRAPH = -2       # DG_FP_NO_GRAPH: n_features of a molecule whose bond list was truncated
MAX_RADIUS = 4      # DG_FP_MAX_RADIUS
_ORDER2 = {SINGLE: 2, DOUBLE: 4, TRIPLE: 6, AROMATIC: 3}      # twice the bond order


def table_words(atom_decoder, bond_decoder):
    """The two tables as host arrays: ``[n_atom_labels]`` uint32 -- the atomic number of every atom label -- and
    ``[n_bond_labels, 2]`` uint32 -- the RDKit bond-type value (1, 2, 3, 12; 0 for the no-bond label) and twice the bond order
    (2, 4, 6, 3; 0).  The decoders are those of ``smiles_out.table_rows``, checked by it: the same ``ValueError``s."""
    _symbol_rows(atom_decoder, bond_decoder)
    atom_words = np.array([int(atom_decoder[l]) for l in range(len(atom_decoder))], dtype=np.uint32)
    bond_rows = np.array([(int(bond_decoder[l]), _ORDER2.get(int(bond_decoder[l]), 0)) for l in range(len(bond_decoder))],
                         dtype=np.uint32).reshape(-1, 2)
    return atom_words, bond_rows


class FingerprintTables:
    """The two tables of ``dg_mol_fingerprint`` on a device (``table_words``); the kernel itself knows no chemistry."""

    def __init__(self, atom_words, bond_rows, device):
        self.atom_words, self.bond_rows = atom_words, bond_rows
        self.n_atom_labels, self.n_bond_labels = len(atom_words), len(bond_rows)
        self.atoms = torch.from_numpy(atom_words.view(np.int32)).to(device).contiguous()      # (the bit patterns)
        self.bonds = torch.from_numpy(bond_rows.view(np.int32)).to(device).contiguous()
        self.device = self.atoms.device      # with its index, as a batch's buffer reports it

    @classmethod
    def from_decoders(cls, atom_decoder, bond_decoder, device):
        """Build and upload the tables; ``ValueError`` on an unknown atomic number or bond type, on labels that are not
        0..n-1 and on more than 255 atom labels (``SmilesTables.from_decoders``' errors)."""
        return cls(*table_words(atom_decoder, bond_decoder), device)


@dataclass
class CircularFingerprints(PackedFingerprints):
    """``metrics.PackedFingerprints`` -- ``words`` [n, nbits / 32] int32, ``counts`` [n] int32, ``nbits`` -- plus
    ``n_features`` [n] int32: the number of distinct features before folding, -2 (``NO_GRAPH``) for a molecule whose bond list
    was truncated (its words are zero).  Every function of ``druggen_amd.metrics`` takes it as it is."""
    n_features: torch.Tensor = None

    @staticmethod
    def empty(n, nbits, device):
        """Device fingerprints over uninitialised memory (``circular_fingerprints(..., out=)`` fills every element)."""
        _check_nbits(nbits)
        return CircularFingerprints(torch.empty((n, nbits // 32), dtype=torch.int32, device=device),
                                    torch.empty((n,), dtype=torch.int32, device=device), nbits,
                                    torch.empty((n,), dtype=torch.int32, device=device))

    def cpu(self):
        """Host copies of the three tensors (three device->host transfers; this one synchronises)."""
        return CircularFingerprints(self.words.cpu(), self.counts.cpu(), self.nbits, self.n_features.cpu())


def _check_radius(radius):
    radius = int(radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be 0..{MAX_RADIUS}, got {radius}")
    return radius


def _launch(batch, tables, code, radius, out, at=0):
    """``dg_mol_fingerprint`` of ``batch`` into the rows ``at ..`` of ``out``."""
    if batch.B == 0:
        return
    cap = batch.cap
    largest = code == SCOPES["largest"]
    _lib.launch("dg_mol_fingerprint", batch.buffer,
                batch.atoms.data_ptr(), batch.bonds.data_ptr() if cap > 0 else None, batch.n_bonds.data_ptr(),
                batch.component.data_ptr() if largest else None, batch.largest.data_ptr() if largest else None, None,
                tables.atoms.data_ptr(), tables.n_atom_labels, tables.bonds.data_ptr(), tables.n_bond_labels,
                batch.B, batch.N, cap, code, radius, out.nbits,
                out.words[at:].data_ptr(), out.counts[at:].data_ptr(), out.n_features[at:].data_ptr())


def _check_tables(tables, who, dev):
    if not isinstance(tables, FingerprintTables):
        raise TypeError(f"{who} takes FingerprintTables (FingerprintTables.from_decoders)")
    if tables.device != dev:
        raise ValueError(f"the tables live on {tables.device}, the molecules on {dev}")


def circular_fingerprints(batch, tables, radius=2, nbits=1024, scope="largest", out=None):
    """``CircularFingerprints`` of a device ``MoleculeBatch``, on its device and the current stream.

    ``radius`` 0..4 (2: the ECFP4 neighbourhood the reference's Morgan fingerprints use), ``nbits`` a multiple of 32 in
    32..4096.  ``scope``: ``"largest"`` -- the largest fragment -- or ``"whole"`` -- every atom except isolated pads; the
    membership rule of ``canon.canonical_forms``.  ``out``: a ``CircularFingerprints.empty(B, nbits, device)`` to write into.
    One launch; every element is written by every call, nothing is allocated with ``out=`` and nothing synchronises:
    capturable."""
    device_batch(batch, "circular_fingerprints", "fingerprint")
    code = _scope_code(scope)
    radius = _check_radius(radius)
    nbits = int(nbits)
    _check_nbits(nbits)
    dev = batch.buffer.device
    _check_tables(tables, "circular_fingerprints", dev)
    B = batch.B
    if out is None:
        out = CircularFingerprints.empty(B, nbits, dev)
    elif (not isinstance(out, CircularFingerprints) or out.nbits != nbits or tuple(out.words.shape) != (B, nbits // 32)
            or tuple(out.counts.shape) != (B,) or tuple(out.n_features.shape) != (B,)
            or any(t.device != dev or t.dtype != torch.int32 or not t.is_contiguous()
                   for t in (out.words, out.counts, out.n_features))):
        raise ValueError("out= must be device CircularFingerprints of this batch's B and nbits (CircularFingerprints.empty)")
    _launch(batch, tables, code, radius, out)
    return out


def fingerprint_store(store, tables, chunk=1024, radius=2, nbits=1024, scope="largest", bond_cap=None):
    """``CircularFingerprints`` of every molecule of a ``resident.ResidentMolecules`` store, ``chunk`` molecules at a time by
    the route of ``CanonicalSet.from_store``: ``store.batch`` -> ``decode_molecule_graphs`` (the one-hots serve as logits) ->
    ``dg_mol_fingerprint``, written at the row offsets of one ``[n, nbits / 32]`` result.  The result does not depend on
    ``chunk``."""
    code = _scope_code(scope)
    radius = _check_radius(radius)
    nbits = int(nbits)
    _check_nbits(nbits)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    _check_tables(tables, "fingerprint_store", store.device)
    n, N = len(store), store.vertexes
    cap = N * (N - 1) // 2 if bond_cap is None else int(bond_cap)
    out = CircularFingerprints.empty(n, nbits, store.device)
    for at in range(0, n, chunk):
        index = torch.arange(at, min(n, at + chunk), device=store.device)
        _, a, x = store.batch(index)
        if store.atom_dim != store.m_dim:
            x = x[..., :store.atom_dim].contiguous()
        _launch(decode_molecule_graphs(x, a, bond_cap=cap), tables, code, radius, out, at)
    return out
