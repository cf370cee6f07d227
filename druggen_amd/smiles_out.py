"""SMILES strings of decoded molecules, written on the GPU (``dg_mol_smiles``, ``include/druggen_hip_text.h``).

The reference's end product is lists of SMILES (``mol_sample`` / ``save_smiles_matrices`` of ``src/util/utils.py``,
``inference.py``, the CSVs under ``results/``), written by RDKit on the host.  ``write_smiles`` writes one string per molecule
of a device ``decode.MoleculeBatch`` -- or of a device ``canon.CanonicalForms``, and then equal forms give equal bytes: a
canonical SMILES in the project's own sense, up to atom order, not up to RDKit's sanitisation -- in the dialect
``druggen_amd.smiles.parse_smiles`` reads back to exactly the graph that was written.

Not written: hydrogens, charges, isotopes, chirality -- the decoded graph carries none.  Bracket atoms are written bare
(``[Se]``): a reader gives them NO hydrogens, whereas organic-subset atoms get theirs from the reader's valence rule, as with
RDKit.  GPU only, no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._packed import PackedRecord
from .canon import SCOPES, CanonicalForms, _scope_code
from .decode import MoleculeBatch, device_batch
from .smiles import _ELEMENTS, _ORGANIC, AROMATIC, DOUBLE, SINGLE, TRIPLE

__all__ = ["SmilesTables", "SmilesBatch", "write_smiles", "table_rows", "STATUS"]

FORMS = 2      # DG_SMILES_FORMS: the scope code of a CanonicalForms source
STATUS = {-2: "no graph (truncated bond list or no form)", -3: "more than 99 ring closures open at once",
          -4: "longer than str_cap"}      # DG_SMILES_NO_GRAPH / _RINGS / _LONG
_BRACKETS, _LOWER = 1, 2      # flag bits of an atom row
_MAY_BE_LOWER = ("B", "C", "N", "O", "P", "S", "Se", "As")      # what parse_smiles reads in lower case
_BOND_SYMBOLS = {SINGLE: "-", DOUBLE: "=", TRIPLE: "#", AROMATIC: ":"}


def table_rows(atom_decoder, bond_decoder):
    """The two symbol tables as host arrays: ``[n_atom_labels, 4]`` uint8 -- two symbol characters (the second 0 if none), a
    flag byte (bit 0: needs brackets, bit 1: may be written lower-case), 0 -- and ``[n_bond_labels, 2]`` uint8 -- the symbol
    character and an is-aromatic flag.  ``atom_decoder``: label -> atomic number (0: written ``*``), ``bond_decoder``: label
    -> RDKit bond-type value (0: no bond, never written), as ``smiles.build_encoders`` returns them; the labels are 0..n-1."""
    tables = []
    for name, decoder, most in (("atom_decoder", atom_decoder, 255), ("bond_decoder", bond_decoder, 256)):
        labels = sorted(decoder)
        if not labels or labels != list(range(len(labels))):
            raise ValueError(f"{name} must map the labels 0..n-1, got {labels}")
        if len(labels) > most:
            raise ValueError(f"{name} has {len(labels)} labels, a label is one byte (at most {most}; atom label 0xFF marks an "
                             "atom outside a form)")
        tables.append(labels)
    atom_rows = np.zeros((len(tables[0]), 4), dtype=np.uint8)
    for l in tables[0]:
        z = int(atom_decoder[l])
        if z == 0:
            sym, flags = "*", 0
        elif 2 <= z <= len(_ELEMENTS):
            sym = _ELEMENTS[z - 1]
            flags = (0 if sym in _ORGANIC else _BRACKETS) | (_LOWER if sym in _MAY_BE_LOWER else 0)
        else:
            raise ValueError(f"atom label {l}: atomic number {z} is not one druggen_amd.smiles reads (0, 2..{len(_ELEMENTS)}; "
                             "hydrogens are not written)")
        atom_rows[l, :len(sym)] = list(sym.encode("ascii"))
        atom_rows[l, 2] = flags
    bond_rows = np.zeros((len(tables[1]), 2), dtype=np.uint8)
    for l in tables[1]:
        t = int(bond_decoder[l])
        if t == 0:
            continue
        if t not in _BOND_SYMBOLS:
            raise ValueError(f"bond label {l}: bond type {t} is not one of SINGLE 1, DOUBLE 2, TRIPLE 3, AROMATIC 12")
        bond_rows[l] = ord(_BOND_SYMBOLS[t]), t == AROMATIC
    return atom_rows, bond_rows


class SmilesTables:
    """The two symbol tables of ``dg_mol_smiles`` on a device (``table_rows``); the kernel itself knows no chemistry."""

    def __init__(self, atom_rows, bond_rows, device):
        self.atom_rows, self.bond_rows = atom_rows, bond_rows
        self.n_atom_labels, self.n_bond_labels = len(atom_rows), len(bond_rows)
        self.atoms = torch.from_numpy(atom_rows).to(device).contiguous()
        self.bonds = torch.from_numpy(bond_rows).to(device).contiguous()
        self.device = self.atoms.device      # with its index, as a batch's buffer reports it

    @classmethod
    def from_decoders(cls, atom_decoder, bond_decoder, device):
        """Build and upload the tables; ``ValueError`` on an unknown atomic number or bond type, on labels that are not
        0..n-1 and on more than 255 atom labels."""
        return cls(*table_rows(atom_decoder, bond_decoder), device)


class SmilesBatch(PackedRecord):
    """The strings of one batch: typed views of one packed byte buffer.

    ===============  ===================  ==========================================================================
    ``length``       [B] int32            the string's length; -2: no graph (truncated bond list, or a form with
                                          ``n_splits`` < 0); -3: more than 99 ring closures open at once; -4: longer
                                          than ``str_cap``
    ``n_written``    [B] int32            atoms of the scope (0 with -2)
    ``order``        [B,N] uint8          the atom index of the k-th atom of the string; 0xFF past ``n_written``
    ``text``         [B,str_cap] uint8    ASCII, zeros past ``length``, all zeros when ``length`` < 0
    ===============  ===================  ==========================================================================

    ``cpu()`` moves the packed buffer with ONE device->host copy; ``strings()`` reads the host copy."""

    def __init__(self, buffer, B, N, str_cap):
        self.B, self.N, self.str_cap = B, N, str_cap
        super().__init__(buffer, B, N, str_cap)

    @staticmethod
    def _fields(B, N, str_cap):
        return ("length", 4, (B,)), ("n_written", 4, (B,)), ("order", 1, (B, N)), ("text", 1, (B, str_cap))

    @staticmethod
    def empty(B, N, str_cap, device):
        """A device record over an uninitialised buffer (``write_smiles(..., out=)`` fills every element)."""
        return SmilesBatch._empty(device, B, N, str_cap)

    def strings(self):
        """One ``str`` per molecule, ``None`` where ``length`` < 0 (``STATUS`` names the reasons); host copy only."""
        self._host("strings")
        return [self.text[b, :n].tobytes().decode("ascii") if n >= 0 else None for b, n in enumerate(self.length.tolist())]


_layout = SmilesBatch.layout      # (B, N, str_cap) -> (name -> (byte offset, bytes, element bytes, shape), size)


def write_smiles(source, tables, scope="largest", str_cap=None, out=None):
    """``SmilesBatch`` of a device ``MoleculeBatch`` or a device ``CanonicalForms``, on its device and the current stream.

    ``scope`` (a ``MoleculeBatch``): ``"largest"`` -- the largest fragment -- or ``"whole"`` -- every atom except isolated
    pads, the fragments joined with ``.``; the membership rule of ``canon.canonical_forms``.  A ``CanonicalForms`` carries its
    scope with it (another ``scope`` is an error: forms made under ``"whole"`` take ``scope="whole"``) and is written in rank order: equal forms give equal strings.  ``str_cap``:
    bytes per string, None = 8 N.  ``out``: a ``SmilesBatch.empty(B, N, str_cap, device)`` to write into.  One launch; every
    element is written by every call, nothing is allocated with ``out=`` and nothing synchronises: capturable."""
    if not isinstance(tables, SmilesTables):
        raise TypeError("write_smiles takes SmilesTables (SmilesTables.from_decoders)")
    if isinstance(source, CanonicalForms):
        if source.is_host or not source.buffer.is_cuda:
            raise RuntimeError("druggen_amd.smiles_out runs on the GPU (no CPU fallback): pass the device CanonicalForms")
        if not 1 <= source.N <= 256:
            raise ValueError(f"write_smiles: 1 <= N <= 256, got {source.N}")
        if scope != source.scope:
            raise ValueError(f"the forms were made with scope = {source.scope!r}, not {scope!r}: a CanonicalForms carries its scope")
        code = FORMS
        atoms, bonds, n_bonds, component, largest, flags = (source.canon_atoms, source.canon_bonds, source.n_bonds, None, None,
                                                            source.n_splits)
    else:
        device_batch(source, "write_smiles", "smiles_out")
        code = _scope_code(scope)
        atoms, bonds, n_bonds, flags = source.atoms, source.bonds, source.n_bonds, None
        component, largest = (source.component, source.largest) if code == SCOPES["largest"] else (None, None)
    B, N, cap = source.B, source.N, source.cap
    dev = source.buffer.device
    if tables.device != dev:
        raise ValueError(f"the tables live on {tables.device}, the batch on {dev}")
    str_cap = 8 * N if str_cap is None else int(str_cap)
    if str_cap < 1:
        raise ValueError(f"str_cap must be >= 1, got {str_cap}")
    if out is None:
        out = SmilesBatch.empty(B, N, str_cap, dev)
    elif (not isinstance(out, SmilesBatch) or out.is_host or (out.B, out.N, out.str_cap) != (B, N, str_cap)
            or out.buffer.device != dev):
        raise ValueError("out= must be a device SmilesBatch of this batch's B, N and str_cap (SmilesBatch.empty)")
    if B == 0:
        return out
    _lib.launch("dg_mol_smiles", source.buffer,
                atoms.data_ptr(), bonds.data_ptr() if cap > 0 else None, n_bonds.data_ptr(),
                None if component is None else component.data_ptr(), None if largest is None else largest.data_ptr(),
                None if flags is None else flags.data_ptr(), tables.atoms.data_ptr(), tables.n_atom_labels,
                tables.bonds.data_ptr(), tables.n_bond_labels, B, N, cap, code, str_cap,
                out.length.data_ptr(), out.n_written.data_ptr(), out.order.data_ptr(), out.text.data_ptr())
    return out
