"""Uniqueness and novelty up to atom order, on the GPU: canonical forms of decoded molecules.

The reference's ``logging()`` (``src/util/utils.py:241-355``) counts distinct canonical SMILES of the longest fragment
(Uniqueness) and checks them against the input molecules and the drug set (Novelty).  ``monitor.MolStats`` compares decoded graphs
position by position; here ``canonical_forms`` rewrites every molecule of a device ``decode.MoleculeBatch`` in an atom order that
depends on the labelled graph alone (``dg_mol_canon``, ``include/druggen_hip.h``), and ``match_forms`` compares those forms
within the batch and against a stock -- the input batch, a drug store, a training store (``dg_mol_canon_match``).

Equal forms ARE isomorphic labelled graphs (a form is a complete relabelled graph), so every duplicate and every stock hit is
true.  Isomorphic graphs get equal forms whenever the cells the kernel splits are orbits; ``n_splits == 0`` marks the
molecules for which that holds unconditionally.  RDKit's sanitisation is not applied: two kekule drawings of one aromatic ring are
different labelled graphs, so the fractions below bound RDKit's Uniqueness / Novelty much more tightly than the positional ones,
but are not those numbers.  GPU only, no CPU fallback."""
from __future__ import annotations

import torch

from . import _lib
from ._packed import PackedRecord, check_key_bits as _check_key_bits
from .decode import decode_molecule_graphs, device_batch

__all__ = ["canonical_forms", "match_forms", "uniqueness_novelty", "CanonicalForms", "CanonicalSet", "FormMatches", "SCOPES",
           "TOT_FIELDS"]

SCOPES = {"whole": 0, "largest": 1}      # DG_CANON_WHOLE / DG_CANON_LARGEST
TOT_FIELDS = ("B", "n_distinct", "n_in_stock", "n_novel", "n_truncated", "n_unsplit")


class CanonicalForms(PackedRecord):
    """The forms of one batch: typed views of one packed byte buffer.

    ===============  ===============  ===============================================================================
    ``n_atoms``      [B] int32        ``n``: atoms in the scope
    ``n_bonds``      [B] int32        bonds between them
    ``n_splits``     [B] int32        individualisations taken; 0: refinement alone told all atoms apart, the form is
                                      canonical unconditionally; -2: the molecule's bond list was truncated, no form
    ``n_rounds``     [B] int32        refinement rounds taken
    ``key``          [B] int64        hash of the form (selects candidates; never the answer)
    ``order``        [B,N] uint8      original position of the atom of rank r; 0xFF past ``n``
    ``canon_atoms``  [B,N] uint8      its label; 0xFF past ``n``
    ``canon_bonds``  [B,cap,4] uint8  ``(hi rank, lo rank, label, 0)`` ascending in (hi, lo); zeros past ``n_bonds``
    ===============  ===============  ===============================================================================

    ``cpu()`` moves the packed buffer with ONE device->host copy; ``form(b)`` reads the host copy."""

    def __init__(self, buffer, B, N, cap, scope):
        self.B, self.N, self.cap, self.scope = B, N, cap, scope
        super().__init__(buffer, B, N, cap)

    @staticmethod
    def _fields(B, N, cap, scope=None):
        return (("n_atoms", 4, (B,)), ("n_bonds", 4, (B,)), ("n_splits", 4, (B,)), ("n_rounds", 4, (B,)), ("key", 8, (B,)),
                ("order", 1, (B, N)), ("canon_atoms", 1, (B, N)), ("canon_bonds", 1, (B, cap, 4)))

    @staticmethod
    def empty(B, N, cap, device, scope="largest"):
        """Device forms over an uninitialised buffer (``canonical_forms(..., out=)`` fills every element)."""
        return CanonicalForms._empty(device, B, N, cap, scope)

    def form(self, b):
        """``(n_atoms, n_bonds, atom labels, bond rows)`` of molecule ``b`` as plain Python values (host copy only): equal
        exactly when the two molecules are reported as the same.  None for a truncated molecule."""
        self._host("form")
        if self.n_splits[b] < 0:
            return None
        n, nb = int(self.n_atoms[b]), int(self.n_bonds[b])
        return n, nb, tuple(self.canon_atoms[b, :n].tolist()), tuple(map(tuple, self.canon_bonds[b, :nb, :3].tolist()))


_layout = CanonicalForms.layout      # (B, N, cap) -> (name -> (byte offset, bytes, element bytes, shape), size)


def _scope_code(scope):
    try:
        return SCOPES[scope]
    except (KeyError, TypeError):
        raise ValueError(f"scope must be 'largest' or 'whole', got {scope!r}") from None


def _launch_canon(batch, code, forms, at=0):
    """``dg_mol_canon`` of ``batch`` into the rows ``at ..`` of ``forms`` (same N and cap)."""
    if batch.B == 0:
        return
    cap = batch.cap
    _lib.launch("dg_mol_canon", batch.buffer,
                batch.atoms.data_ptr(), batch.bonds.data_ptr() if cap > 0 else None, batch.n_bonds.data_ptr(),
                batch.component.data_ptr(), batch.largest.data_ptr(), batch.B, batch.N, cap, code,
                forms.n_atoms[at:].data_ptr(), forms.n_bonds[at:].data_ptr(), forms.n_splits[at:].data_ptr(),
                forms.n_rounds[at:].data_ptr(), forms.order[at:].data_ptr(), forms.canon_atoms[at:].data_ptr(),
                forms.canon_bonds[at:].data_ptr() if cap > 0 else None, forms.key[at:].data_ptr())


def canonical_forms(batch, scope="largest", out=None):
    """``CanonicalForms`` of a device ``MoleculeBatch`` (``decode.decode_molecule_graphs``), on its device and the current stream.

    ``scope``: ``"largest"`` -- the atoms of the largest fragment, what ``logging()`` compares -- or ``"whole"`` -- every atom
    except isolated pads (label 0 and no bond).  ``out``: a ``CanonicalForms.empty(B, N, cap, device)`` to write into.  One
    launch; every element is written by every call, nothing is allocated with ``out=`` and nothing synchronises, so the call can
    be captured into a hipGraph."""
    device_batch(batch, "canonical_forms", "canon")
    code = _scope_code(scope)
    B, N, cap = batch.B, batch.N, batch.cap
    dev = batch.buffer.device
    if out is None:
        out = CanonicalForms.empty(B, N, cap, dev, scope)
    elif (not isinstance(out, CanonicalForms) or out.is_host or (out.B, out.N, out.cap) != (B, N, cap)
            or out.buffer.device != dev):
        raise ValueError("out= must be a device CanonicalForms of this batch's B, N and bond_cap (CanonicalForms.empty)")
    out.scope = scope
    _launch_canon(batch, code, out)
    return out


class CanonicalSet:
    """A stock of forms to look molecules up in: the forms in their original order, their keys -- masked to ``key_bits`` bits --
    sorted ascending, and the sorted position -> original index table (ascending inside a run of equal keys)."""

    def __init__(self, forms, keys, index, key_bits):
        self.forms, self.keys, self.index, self.key_bits = forms, keys, index, key_bits

    def __len__(self):
        return self.forms.B

    @classmethod
    def from_forms(cls, forms, key_bits=64):
        """Sort the keys of device ``forms`` on the device (``torch.sort(stable=True)``); ``forms`` is kept, not copied."""
        if not isinstance(forms, CanonicalForms):
            raise TypeError("CanonicalSet.from_forms takes CanonicalForms")
        if forms.is_host:
            raise RuntimeError("druggen_amd.canon runs on the GPU (no CPU fallback): pass the device CanonicalForms")
        _check_key_bits(key_bits)
        keys = forms.key if key_bits == 64 else forms.key & ((1 << key_bits) - 1)
        keys, index = torch.sort(keys, stable=True)
        return cls(forms, keys.contiguous(), index.to(torch.int32).contiguous(), key_bits)

    @classmethod
    def from_store(cls, store, chunk=1024, scope="largest", key_bits=64, bond_cap=None):
        """The forms of every molecule of a ``resident.ResidentMolecules`` store, ``chunk`` molecules at a time through
        ``store.batch`` -> ``decode_molecule_graphs`` (the one-hots serve as logits) -> ``dg_mol_canon``."""
        code = _scope_code(scope)
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        n, N = len(store), store.vertexes
        cap = N * (N - 1) // 2 if bond_cap is None else int(bond_cap)
        forms = CanonicalForms.empty(n, N, cap, store.device, scope)
        for at in range(0, n, chunk):
            index = torch.arange(at, min(n, at + chunk), device=store.device)
            _, a, x = store.batch(index)
            if store.atom_dim != store.m_dim:
                x = x[..., :store.atom_dim].contiguous()
            _launch_canon(decode_molecule_graphs(x, a, bond_cap=cap), code, forms, at)
        return cls.from_forms(forms, key_bits)


class FormMatches(PackedRecord):
    """What ``match_forms`` found: typed views of one packed byte buffer (``tot`` first, then ``match``).

    ``match`` [B,2] int32: ``duplicate_of`` -- smallest ``j < b`` with an equal form, -1 none, -2 truncated -- and ``stock_hit``
    -- smallest original stock index with an equal form, -1 none, -2 truncated, -3 no stock given.  ``tot`` [8] int64
    (``TOT_FIELDS``): B, ``n_distinct`` (``duplicate_of == -1``), ``n_in_stock``, ``n_novel`` (``stock_hit == -1``),
    ``n_truncated``, ``n_unsplit`` (``n_splits == 0``), zeros.  The fractions read the host copy (``cpu()``: one transfer)."""

    TOT_FIELDS = TOT_FIELDS
    _PAD_END = False      # 64 + 8 B bytes: the buffer ends with its last row

    def __init__(self, buffer, B):
        self.B = B
        super().__init__(buffer, B)

    @staticmethod
    def _fields(B):
        return ("tot", 8, (8,)), ("match", 4, (B, 2))

    @staticmethod
    def empty(B, device):
        return FormMatches._empty(device, B)

    @property
    def duplicate_of(self):
        return self.match[:, 0]

    @property
    def stock_hit(self):
        return self.match[:, 1]

    def _over_complete(self, name):
        complete = self.B - self.total("n_truncated")
        return self.total(name) / complete if complete else float("nan")

    @property
    def unique_fraction(self):
        """``n_distinct / (B - n_truncated)``: distinct forms among the molecules that have one."""
        return self._over_complete("n_distinct")

    @property
    def novel_fraction(self):
        """``n_novel / (B - n_truncated)``: molecules whose form is not in the stock (nan without a stock: nothing is novel
        or known then)."""
        if self.total("n_novel") + self.total("n_in_stock") == 0:
            return float("nan")
        return self._over_complete("n_novel")

    @property
    def unsplit_fraction(self):
        """``n_unsplit / (B - n_truncated)``: molecules whose form is canonical unconditionally."""
        return self._over_complete("n_unsplit")


def match_forms(forms, stock=None, key_bits=64, out=None):
    """``FormMatches`` of device ``forms``: duplicates within the batch and, with ``stock`` (a ``CanonicalSet``), membership in
    it.  ``key_bits`` (1..64): width of the keys that select candidates; every key match is verified byte by byte, so the result
    does not depend on it -- but a stock has to be sorted under the same width (``CanonicalSet.from_forms(..., key_bits)``).
    ``out``: a ``FormMatches.empty(B, device)``.  Two launches, no allocation with ``out=``, no synchronisation: capturable."""
    if not isinstance(forms, CanonicalForms):
        raise TypeError("match_forms takes CanonicalForms")
    if forms.is_host or not forms.buffer.is_cuda:
        raise RuntimeError("druggen_amd.canon runs on the GPU (no CPU fallback): pass the device CanonicalForms")
    _check_key_bits(key_bits)
    B, N, cap = forms.B, forms.N, forms.cap
    dev = forms.buffer.device
    S, s_cap, s = 0, 0, None
    if stock is not None:
        if not isinstance(stock, CanonicalSet):
            raise TypeError("stock must be a CanonicalSet (CanonicalSet.from_forms / from_store)")
        s = stock.forms
        if s.N != N:
            raise ValueError(f"the stock holds molecules of N = {s.N} positions, the batch of N = {N}")
        if stock.key_bits != key_bits:
            raise ValueError(f"the stock was sorted under key_bits = {stock.key_bits}, not {key_bits}: sort it again "
                             "(CanonicalSet.from_forms(stock.forms, key_bits))")
        if s.buffer.device != dev:
            raise ValueError(f"the stock lives on {s.buffer.device}, the batch on {dev}")
        S, s_cap = s.B, s.cap
    if out is None:
        out = FormMatches.empty(B, dev)
    elif not isinstance(out, FormMatches) or out.is_host or out.B != B or out.buffer.device != dev:
        raise ValueError("out= must be a device FormMatches of this batch's B (FormMatches.empty)")
    none = [None] * 7
    _lib.launch("dg_mol_canon_match", forms.buffer,
                forms.key.data_ptr(), forms.n_atoms.data_ptr(), forms.n_bonds.data_ptr(), forms.n_splits.data_ptr(),
                forms.canon_atoms.data_ptr(), forms.canon_bonds.data_ptr() if cap > 0 else None, B, N, cap,
                *(none if S == 0 else [stock.keys.data_ptr(), stock.index.data_ptr(), s.n_atoms.data_ptr(), s.n_bonds.data_ptr(),
                                       s.n_splits.data_ptr(), s.canon_atoms.data_ptr(),
                                       s.canon_bonds.data_ptr() if s_cap > 0 else None]),
                S, s_cap, key_bits, out.match.data_ptr(), out.tot.data_ptr())
    return out


def uniqueness_novelty(batch, stock=None, scope="largest"):
    """``(forms, matches)`` of a device ``MoleculeBatch``: ``canonical_forms`` then ``match_forms`` (three launches).  A stock
    built under another scope is refused: its forms describe other atom sets."""
    if stock is not None and isinstance(stock, CanonicalSet) and stock.forms.scope != scope:
        raise ValueError(f"the stock's forms were made with scope = {stock.forms.scope!r}, not {scope!r}")
    forms = canonical_forms(batch, scope)
    return forms, match_forms(forms, stock, 64 if stock is None else stock.key_bits)
