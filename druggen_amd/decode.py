"""Argmax decode on the GPU (reference ``inference.py:197-198``,
``src/util/utils.py:220-221``): logits -> compact uint8 label tensors, so the
CPU-side RDKit ``matrices2mol`` receives bytes instead of float logits.

``decode_molecule_graphs`` goes the rest of the way to what ``matrices2mol`` (``dataset.py:218-223``) reads: per
molecule the atom labels, the bond LIST in ``np.nonzero`` order (``start > end``), the connected components and twice
the valence of every atom -- one launch for the batch (``dg_decode_graph``), one device->host copy (``MoleculeBatch.cpu``)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._packed import PackedRecord, uploaded
from .functional import _c

__all__ = ["argmax_labels", "decode_molecule_labels", "decode_molecule_graphs", "MoleculeBatch"]


def argmax_labels(logits):
    """``torch.max(logits, -1)[1]`` as uint8 (classes <= 255)."""
    if not logits.is_cuda:
        raise RuntimeError("druggen_amd.decode runs on the GPU (no CPU fallback)")
    x = _c(logits.detach())
    E = x.shape[-1]
    rows = x.numel() // E
    out = torch.empty(x.shape[:-1], dtype=torch.uint8, device=x.device)
    _lib.launch("dg_argmax_decode", x, _lib.ptr(x), rows, E, out.data_ptr())
    return out


def decode_molecule_labels(node_sample, edge_sample):
    """(atom labels [B,N], bond labels [B,N,N]) from the Generator's logits."""
    return argmax_labels(node_sample), argmax_labels(edge_sample)


# ---- graph decode ---------------------------------------------------------------------------------------------------
_FIELDS = ("n_bonds", "n_components", "largest", "largest_size", "atoms", "component", "valence2", "bonds")


class MoleculeBatch(PackedRecord):
    """The decoded batch: typed views of one packed byte buffer.

    =============================================  =====================================================================
    ``atoms``        [B,N]     uint8               atom label per position
    ``bonds``        [B,cap,4] uint8               ``(start, end, label, 0)`` per bond, ``start > end``, in the order
                                                   ``zip(*np.nonzero(labels))`` yields them; rows past
                                                   ``min(n_bonds, cap)`` are unwritten memory
    ``n_bonds``      [B]       int32               the true bond count (``> cap``: the list was truncated)
    ``component``    [B,N]     uint8               smallest atom index of the atom's connected component
    ``n_components``, ``largest``, ``largest_size`` [B] int32   component count; the component with the most atoms
                                                   (ties: the smaller label) and its atom count
    ``valence2``     [B,N]     uint16 or None      sum of ``bond_order2[label]`` over the atom's bonds
    =============================================  =====================================================================

    On the device the fields are ``torch`` tensors.  ``cpu()`` moves the packed buffer with ONE device->host copy and
    returns a host batch whose fields are ``numpy`` views of it; ``edge_list`` / ``edge_labels`` / ``truncated`` work on
    the host batch.  ``validity``: the ``validity.MoleculeValidity`` of a batch sampled by ``MoleculeSampler(..., validity=)``,
    else None; ``descriptors``: the ``descriptors.MoleculeDescriptors`` of one sampled with ``descriptors=`` too, else None;
    ``matches``: the ``substructure.MoleculeMatches`` of one sampled with ``substructures=`` as well, else None; ``scaffolds``: the
    ``scaffolds.MoleculeScaffolds`` of one sampled with ``scaffolds=True``, else None."""

    validity = None
    descriptors = None
    matches = None
    scaffolds = None

    def __init__(self, buffer, B, N, cap, with_valence):
        self.B, self.N, self.cap = B, N, cap
        self.valence2 = None
        super().__init__(buffer, B, N, cap, with_valence)

    @staticmethod
    def _fields(B, N, cap, with_valence):
        sizes = {"atoms": (1, (B, N)), "component": (1, (B, N)), "valence2": (2, (B, N)), "bonds": (1, (B, cap, 4))}
        return [(name, *sizes.get(name, (4, (B,)))) for name in _FIELDS if name != "valence2" or with_valence]

    @staticmethod
    def empty(B, N, cap, with_valence, device):
        """A device batch over an uninitialised buffer (``decode_molecule_graphs(..., out=)`` fills it)."""
        return MoleculeBatch._empty(device, B, N, cap, with_valence)

    @property
    def truncated(self):
        """Mask [B]: the molecule has more bonds than ``cap`` rows."""
        return self.n_bonds > self.cap

    def edge_list(self, b):
        """``(start, end, label)`` triples of molecule ``b`` as an ``[n, 3]`` uint8 array, in ``matrices2mol``'s order."""
        self._host("edge_list")
        return self.bonds[b, :min(int(self.n_bonds[b]), self.cap), :3]

    def edge_labels(self, b):
        """The dense ``[N,N]`` bond-label matrix of molecule ``b`` rebuilt from its list: lower triangle only (what
        ``matrices2mol`` keeps of the dense argmax), zeros elsewhere."""
        self._host("edge_labels")
        e = self.edge_list(b)
        dense = np.zeros((self.N, self.N), dtype=np.uint8)
        dense[e[:, 0], e[:, 1]] = e[:, 2]
        return dense


_layout = MoleculeBatch.layout      # (B, N, cap, with_valence) -> (name -> (byte offset, bytes, element bytes, shape), size)


def device_batch(batch, who, module):
    """``who`` (a function of ``druggen_amd.<module>``) takes a device ``MoleculeBatch`` of 1 <= N <= 256."""
    if not isinstance(batch, MoleculeBatch):
        raise TypeError(f"{who} takes a decode.MoleculeBatch")
    if batch.is_host or not batch.buffer.is_cuda:
        raise RuntimeError(f"druggen_amd.{module} runs on the GPU (no CPU fallback): pass the device MoleculeBatch")
    if not 1 <= batch.N <= 256:
        raise ValueError(f"{who}: 1 <= N <= 256, got {batch.N}")


def _order2_table(bond_order2, E, device):
    if bond_order2 is None:
        return None
    if torch.is_tensor(bond_order2):
        t = bond_order2
        if t.dtype != torch.uint8 or t.device != device:
            t = t.to(device=device, dtype=torch.uint8)
    else:
        vals = tuple(int(v) for v in bond_order2)
        if any(v < 0 or v > 255 for v in vals):
            raise ValueError("bond_order2 holds twice the bond order of every bond label as a byte (0..255)")
        t = uploaded(vals, np.uint8, device)
    if t.dim() != 1 or t.shape[0] != E:
        raise ValueError(f"bond_order2 needs one entry per bond label ({E}), got shape {tuple(t.shape)}")
    return _c(t)


def decode_molecule_graphs(node_sample, edge_sample, *, bond_order2=None, bond_cap=None, out=None):
    """Generator logits ``node_sample`` [B,N,M], ``edge_sample`` [B,N,N,E] -> ``MoleculeBatch`` on their device.

    ``bond_order2``: twice the bond order of every bond label (a sequence or uint8 tensor of E entries, e.g.
    ``[0, 2, 4, 6, 3]`` for no bond / single / double / triple / aromatic) -- asks for ``valence2``.  ``bond_cap``: rows
    of the bond list per molecule; None = N (N - 1) / 2, which nothing can exceed.  ``out``: a device ``MoleculeBatch``
    of the same geometry to write into (``MoleculeBatch.empty``) instead of a fresh buffer."""
    if not (node_sample.is_cuda and edge_sample.is_cuda):
        raise RuntimeError("druggen_amd.decode runs on the GPU (no CPU fallback)")
    if node_sample.dim() != 3 or edge_sample.dim() != 4:
        raise ValueError("decode_molecule_graphs takes node logits [B,N,M] and edge logits [B,N,N,E]")
    B, N, M = node_sample.shape
    E = edge_sample.shape[-1]
    if tuple(edge_sample.shape) != (B, N, N, E) or edge_sample.device != node_sample.device:
        raise ValueError(f"edge logits {tuple(edge_sample.shape)} do not belong to node logits {tuple(node_sample.shape)}")
    x, e = _c(node_sample.detach()), _c(edge_sample.detach())
    cap = N * (N - 1) // 2 if bond_cap is None else int(bond_cap)
    if cap < 0:
        raise ValueError("bond_cap must be >= 0")
    order2 = _order2_table(bond_order2, E, x.device)
    if out is None:
        out = MoleculeBatch.empty(B, N, cap, order2 is not None, x.device)
    elif (out.is_host or (out.B, out.N, out.cap) != (B, N, cap) or (out.valence2 is not None) != (order2 is not None)
            or out.buffer.device != x.device):
        raise ValueError("out= must be a device MoleculeBatch of this batch's B, N, bond_cap and valence2 choice")
    if B == 0:
        return out
    _lib.launch("dg_decode_graph", x, _lib.fptr(x), _lib.fptr(e), None if order2 is None else order2.data_ptr(), B, N, M, E,
                cap, out.atoms.data_ptr(), out.bonds.data_ptr() if cap > 0 else None, out.n_bonds.data_ptr(),
                out.component.data_ptr(), out.n_components.data_ptr(), out.largest.data_ptr(), out.largest_size.data_ptr(),
                None if order2 is None else out.valence2.data_ptr())
    return out
