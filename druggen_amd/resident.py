"""A molecule set that stays on the GPU, and training batches assembled from it by index.

The reference feeds its training step through three PyG ``DataLoader``s (``train.py:97-115``, ``inference.py:93-96``):
``B`` ``Data`` objects are collated on the host, four tensors cross PCIe, and ``load_molecules`` densifies them
(``druggen_amd.data``: two memsets and two launches).  The set itself is small in compact form -- one byte per atom
position and one 32-bit word per directed bond -- so ``ResidentMolecules`` uploads it ONCE and builds any batch from an
int64 index tensor with one kernel (``dg_mol_gather``, csrc/mol_gather.hip):

    store = ResidentMolecules.from_graphs(graphs)            # smiles.MolGraph or PyG Data objects
    for idx in store.epoch(batch_size):                      # int64 GPU index tensors, shuffled on the device
        real_graphs, a_tensor, x_tensor = store.batch(idx)   # == load_molecules(collate([graphs[i] for i in idx]))

The result is bit-identical to ``load_molecules``', ``a_tensor`` carries its int32 labels
(``functional.attach_one_hot_labels``), nothing synchronises with the host, and the call can be captured in a hipGraph
(``out=`` writes into the static buffers of a graphed step or sampler).

Store layout (also the C ABI, include/druggen_hip.h): ``atoms`` uint8 ``[n, N]`` (PAD = 0), ``ptr`` int64 ``[n + 1]``,
``entries`` one word per non-zero of a molecule's dense ``[N, N]`` bond-label matrix, ``row | col << 8 | label << 16``.

Node matrices are one-hot by default.  The reference's ``--features`` matrices (``dataset.py:305-307``: the one-hot atom type
followed by 54 boolean descriptors) are taken with ``atom_dim=``: the first ``atom_dim`` columns of ``x`` must be one-hot and
are the ``atoms`` byte, the other ``F = m_dim - atom_dim`` columns must be exactly 0 or 1 and are kept as a bit plane,
``bits`` int32 ``[n, N, ceil(F / 32)]`` (feature ``f`` = bit ``f % 32`` of word ``f // 32``, the packing of DESIGN 3.20):

    store = ResidentMolecules.from_graphs(graphs, atom_dim=13)     # x [N, 13 + 54]: 9 bytes per atom position
    real_graphs, a_tensor, x_tensor = store.batch(idx)             # x_tensor [B, N, 67], as load_molecules returns it

Such a store launches ``dg_mol_gather_features`` (include/druggen_hip.h); everything else is the same.

GPU only, no CPU fallback (``pack`` and ``split_batch`` are host-side numpy)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .functional import attach_one_hot_labels

__all__ = ["ResidentMolecules", "epoch_batches", "MAX_VERTEXES", "MAX_B_DIM", "MAX_M_DIM"]

MAX_VERTEXES, MAX_B_DIM, MAX_M_DIM = 256, 16, 255      # dg_mol_gather: row / col in a byte each, E <= 16, atom label in a byte

_SLOT_CHUNK = 64          # pinned counters are allocated this many at a time (a pinned allocation synchronises the device)
_side_streams = {}        # device index -> the stream that carries the counters' device -> host copies


def _side_stream(dev):
    st = _side_streams.get(dev.index)
    if st is None:
        st = _side_streams[dev.index] = torch.cuda.Stream(dev)
    return st


def _host_array(t, what, i):
    if torch.is_tensor(t):
        if t.is_cuda:
            raise ValueError(f"molecule {i}: {what} is a GPU tensor; ResidentMolecules.pack runs on the host "
                             "(numpy arrays or CPU tensors)")
        t = t.detach().numpy()
    return np.asarray(t)


def _integers(t, what, i):
    t = _host_array(t, what, i)
    if t.dtype.kind not in "iu":
        if t.dtype.kind != "f" or not np.array_equal(t, np.rint(t)):
            raise ValueError(f"molecule {i}: {what} must hold integers, got dtype {t.dtype}")
    return t.astype(np.int64)


def epoch_batches(order, batch_size: int, drop_last: bool = True):
    """The batches of one epoch as consecutive slices of the permutation ``order`` (a 1-D tensor, any device); the last,
    shorter one only with ``drop_last=False`` -- ``DataLoader``'s rule."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    n = int(order.shape[0])
    stop = n - n % batch_size if drop_last else n
    for i in range(0, stop, batch_size):
        yield order[i:min(i + batch_size, n)]


class ResidentMolecules:
    """``atoms`` uint8 ``[n, vertexes]``, ``ptr`` int64 ``[n + 1]``, ``entries`` int32 (the bit patterns of the uint32 words)
    on one GPU; ``n`` molecules of ``vertexes`` atom positions, ``m_dim`` node columns, ``b_dim`` bond classes.  With a feature
    plane: ``bits`` int32 ``[n, vertexes, ceil((m_dim - atom_dim) / 32)]`` (bit patterns again) and ``atom_dim``, the width of
    the one-hot part of a node row; without one ``atom_dim == m_dim``."""

    def __init__(self, atoms, ptr, entries, m_dim: int, b_dim: int, bits=None, atom_dim=None):
        arrays = [(atoms, torch.uint8, "atoms"), (ptr, torch.int64, "ptr"), (entries, torch.int32, "entries")]
        if bits is not None:
            arrays.append((bits, torch.int32, "bits"))
        for t, dtype, name in arrays:
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"druggen_amd.resident keeps the molecule set on the GPU (no CPU fallback); {name} is not a GPU tensor")
            if t.dtype != dtype or not t.is_contiguous() or t.device != atoms.device:
                raise ValueError(f"{name} must be a contiguous {dtype} tensor on the store's device")
        if atoms.dim() != 2 or ptr.dim() != 1 or entries.dim() != 1 or ptr.shape[0] != atoms.shape[0] + 1:
            raise ValueError("ResidentMolecules: atoms [n, N], ptr [n + 1], entries [nnz]")
        self.atoms, self.ptr, self.entries = atoms, ptr, entries
        self.n, self.vertexes = int(atoms.shape[0]), int(atoms.shape[1])
        self.m_dim, self.b_dim = int(m_dim), int(b_dim)
        _check_limits(self.vertexes, self.m_dim, self.b_dim)
        self.bits, self.atom_dim = bits, self.m_dim if atom_dim is None else int(atom_dim)
        if bits is None:
            if self.atom_dim != self.m_dim:
                raise ValueError(f"ResidentMolecules: atom_dim = {self.atom_dim} of m_dim = {self.m_dim} columns needs the feature plane (bits=)")
        else:
            if atom_dim is None or not 1 <= self.atom_dim < self.m_dim:
                raise ValueError(f"ResidentMolecules: a feature plane needs 1 <= atom_dim < m_dim = {self.m_dim}, got atom_dim = {atom_dim}")
            want = (self.n, self.vertexes, _feature_words(self.m_dim - self.atom_dim))
            if tuple(bits.shape) != want:
                raise ValueError(f"ResidentMolecules: bits [n, N, ceil((m_dim - atom_dim) / 32)] = {want}, got {tuple(bits.shape)}")
        self.device = atoms.device
        self._captured_bad = torch.zeros(1, dtype=torch.int32, device=self.device)     # counter of calls captured in a graph
        self._captured = False
        self._pending = []        # (pinned host counter, event behind its copy) per call whose counter is not read yet
        self._free_slots = []     # pinned int32 views not in use: one slot per PENDING call, handed back when it is read

    # ---- host side: the compact form ---------------------------------------------------------------------------------
    @staticmethod
    def pack(graphs, m_dim=None, b_dim=None):
        """numpy ``(atoms uint8 [n, N], ptr int64 [n + 1], entries uint32 [nnz])`` of a sequence of per-molecule objects with
        ``x [N, M]``, ``edge_index [2, nnz]``, ``edge_attr [nnz]`` (``smiles.MolGraph``, PyG ``Data``; numpy arrays or CPU
        tensors).  Duplicate ``(row, col)`` pairs are summed, as ``to_dense_adj``'s scatter-add does, and sums of zero are
        dropped; the entries of a molecule are in row-major order.  ``m_dim`` / ``b_dim`` default to the width of ``x`` and
        to the largest summed label + 1.  ``ValueError`` (naming the molecule) for a node matrix that is not exactly one-hot
        per row, a summed label outside ``[0, b_dim)``, a node id outside ``[0, N)``, graphs of different ``N``, and for
        ``N > 256``, ``b_dim > 16`` or ``m_dim > 255``."""
        return _pack(graphs, m_dim, b_dim)[:3]

    @staticmethod
    def pack_features(graphs, atom_dim, m_dim=None, b_dim=None):
        """``pack`` for node matrices ``x [N, m_dim]`` that are a one-hot atom type in the first ``atom_dim`` columns followed
        by ``F = m_dim - atom_dim`` feature columns of exactly 0 or 1 (the reference's ``--features``): numpy ``(atoms, ptr,
        entries, bits)``, the first three as ``pack`` gives them for the graphs cut to their first ``atom_dim`` columns, and
        ``bits`` uint32 ``[n, N, ceil(F / 32)]`` with feature ``f`` of an atom position in bit ``f % 32`` of word ``f // 32``
        (unused high bits zero).  ``ValueError`` (naming the molecule) for a prefix that is not one-hot per row, a feature
        value other than 0 or 1, ``atom_dim`` outside ``[1, m_dim]``, a graph of another width, and all of ``pack``'s."""
        atoms, ptr, entries, _, _, bits = _pack(graphs, m_dim, b_dim, atom_dim=atom_dim)
        return atoms, ptr, entries, bits

    @staticmethod
    def split_batch(data, batch_size: int):
        """The per-molecule graphs of a whole-dataset PyG-style batch (``x [B N, M]``, ``edge_index``, ``edge_attr``,
        ``batch``; host side): an edge belongs to graph ``src // N`` at ``(src % N, dst % N)`` -- an edge whose endpoints lie
        in different graphs lands in the SOURCE graph at column ``dst mod N``, as ``data.dense_one_hot_adjacency`` documents."""
        def host(t):
            return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        x, ei, attr = host(data.x), host(data.edge_index).astype(np.int64), host(data.edge_attr).reshape(-1)
        batch_size = int(batch_size)
        rows = int(host(data.batch).shape[0])
        if batch_size < 1 or rows % batch_size or x.shape[0] != rows:
            raise ValueError(f"a batch of {batch_size} padded graphs needs a multiple of {batch_size} node rows, got {rows}")
        N = rows // batch_size
        if ei.size and (ei.min() < 0 or ei.max() >= rows):
            bad = int(ei[0][(ei.min(0) < 0) | (ei.max(0) >= rows)][0])
            raise ValueError(f"molecule {min(max(bad // N, 0), batch_size - 1)}: node id outside [0, {rows}) in edge_index")
        owner = ei[0] // N
        order = np.argsort(owner, kind="stable")
        bounds = np.searchsorted(owner[order], np.arange(batch_size + 1))
        graphs = []
        for g in range(batch_size):
            sel = order[bounds[g]:bounds[g + 1]]
            graphs.append(SimpleNamespace(x=x[g * N:(g + 1) * N], edge_index=ei[:, sel] % N, edge_attr=attr[sel]))
        return graphs

    # ---- upload ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, atoms, ptr, entries, m_dim: int, b_dim: int, device=None, bits=None, atom_dim=None):
        """Upload the three arrays of ``pack`` (once), or the four of ``pack_features`` with its ``atom_dim``; a plane without
        a column (``atom_dim == m_dim``) is not kept."""
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError(f"druggen_amd.resident keeps the molecule set on the GPU (no CPU fallback); got device {device}")
        entries = np.ascontiguousarray(entries, dtype=np.uint32)
        if entries.size == 0:
            entries = np.zeros(1, np.uint32)      # (a molecule set without a single bond: keep the pointer non-null)
        if bits is not None:
            bits = np.ascontiguousarray(bits, dtype=np.uint32)
            if bits.ndim == 3 and bits.shape[2] == 0:      # F = 0: today's store
                bits = None
            else:
                bits = torch.from_numpy(bits.view(np.int32)).to(device)
        return cls(torch.from_numpy(np.ascontiguousarray(atoms, dtype=np.uint8)).to(device),
                   torch.from_numpy(np.ascontiguousarray(ptr, dtype=np.int64)).to(device),
                   torch.from_numpy(entries.view(np.int32)).to(device), m_dim, b_dim, bits, atom_dim)

    @classmethod
    def from_graphs(cls, graphs, device=None, m_dim=None, b_dim=None, atom_dim=None):
        """``pack`` + one upload.  ``m_dim`` / ``b_dim``: see ``pack``.  ``atom_dim``: ``pack_features`` instead."""
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError(f"druggen_amd.resident keeps the molecule set on the GPU (no CPU fallback); got device {device}")
        atoms, ptr, entries, m_dim, b_dim, bits = _pack(graphs, m_dim, b_dim, atom_dim=atom_dim)
        return cls.from_arrays(atoms, ptr, entries, m_dim, b_dim, device, bits=bits, atom_dim=atom_dim)

    @classmethod
    def from_batch(cls, data, batch_size: int, device=None, m_dim=None, b_dim=None, atom_dim=None):
        """A whole-dataset PyG-style batch (``x``, ``edge_index``, ``edge_attr``, ``batch``) split by ``split_batch``."""
        if device is None and torch.is_tensor(data.x) and data.x.is_cuda:
            device = data.x.device
        return cls.from_graphs(cls.split_batch(data, batch_size), device=device, m_dim=m_dim, b_dim=b_dim, atom_dim=atom_dim)

    def __len__(self):
        return self.n

    def nbytes(self) -> int:
        """Device bytes of the store."""
        return sum(t.numel() * t.element_size() for t in (self.atoms, self.ptr, self.entries, self.bits) if t is not None)

    # ---- batches -----------------------------------------------------------------------------------------------------
    def epoch(self, batch_size: int, *, shuffle: bool = True, drop_last: bool = True, generator=None):
        """Iterator of int64 GPU index tensors ``[batch_size]`` over ``torch.randperm(n)`` made on the device
        (``shuffle=False``: ``arange``); ``shuffle=True, drop_last=True`` are the settings of the reference's loaders."""
        if shuffle:
            order = torch.randperm(self.n, device=self.device, generator=generator)
        else:
            order = torch.arange(self.n, device=self.device)
        return epoch_batches(order, batch_size, drop_last)

    def _index(self, index):
        if not torch.is_tensor(index):
            index = torch.as_tensor(index, dtype=torch.int64)
        if index.dim() != 1:
            raise ValueError(f"index must be 1-D, got shape {tuple(index.shape)}")
        if index.dtype != torch.int64:
            if index.is_floating_point() or index.dtype == torch.bool:
                raise ValueError(f"index must hold integers, got {index.dtype}")
            index = index.long()
        if index.device != self.device:
            index = index.to(self.device)
        return index if index.is_contiguous() else index.contiguous()

    def _check_out(self, out, B):
        try:
            a, labels, x = out
        except (TypeError, ValueError):
            raise ValueError("out must be the triple (a, labels, x)") from None
        N, M, E = self.vertexes, self.m_dim, self.b_dim
        for t, shape, dtype, name in ((a, (B, N, N, E), torch.float32, "a"), (labels, (B, N, N), torch.int32, "labels"),
                                      (x, (B, N, M), torch.float32, "x")):
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"out: {name} must be a contiguous {dtype} tensor {shape} on {self.device}, got {got}")
        return a, labels, x

    def batch(self, index, *, out=None):
        """``(real_graphs, a_tensor, x_tensor)`` of the molecules ``index`` (int64 ``[B]``, on the store's device; a CPU
        tensor or a list is uploaded; repeats allowed), with ``load_molecules``' shapes and values: ``a_tensor [B,N,N,b_dim]``
        one-hot float32 with its int32 labels attached, ``x_tensor [B,N,m_dim]``, ``real_graphs`` their concatenation per
        molecule.  ``out=(a, labels, x)`` writes into caller-owned buffers (every element is overwritten), re-attaches
        ``labels`` to ``a`` and returns ``real_graphs = None``.

        No device -> host read: an index outside ``[0, n)`` is clamped into range on the device and counted; the counter
        reaches pinned host memory on a side stream, and a LATER call (or ``raise_bad_indices``) raises for it.  Inside a
        graph capture the counter stays on the device (every replay rewrites it); ``raise_bad_indices(wait=True)`` reads it."""
        index = self._index(index)
        B, N, M, E = int(index.shape[0]), self.vertexes, self.m_dim, self.b_dim
        if out is None:
            a = torch.empty(B, N, N, E, dtype=torch.float32, device=self.device)
            labels = torch.empty(B, N, N, dtype=torch.int32, device=self.device)
            x = torch.empty(B, N, M, dtype=torch.float32, device=self.device)
        else:
            a, labels, x = self._check_out(out, B)
        if B:
            if self.n == 0:
                raise ValueError("ResidentMolecules.batch: the store is empty")
            capturing = torch.cuda.is_current_stream_capturing()
            if not capturing:
                self.raise_bad_indices()      # counters of earlier calls whose host copies are complete by now
            bad = self._captured_bad if capturing else torch.empty(1, dtype=torch.int32, device=self.device)
            if self.bits is None:
                _lib.launch("dg_mol_gather", a, self.atoms.data_ptr(), self.ptr.data_ptr(), self.entries.data_ptr(), self.n,
                            index.data_ptr(), B, N, M, E, a.data_ptr(), labels.data_ptr(), x.data_ptr(), bad.data_ptr())
            else:
                _lib.launch("dg_mol_gather_features", a, self.atoms.data_ptr(), self.ptr.data_ptr(), self.entries.data_ptr(),
                            self.bits.data_ptr(), self.n, index.data_ptr(), B, N, M, E, int(self.bits.shape[2]), self.atom_dim,
                            a.data_ptr(), labels.data_ptr(), x.data_ptr(), bad.data_ptr())
            if capturing:
                self._captured = True
            else:
                self._defer(bad)
        attach_one_hot_labels(a, labels)
        if out is not None:
            return None, a, x
        return torch.concat((x.reshape(B, N * M), a.reshape(B, N * N * E)), dim=-1), a, x      # (explicit widths: B may be 0)

    # ---- the deferred index check ------------------------------------------------------------------------------------
    def _slot(self):
        if not self._free_slots:
            chunk = torch.zeros(_SLOT_CHUNK, dtype=torch.int32, pin_memory=True)
            self._free_slots.extend(chunk[i:i + 1] for i in range(_SLOT_CHUNK))
        return self._free_slots.pop()

    def _defer(self, bad):
        """counter -> its own pinned slot, on a side stream that waits for the kernel: the compute stream sees one event record."""
        host = self._slot()
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        side = _side_stream(self.device)
        side.wait_event(done)
        with torch.cuda.stream(side):
            host.copy_(bad, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        bad.record_stream(side)
        self._pending.append((host, ev))

    def raise_bad_indices(self, wait: bool = False) -> None:
        """Raise ``RuntimeError`` for earlier ``batch`` calls that had an index outside ``[0, n)`` (those were clamped into
        range).  Only counters whose copies have FINISHED are looked at; ``wait=True`` waits for all of them and also reads
        the counter of calls captured in a graph (its last replay).  The compute stream is never touched without ``wait``."""
        keep, found = [], []
        for host, ev in self._pending:
            if wait:
                ev.synchronize()
            elif not ev.query():
                keep.append((host, ev))
                continue
            n_bad = int(host[0])      # a plain host read: the copy behind `ev` has completed
            self._free_slots.append(host)
            if n_bad:
                found.append(n_bad)
        self._pending[:] = keep
        if wait and self._captured:
            n_bad = int(self._captured_bad.item())
            if n_bad:
                found.append(n_bad)
        if found:
            more = f" (and {len(found) - 1} more such calls)" if len(found) > 1 else ""
            raise RuntimeError(f"{found[0]} bad indices in an EARLIER ResidentMolecules.batch call: outside [0, {self.n}){more} "
                               f"(they were clamped into range on the device)")


def _feature_words(F):
    return (F + 31) // 32


def _pack(graphs, m_dim, b_dim, atom_dim=None):
    """``ResidentMolecules.pack`` plus the ``m_dim`` and ``b_dim`` it settled on and, with ``atom_dim``, the feature plane of
    ``pack_features`` (else ``None``)."""
    graphs = list(graphs)
    if not graphs:
        raise ValueError("ResidentMolecules.pack: no molecules")
    N = None
    atoms, counts, words, planes = [], [], [], []
    top = 0
    for i, g in enumerate(graphs):
        x = _host_array(g.x, "x", i)
        if x.ndim != 2:
            raise ValueError(f"molecule {i}: x must be [N, M], got shape {x.shape}")
        if N is None:
            N = int(x.shape[0])
            m_dim = int(x.shape[1] if m_dim is None else m_dim)
            _check_limits(N, m_dim, 1 if b_dim is None else int(b_dim), who="molecule 0: ")
            if atom_dim is not None and not 1 <= int(atom_dim) <= m_dim:
                raise ValueError(f"molecule 0: atom_dim = {atom_dim} outside [1, m_dim = {m_dim}]")
            A = m_dim if atom_dim is None else int(atom_dim)
        if x.shape[0] != N:
            raise ValueError(f"molecule {i}: {x.shape[0]} atom positions, molecule 0 has {N} (every graph is padded to the same N)")
        if x.shape[1] != m_dim:
            raise ValueError(f"molecule {i}: x has {x.shape[1]} columns, m_dim is {m_dim}")
        if atom_dim is None:
            if not (((x == 0) | (x == 1)).all() and (x.sum(1) == 1).all()):
                raise ValueError(f"molecule {i}: x is not one-hot per row (the reference's --features node matrices, a "
                                 "one-hot atom type followed by 0 / 1 columns, are taken with atom_dim=: pack_features)")
        else:
            x, feats = x[:, :A], x[:, A:]
            if not (((x == 0) | (x == 1)).all() and (x.sum(1) == 1).all()):
                raise ValueError(f"molecule {i}: the first atom_dim = {A} columns of x are not one-hot per row")
            if not ((feats == 0) | (feats == 1)).all():
                raise ValueError(f"molecule {i}: a feature column of x (from column atom_dim = {A} up) holds a value other "
                                 "than 0 or 1")
            octets = np.zeros((N, 4 * _feature_words(m_dim - A)), dtype=np.uint8)      # bit f % 8 of octet f // 8, little end first
            octets[:, :(m_dim - A + 7) // 8] = np.packbits(feats != 0, axis=1, bitorder="little")
            planes.append(octets.view("<u4").astype(np.uint32))
        atoms.append(x.argmax(1).astype(np.uint8))
        ei = _integers(g.edge_index, "edge_index", i)
        attr = _integers(g.edge_attr, "edge_attr", i).reshape(-1)
        if ei.ndim != 2 or ei.shape[0] != 2 or ei.shape[1] != attr.shape[0]:
            raise ValueError(f"molecule {i}: edge_index must be [2, nnz] and edge_attr [nnz], got {ei.shape} and {attr.shape}")
        if ei.size and (ei.min() < 0 or ei.max() >= N):
            raise ValueError(f"molecule {i}: node id outside [0, {N}) in edge_index")
        dense = np.zeros((N, N), dtype=np.int64)
        np.add.at(dense, (ei[0], ei[1]), attr)
        row, col = np.nonzero(dense)
        lab = dense[row, col]
        limit = MAX_B_DIM if b_dim is None else int(b_dim)
        if lab.size and (lab.min() < 0 or lab.max() >= limit):
            worst = int(lab.max() if lab.max() >= limit else lab.min())
            raise ValueError(f"molecule {i}: summed bond label {worst} outside [0, {limit})"
                             + ("" if b_dim is not None else f" (b_dim <= {MAX_B_DIM})"))
        top = max(top, int(lab.max()) if lab.size else 0)
        words.append((row | (col << 8) | (lab << 16)).astype(np.uint32))
        counts.append(row.size)
    ptr = np.zeros(len(graphs) + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    return (np.stack(atoms), ptr, np.concatenate(words), m_dim, (top + 1 if b_dim is None else int(b_dim)),
            None if atom_dim is None else np.stack(planes))


def _check_limits(N, m_dim, b_dim, who=""):
    if N < 1 or N > MAX_VERTEXES:
        raise ValueError(f"{who}ResidentMolecules: N = {N} atom positions, supported 1..{MAX_VERTEXES}")
    if m_dim < 1 or m_dim > MAX_M_DIM:
        raise ValueError(f"{who}ResidentMolecules: m_dim = {m_dim}, supported 1..{MAX_M_DIM}")
    if b_dim < 1 or b_dim > MAX_B_DIM:
        raise ValueError(f"{who}ResidentMolecules: b_dim = {b_dim}, supported 1..{MAX_B_DIM}")
