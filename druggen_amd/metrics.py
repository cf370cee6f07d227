"""Fingerprint similarity on the GPU (reference ``src/util/utils.py:550-611``: ``average_agg_tanimoto`` and
``internal_diversity``, called for SNN and IntDiv by ``inference.py:261-263``, ``results/evaluate.py:45`` and the
training loop's ``logging()``).

Fingerprints are kept PACKED: ``[n, nbits / 32]`` 32-bit words, bit ``k`` of a fingerprint in bit ``k % 32`` of word
``k // 32`` (``np.packbits(..., bitorder='little')`` read as little-endian ``uint32``), plus the bit count of every row.
A ChEMBL-sized stock of 1.6 M 1024-bit fingerprints is 200 MB this way instead of 6 GB of float32.  ``dg_fp_tanimoto``
(csrc/fp_tanimoto.hip) computes for every generated row the maximum (and where it is attained) or the mean
of ``float32(c) / float32(a + b - c)`` over the stock -- the reference's float32 quotient, 0 / 0 taken as 1.

GPU only, no CPU fallback.  This module starts from bits: RDKit's Morgan fingerprints come from the host as dense rows
(``pack_fingerprints``); ``druggen_amd.fingerprint`` makes the project's own circular fingerprints of decoded molecules on the
device and hands them over as ``PackedFingerprints``."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .functional import _c

__all__ = ["PackedFingerprints", "pack_bits_numpy", "pack_fingerprints", "tanimoto_aggregate", "average_agg_tanimoto",
           "internal_diversity"]

MAX_NBITS = 4096
_MODES = {"max": 0, "mean": 1}      # DG_FP_MAX / DG_FP_MEAN of include/druggen_hip.h
_DENSE = {torch.uint8: 0, torch.bool: 0, torch.float32: 1}      # DG_FP_DENSE_U8 / DG_FP_DENSE_F32


def _check_nbits(nbits):
    if nbits < 32 or nbits > MAX_NBITS or nbits % 32:
        raise ValueError(f"fingerprints need a multiple of 32 bits between 32 and {MAX_NBITS}, got {nbits}")


@dataclass
class PackedFingerprints:
    """``words`` [n, nbits / 32] int32 (the bit patterns of the packed uint32 words), ``counts`` [n] int32, ``nbits``."""
    words: torch.Tensor
    counts: torch.Tensor
    nbits: int

    def __len__(self):
        return self.words.shape[0]


def pack_bits_numpy(x):
    """Dense ``[n, nbits]`` array (any element != 0 is a set bit) -> (``uint32`` words ``[n, nbits / 32]``, ``int32`` bit
    counts ``[n]``) on the host."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"fingerprints are a 2-D array [n, nbits], got shape {x.shape}")
    _check_nbits(x.shape[1])
    bits = x != 0
    words = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u4")
    return words.astype(np.uint32, copy=False), bits.sum(1, dtype=np.int64).astype(np.int32)


def _cuda_device(device):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"druggen_amd.metrics runs on the GPU (no CPU fallback); got device {device}")
    return device


def pack_fingerprints(x, device=None):
    """``PackedFingerprints`` on the GPU.  A numpy array is packed on the host (``np.packbits``) and uploaded packed -- the
    loader's route, 32 times fewer bytes than the dense floats; a GPU tensor (uint8, bool, float32; other dtypes through
    ``!= 0``) is packed there by ``dg_fp_pack``."""
    if isinstance(x, PackedFingerprints):
        return x
    if torch.is_tensor(x):
        if x.dim() != 2:
            raise ValueError(f"fingerprints are a 2-D tensor [n, nbits], got shape {tuple(x.shape)}")
        n, nbits = x.shape
        _check_nbits(nbits)
        if not x.is_cuda:
            raise RuntimeError("druggen_amd.metrics runs on the GPU (no CPU fallback): pass a GPU tensor, or a numpy array "
                               "to pack on the host and upload")
        x = x.detach()
        if x.dtype not in _DENSE:
            x = x != 0
        x = _c(x)
        words = torch.empty((n, nbits // 32), dtype=torch.int32, device=x.device)
        counts = torch.empty((n,), dtype=torch.int32, device=x.device)
        if n:
            _lib.launch("dg_fp_pack", x, x.data_ptr(), _DENSE[x.dtype], n, nbits, words.data_ptr(), counts.data_ptr())
        return PackedFingerprints(words, counts, nbits)
    words, counts = pack_bits_numpy(x)
    device = _cuda_device(device)
    return PackedFingerprints(torch.from_numpy(words.view(np.int32)).to(device), torch.from_numpy(counts).to(device),
                              int(np.asarray(x).shape[1]))


def _nbits_of(x):
    return x.nbits if isinstance(x, PackedFingerprints) else int(x.shape[-1])


def tanimoto_aggregate(stock, gen, agg="max", return_index=False):
    """For every row of ``gen`` the maximum (``agg='max'``) or the mean (``'mean'``) over the rows of ``stock`` of the
    Tanimoto similarity ``float32(c) / float32(a + b - c)`` (1 where both rows are empty): a float64 GPU tensor ``[G]``.
    ``return_index=True`` (max only) adds the int32 ``[G]`` stock index that attains the maximum, the smallest on ties.
    Inputs are ``PackedFingerprints`` or dense arrays / tensors, packed on the way.  The mean sums the float32 quotients in
    float64.  Results are bit-reproducible.  An empty stock gives the reference's values: 0 (index -1) for max, NaN for
    mean."""
    if agg not in _MODES:
        raise ValueError("Can aggregate only max or mean")
    if return_index and agg != "max":
        raise ValueError("return_index belongs to agg='max'")
    if _nbits_of(stock) != _nbits_of(gen):
        raise ValueError(f"stock has {_nbits_of(stock)}-bit fingerprints, gen {_nbits_of(gen)}-bit ones")
    gen = pack_fingerprints(gen)
    stock = pack_fingerprints(stock, device=gen.words.device)
    for t in (stock.words, stock.counts, gen.words, gen.counts):
        if not t.is_cuda:
            raise RuntimeError("druggen_amd.metrics runs on the GPU (no CPU fallback)")
        if t.device != gen.words.device or t.dtype != torch.int32:
            raise ValueError("PackedFingerprints hold int32 words and counts on one device")
    _check_nbits(gen.nbits)
    W = gen.nbits // 32
    if stock.nbits != gen.nbits or stock.words.shape[1:] != (W,) or gen.words.shape[1:] != (W,):
        raise ValueError("packed words do not match nbits")
    S, G = len(stock), len(gen)
    if stock.counts.shape != (S,) or gen.counts.shape != (G,):
        raise ValueError("one bit count per fingerprint")
    dev = gen.words.device
    mean = agg == "mean"
    if S == 0 or G == 0:
        out = torch.full((G,), float("nan") if mean else 0.0, dtype=torch.float64, device=dev)
        return (out, torch.full((G,), -1, dtype=torch.int32, device=dev)) if return_index else out
    sw, sc, gw, gc = _c(stock.words), _c(stock.counts), _c(gen.words), _c(gen.counts)
    lib = _lib.load()
    need = int(lib.dg_fp_tanimoto_workspace_bytes(S, G))
    work = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    out = torch.empty((G,), dtype=torch.float64 if mean else torch.float32, device=dev)
    idx = torch.empty((G,), dtype=torch.int32, device=dev) if return_index else None
    _lib.launch("dg_fp_tanimoto", gw, sw.data_ptr(), sc.data_ptr(), S, gw.data_ptr(), gc.data_ptr(), G, gen.nbits,
                _MODES[agg], out.data_ptr(), None if idx is None else idx.data_ptr(),
                None if work is None else work.data_ptr(), need)
    out = out if mean else out.double()      # float32 -> float64 is exact
    return (out, idx) if return_index else out


def average_agg_tanimoto(stock_vecs, gen_vecs, batch_size=5000, agg="max", device=None, p=1, intdiv=False):
    """The reference's ``average_agg_tanimoto`` (utils.py:566-611) on the GPU: ``float`` (the mean over the generated
    rows), or with ``intdiv=True`` the per-row float64 ``np.ndarray``.  ``batch_size`` is accepted and ignored (the kernel
    never materialises a block of similarities).  ``p != 1`` raises ``ValueError``: no caller in the reference passes it.
    ``device``: the GPU to upload numpy inputs to (None: the current one); a CPU device is an error."""
    if agg not in _MODES:
        raise ValueError("Can aggregate only max or mean")
    if p != 1:
        raise ValueError("average_agg_tanimoto: only p = 1 is implemented (no caller of the reference uses another p)")
    if _nbits_of(stock_vecs) != _nbits_of(gen_vecs):
        raise ValueError(f"stock has {_nbits_of(stock_vecs)}-bit fingerprints, gen {_nbits_of(gen_vecs)}-bit ones")
    gen = pack_fingerprints(gen_vecs, device)
    stock = pack_fingerprints(stock_vecs, gen.words.device)
    per_row = tanimoto_aggregate(stock, gen, agg).cpu().numpy()
    return per_row if intdiv else np.mean(per_row)


def internal_diversity(gen):
    """(mean, std) over the rows of ``1 - mean similarity to all rows`` (diagonal included), as the reference's
    ``internal_diversity`` (utils.py:550-563)."""
    gen = pack_fingerprints(gen)
    diversity = 1 - average_agg_tanimoto(gen, gen, agg="mean", intdiv=True)
    return np.mean(diversity), np.std(diversity)
