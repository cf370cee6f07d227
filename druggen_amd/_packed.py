"""What the records of the molecule pipeline share (``decode.MoleculeBatch``, ``monitor.MolStats``, ``canon.CanonicalForms``,
``canon.FormMatches``): typed views of ONE packed byte buffer, on the device (``torch``) or on the host (``numpy``), so that a
record travels with one device->host copy; and the small argument helpers of the modules that fill them."""
from __future__ import annotations

import copy

import numpy as np
import torch

_TORCH_TYPES = {1: torch.uint8, 2: torch.uint16, 4: torch.int32, 8: torch.int64}
_NUMPY_TYPES = {1: np.uint8, 2: np.uint16, 4: np.int32, 8: np.int64}


def layout(fields, pad_end=True):
    """``fields``: ``(name, element bytes, shape)`` in buffer order -> name -> (byte offset, bytes, element bytes, shape), and
    the buffer's size.  Every field starts on a 16-byte boundary; the size is at least 16 bytes, and a multiple of 16 unless
    ``pad_end`` is off."""
    table, off, end = {}, 0, 0
    for name, item, shape in fields:
        nbytes = item * int(np.prod(shape, dtype=np.int64))
        table[name] = (off, nbytes, item, shape)
        end = off + nbytes
        off = (end + 15) & ~15
    return table, max(off if pad_end else end, 16)


class PackedRecord:
    """A class names its fields in ``_fields(*args)``, ``args`` being what its constructor takes after the buffer; every field
    becomes an attribute.  ``TOT_FIELDS`` names the entries of a ``tot`` field for ``total``."""

    _PAD_END = True
    TOT_FIELDS = ()

    def __init__(self, buffer, *geometry):
        table, total = self.layout(*geometry)
        assert buffer.shape[0] == total
        self.buffer = buffer
        self.is_host = isinstance(buffer, np.ndarray)
        for name, (off, nbytes, item, shape) in table.items():
            part = buffer[off:off + nbytes]
            view = part.view(_NUMPY_TYPES[item]).reshape(shape) if self.is_host else part.view(_TORCH_TYPES[item]).view(shape)
            setattr(self, name, view)
        self._geometry = geometry

    @classmethod
    def layout(cls, *geometry):
        return layout(cls._fields(*geometry), cls._PAD_END)

    @classmethod
    def _empty(cls, device, *geometry):
        """A device record over an uninitialised buffer."""
        return cls(torch.empty(cls.layout(*geometry)[1], dtype=torch.uint8, device=device), *geometry)

    def cpu(self):
        """The record on the host: ONE transfer of the packed buffer for all its fields."""
        if self.is_host:
            return self
        host = copy.copy(self)
        PackedRecord.__init__(host, self.buffer.cpu().numpy(), *self._geometry)
        return host

    def _host(self, what):
        if not self.is_host:
            raise RuntimeError(f"{type(self).__name__}.{what} reads the host copy: call .cpu() once for the batch first")

    def total(self, name):
        """Entry ``name`` of ``tot`` (``TOT_FIELDS``) as a Python int; host copy only."""
        if not self.is_host:
            raise RuntimeError(f"{type(self).__name__} totals and fractions read the host copy: call .cpu() once first")
        return int(self.tot[self.TOT_FIELDS.index(name)])


_uploads = {}


def uploaded(values, dtype, device):
    """The tuple ``values`` as a 1-d device tensor of the numpy ``dtype``; a host sequence is uploaded once per device, not at
    every call."""
    key = (values, np.dtype(dtype), device)
    t = _uploads.get(key)
    if t is None:
        if len(_uploads) > 64:
            _uploads.clear()
        t = _uploads[key] = torch.from_numpy(np.asarray(values, dtype=dtype)).to(device)
    return t


def check_key_bits(key_bits):
    if not isinstance(key_bits, int) or isinstance(key_bits, bool) or not 1 <= key_bits <= 64:
        raise ValueError(f"key_bits must be an integer in 1..64, got {key_bits!r}")
