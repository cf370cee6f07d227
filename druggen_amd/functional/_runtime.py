"""State every autograd node family shares: per-kernel traffic accounting for bench.py, the storage modes of the feed-forward's
hidden tensors, scratch workspaces, the activation dtype, the pass flags (inputs-only backward, second-order forward) and the
thread-local scopes of the C library (reduce batches, riding launches)."""
from __future__ import annotations

import contextlib
import threading
import weakref

import torch

from .. import _lib
from ..options import options


# Algorithmic HBM bytes per kernel, accumulated per launch so that
# bench.py can turn the HIP-event times of dg_prof_* into achieved GB/s.
_traffic = {}


def traffic_reset() -> None:
    _traffic.clear()


def traffic_bytes(kernel: str) -> int:
    return _traffic.get(kernel, 0)


def _account(kernel: str, nbytes: int, flops: int = 0, floor: int = -1) -> None:
    """``nbytes``: what the launch must move given what it is asked to produce (inputs + outputs + tensors it saves for a
    backward).  ``floor``: inputs + outputs only (nothing saved, a backward recomputes) -- defaults to
    ``nbytes`` for launches that save nothing."""
    _traffic[kernel] = _traffic.get(kernel, 0) + nbytes
    _traffic[kernel + ":floor"] = _traffic.get(kernel + ":floor", 0) + (nbytes if floor < 0 else floor)
    if flops:
        _traffic[kernel + ":flops"] = _traffic.get(kernel + ":flops", 0) + flops


def traffic_floor_bytes(kernel: str) -> int:
    return _traffic.get(kernel + ":floor", 0)


def _gemm_key(R: int, K: int, N: int) -> str:
    """Profiler / traffic key of a row GEMM launch: edge-level launches by shape (DG_K_ROW_GEMM_E_*), the rest together."""
    if R < _lib.edge_rows():
        return "row_gemm"
    return "row_gemm_e_k384" if K == 384 else ("row_gemm_e_n384" if N == 384 else "row_gemm_e128")


def _wgrad_key(R: int, N: int, K: int) -> str:
    """Profiler / traffic key of a weight-gradient launch (DG_K_LINEAR_WGRAD_E_*: edge-level launches by shape of dW)."""
    if R >= _lib.edge_rows():
        if (N, K) == (128, 128):
            return "linear_wgrad_e128"
        if (N, K) == (384, 128):
            return "linear_wgrad_e_n384"
        if (N, K) == (128, 384):
            return "linear_wgrad_e_k384"
    return "linear_wgrad"


def traffic_flops(kernel: str) -> int:
    return _traffic.get(kernel + ":flops", 0)


_dev = _lib._dev      # (lives next to ``_lib.launch``, which needs it)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# --------------------------------------------------------------------------
# storage of the [R,384] hidden tensors of the float32 feed-forward (DG_DTYPE_F32_H16, include/druggen_hip.h)
# --------------------------------------------------------------------------
_HIDDEN_MODES = ("f32", "dh16", "dh24", "f24", "f16")


def hidden_storage() -> str:
    """Storage of the [R,384] hidden tensors of the float32 feed-forward (``options.hidden``, DG_HIDDEN at import):
      "f32"   plain float32;
      "dh16"  (default) the BACKWARD's hidden tensors -- dh = (dz W2) * m and its second-order twin -- as ONE fp16 plane per row
              under an exact power-of-two row scale (DG_DTYPE_F32_H16); the forward's h = relu(fc1 x) stays float32 class: on chip
              in the fused forward (dg_ffn_ln_fwd_f32), pre-split hi + lo planes in the two-launch forward (DG_DTYPE_F32_H32);
      "dh24"  the backward's tensors as the top 24 bits of every float32 (DG_DTYPE_F32_H24), h float32;
      "f24" / "f16"   h as well.  Rounding h perturbs the forward pass, and a perturbed forward flips ReLU masks in the layers
              behind it: gradient errors of the order of the SQUARE ROOT of the perturbation on small batches (two-molecule
              goldens: 1.4e-3 - 4e-3 with f24's 2^-17, up to 1.5e-2 with f16's 2^-11) -- outside the 1e-3 parity bar, labelled
              modes like the bf16 configuration.  dh only travels through linear maps: its rounding stays a rounding."""
    return options.hidden


def set_hidden_storage(mode: str) -> None:
    """``options.hidden = mode`` (one of f32, dh16, dh24, f24, f16)."""
    options.hidden = mode


# Above this many atoms the default mode keeps the backward's hidden tensors in 24 bits (the "dh24" pairing) instead of the fp16
# plane: a node's gradient sums N edge rows' fp16 roundings while their signal cancels (softmax), so the spend grows with N --
# worst golden tensor 6.4e-4 at N = 128 with dh16 (tests/test_hip_model.py::test_parity_margin_tripwire allows 6e-4), 3.8e-5
# with dh24.
DH16_MAX_ATOMS = 96


def _long_rows(x) -> bool:
    """``x`` ([B,N,C] node or [B,N,N,C] edge rows) belongs to molecules of more than DH16_MAX_ATOMS atoms."""
    return x.dim() >= 3 and x.shape[-2] > DH16_MAX_ATOMS


def hidden_forward_storage(long_rows: bool = False) -> str:
    """Storage of the FORWARD's h = relu(fc1 x) when it goes through HBM in the default mode: "split" -- the float32-class
    hi / lo fp16 split under one row scale, done once by the launch that writes h (DG_DTYPE_F32_H32: fc2's launch only moves the
    planes, the weight gradient dW2 = dz^T h reads the hi plane alone) -- or "f32" (every other mode, and molecules of more than
    DH16_MAX_ATOMS atoms, whose backward then stores dh in 24 bits: ``_ffn_bwd_codes``)."""
    return "split" if hidden_storage() == "dh16" and not long_rows else "f32"


def _hidden_code(adt, long_rows: bool = False) -> int:
    """ABI dtype code of the FORWARD's hidden tensor h for activations of ``adt``."""
    if adt == torch.float32:
        mode = hidden_storage()
        if mode in ("f16", "f24"):
            return _lib.F32_H16 if mode == "f16" else _lib.F32_H24
        if hidden_forward_storage(long_rows) == "split":
            return _lib.F32_H32
    return _lib.DTYPES[adt]


def _hidden_code_bwd(adt) -> int:
    """ABI dtype code of the BACKWARD's hidden tensors (dh, and (t W1^T) * m of the second order)."""
    if adt == torch.float32:
        mode = hidden_storage()
        if mode in ("f16", "dh16"):
            return _lib.F32_H16
        if mode in ("f24", "dh24"):
            return _lib.F32_H24
    return _lib.DTYPES[adt]


def _ffn_bwd_codes(h, adt, R: int, H: int):
    """(dtype code of the dg_edge_ffn_ln_bwd call, storage code of dh): h's storage is what the forward chose, dh's what
    ``_hidden_code_bwd`` says now -- equal, or (h float32, dh narrow) the DG_DTYPE_F32_DH16 / _DH24 pairs."""
    if _is_h16(h):
        code = _hidden_code_of(h, R, H)
        if code == _lib.F32_H32:      # (h pre-split: dh is the fp16 plane of the default mode)
            return _lib.F32_H32_DH16, _lib.F32_H16
        return code, code
    dh_code = _hidden_code_bwd(adt)
    if dh_code == _lib.F32_H16 and hidden_storage() == "dh16":
        # float32 h in the default mode: the forward took molecules of more than DH16_MAX_ATOMS atoms -- dh in 24 bits
        dh_code = _lib.F32_H24
    if dh_code == _lib.F32_H16:
        return _lib.F32_DH16, dh_code
    if dh_code == _lib.F32_H24:
        return _lib.F32_DH24, dh_code
    return _lib.DTYPES[adt], _lib.DTYPES[adt]


def _hidden_empty(R: int, H: int, adt, code: int, device):
    """An uninitialised [R,H] hidden tensor: float32 / bfloat16 [R,H], or (DG_DTYPE_F32_H16) the opaque byte buffer
    [R][H] fp16 + [R] float32 inverse row scales that only the kernels read."""
    if code in _lib.HIDDEN_CODES:
        return torch.empty(int(_lib.load().dg_hidden_bytes(R, H, code)), dtype=torch.uint8, device=device)
    return torch.empty(R, H, dtype=adt, device=device)


def _hrow_bytes(code: int, es: int, H: int) -> int:
    """Bytes per row of a hidden tensor (traffic accounting)."""
    if code == _lib.F32_H32:
        return 4 * H + 4
    return 2 * H + 4 if code == _lib.F32_H16 else (3 * H if code == _lib.F32_H24 else es * H)


def _is_h16(t) -> bool:
    return t is not None and t.dtype == torch.uint8


def _hptr(t):
    """Device pointer of a hidden tensor (either storage)."""
    return t.data_ptr() if _is_h16(t) else _lib.ptr(t)


def _hidden_code_of(buf, R: int, H: int = 384) -> int:
    """The ABI dtype code of a hidden buffer made by ``_hidden_empty`` (its size tells the storage)."""
    if buf.numel() == R * H * 3:
        return _lib.F32_H24
    plane = (R * H * 2 + 255) // 256 * 256
    return _lib.F32_H32 if buf.numel() == 2 * plane + 4 * R else _lib.F32_H16


def hidden_to_float(buf, R: int, H: int = 384):
    """Decode a DG_DTYPE_F32_H16 / _H24 buffer into a float32 [R,H] tensor (tests, probes)."""
    if _hidden_code_of(buf, R, H) == _lib.F32_H24:
        b = buf.view(R * H, 3).to(torch.int32)
        bits = (b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)
        return bits.view(torch.float32).view(R, H)
    off = int(_lib.load().dg_hidden_scale_offset(R, H))
    half = buf[:R * H * 2].view(torch.float16).view(R, H).float()
    if _hidden_code_of(buf, R, H) == _lib.F32_H32:      # hi plane | lo plane | scales
        half = half + buf[off:off + R * H * 2].view(torch.float16).view(R, H).float()
        off *= 2
    scale = buf[off:off + 4 * R].view(torch.float32)
    return half * scale[:, None]


_ws_cache = {}
_cache_lock = threading.Lock()      # nn.DataParallel replica threads insert into / sweep the module-level caches concurrently


def _scratch(ref, need, tag="ln"):
    """Per (device, stream, thread, tag) scratch buffer owned by the caller side (PyTorch).  The thread is part of the key
    because nn.DataParallel replicas are threads: two of them on ONE device and stream (device_ids=[0, 0]) would
    otherwise interleave a kernel of one call with the reduction of another over the same workspace."""
    key = (ref.device, _lib.stream_of(ref), threading.get_ident(), tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=ref.device)
        with _cache_lock:
            if len(_ws_cache) > 256:      # nn.DataParallel starts fresh replica threads per forward: drop dead threads' buffers
                alive = {t.ident for t in threading.enumerate()}
                for k in [k for k in list(_ws_cache) if k[2] not in alive]:
                    _ws_cache.pop(k, None)
            _ws_cache[key] = buf
    return buf


def _workspace(ref, R, C):
    need = int(_lib.load().dg_ln_workspace_bytes(R, C))
    return _scratch(ref, need, "ln"), need


_ACT_DTYPES = {"f32": torch.float32, "fp32": torch.float32, "float32": torch.float32,
               "bf16": torch.bfloat16, "bfloat16": torch.bfloat16}


def _as_act_dtype(dtype):
    dtype = _ACT_DTYPES.get(dtype, dtype) if isinstance(dtype, str) else dtype
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"activation dtype must be torch.float32 or torch.bfloat16, got {dtype!r}")
    return dtype


def set_activation_dtype(dtype) -> None:
    """Storage type of the encoder activations produced by Generator / Discriminator from now on:
    ``torch.float32`` (BASELINE configs[1], default) or ``torch.bfloat16`` (configs[2]: every
    [B,N,N,C] / [B,N,C] activation and activation gradient lives in HBM as bf16, one bf16 MFMA per
    product, fp32 accumulation, fp32 softmax / LayerNorm statistics, fp32 parameters, optimizer
    state and weight gradients).  Model inputs and outputs (one-hot graphs, logits) stay float32."""
    _flags.act_dtype = _as_act_dtype(dtype)


def activation_dtype():
    return _flags.act_dtype


@contextlib.contextmanager
def activations(dtype):
    """``with activations(torch.bfloat16): ...`` -- scoped form of ``set_activation_dtype``."""
    prev = _flags.act_dtype
    _flags.act_dtype = _as_act_dtype(dtype)
    try:
        yield
    finally:
        _flags.act_dtype = prev


class _Flags:
    """Process-wide (NOT thread-local) pass flags.  A backward node of a CUDA tensor runs on the
    autograd engine's device thread, and nn.DataParallel runs every replica forward on its own thread:
    neither sees a ``threading.local`` set by the thread that entered the context manager (round-1
    bug: the gradient penalty's first-order pass still computed every weight gradient).  The contexts
    are entered by the CALLER of the model (``gradient_penalty``), never by a replica: the caller blocks
    until every replica thread / engine thread has finished, so all of them see one consistent value
    (``tests/test_hip_scale.py::test_dataparallel_replicas_on_one_device...`` runs two replica threads
    through the gradient penalty).  Two independent training loops in ONE process would race them."""
    inputs_only = 0
    second_order = 0
    act_dtype = torch.float32


_flags = _Flags()


def _inputs_only() -> bool:
    return _flags.inputs_only > 0


@contextlib.contextmanager
def inputs_only_backward():
    """Inside this context a backward pass skips parameter gradients of the
    custom ops.  Used around the gradient penalty's first-order
    ``autograd.grad(..., inputs=[int_node, int_edge])`` (loss.py:32-39), where
    PyTorch's built-in ops skip them too but custom Functions cannot tell."""
    _flags.inputs_only += 1
    try:
        yield
    finally:
        _flags.inputs_only -= 1


@contextlib.contextmanager
def _reduce_batch(ref, on=True):
    """dg_linear_wgrad_batch_begin / _end around a block's backward: the fixed-order reductions of its weight gradients
    (``_wgrad_many(..., open_batch=False)``) and of its LayerNorms' dgamma / dbeta (``_ln_bwd_rows(batch_slot=i)``) run
    as ONE launch at the end (at most 8 of them; further ones reduce at once)."""
    if not (on and ref.is_cuda):
        yield False
        return
    with _dev(ref):
        _lib.check(_lib.load().dg_linear_wgrad_batch_begin(), "dg_linear_wgrad_batch_begin")
        try:
            yield True
        finally:
            _lib.launch("dg_linear_wgrad_batch_end", ref)


_pair_tls = threading.local()


def _pair_hold(*tensors) -> None:
    """Lifetime contract of riding launches (csrc/pair.h keeps RAW device pointers of a waiting launch until its carrier or
    dg_launch_pair_end): every operand of a launch issued inside ``_pair_launches`` is referenced from here until the
    region ends, so a temporary (a ``.contiguous()`` / ``.to()`` copy) cannot go back to the caching allocator -- and be
    handed to a kernel that is launched EARLIER in stream order -- while a rider still points at it."""
    keep = getattr(_pair_tls, "keep", None)
    if keep is not None:
        keep.extend(t for t in tensors if t is not None)


@contextlib.contextmanager
def _pair_launches(ref, on=True):
    """dg_launch_pair_begin / _end: node-level launches of the 384-wide row GEMMs and of the producer / consumer weight
    gradients issued inside wait for -- and ride in -- the next launch of the same kernel (include/druggen_hip.h).  The
    caller issues node, edge, node, edge ... and reads no waiting result before its carrier was called."""
    if not (on and ref.is_cuda):
        yield False
        return
    outer = getattr(_pair_tls, "keep", None)
    if outer is None:
        _pair_tls.keep = []
    with _dev(ref):
        _lib.check(_lib.load().dg_launch_pair_begin(), "dg_launch_pair_begin")
        try:
            yield True
        finally:
            try:      # (also on an exception path: whatever waits is launched before its operands can be freed)
                _lib.launch("dg_launch_pair_end", ref)
            finally:
                if outer is None:
                    _pair_tls.keep = None


@contextlib.contextmanager
def second_order_forward():
    """Forward passes run inside this context will be differentiated twice
    (gradient penalty, loss.py:28-39): modules then build their graph from the
    twice-differentiable ops (linear / ln_residual / attn_core) instead of the
    fused first-order ones, which would have to recompute."""
    _flags.second_order += 1
    try:
        yield
    finally:
        _flags.second_order -= 1


def in_second_order_forward() -> bool:
    return _flags.second_order > 0


def _alias_outputs_enabled() -> bool:
    return options.penalty_wgrad == "joined"


# --------------------------------------------------------------------------
# packed weights: kernels that read a weight in MFMA fragment order keep a packed copy per parameter
# --------------------------------------------------------------------------
_alias_canon = {}      # data pointer -> weakref of the parameter an alias output stands for


def _weight_alias(t):
    """A view of parameter ``t`` that a forward node returns as an extra output and hands to its differentiable backward
    node in place of ``t`` (second-order forward of the gradient penalty): the second-order gradient of the parameter
    then comes back to the forward node as the gradient of that output and joins the node's own parameter gradient in
    one multi-tensor add -- otherwise the autograd engine sums the two contributions of every parameter with a launch
    each (~50 tiny adds per step)."""
    a = t.view_as(t)
    with _cache_lock:
        if len(_alias_canon) > 4096:
            for k in [k for k, r in list(_alias_canon.items()) if r() is None]:
                _alias_canon.pop(k, None)
        _alias_canon[a.data_ptr()] = weakref.ref(t)
    return a


def _canon(w):
    """The parameter behind an alias made by ``_weight_alias`` (same storage, shape, version), else ``w``: the pack
    caches are keyed by the parameter object."""
    r = _alias_canon.get(w.data_ptr())
    o = r() if r is not None else None
    if (o is not None and o is not w and o.data_ptr() == w.data_ptr() and o.shape == w.shape and o.stride() == w.stride()
            and o._version == w._version and o.dtype == w.dtype):
        return o
    return w


_weights_epoch = [0]                # bumped by writers that change parameters without touching ``tensor._version``
_pack_caches = weakref.WeakSet()    # every PackCache alive: ``bump_weights_epoch`` sweeps them all
_EPOCH_SWEEP_ABOVE = 8192           # entries over all caches above which a bump sweeps


class _PackEntry:
    __slots__ = ("refs", "versions", "ptrs", "epoch", "extra", "packed")

    def stamp(self, weights) -> None:
        self.versions = tuple(w._version for w in weights)
        self.ptrs = tuple(w.data_ptr() for w in weights)
        self.epoch = _weights_epoch[0]


class PackCache:
    """Packed copies of one kernel family's weights, keyed by ``(*ids of the weights, *extra)``.  An entry is fresh while
    every weight is still the same object with the same ``_version`` and ``data_ptr()`` and the weights epoch has not moved;
    anything else re-makes it.  Touches nothing device-specific: allocation and the pack launch are the caller's ``make``."""

    def __init__(self, limit: int):
        self.limit = limit      # entries above which a miss first drops those of dead weights (e.g. DataParallel replicas)
        self._entries = {}
        _pack_caches.add(self)

    def __len__(self) -> int:
        return len(self._entries)

    def get(self, weights, extra, make):
        """The pack of the tuple ``weights`` under the hashable tuple ``extra`` (mode, dtype, ...); ``make(*weights)``
        builds it on a miss.  Aliases made by ``_weight_alias`` share their parameter's entry."""
        weights = tuple(map(_canon, weights))
        key = (*map(id, weights), *extra)
        e = self._entries.get(key)
        if e is not None and e.epoch == _weights_epoch[0]:
            for r, v, p, w in zip(e.refs, e.versions, e.ptrs, weights):
                if r() is not w or v != w._version or p != w.data_ptr():
                    break
            else:
                return e.packed
        if len(self._entries) > self.limit:
            self.sweep()
        e = _PackEntry()
        e.refs, e.extra = tuple(weakref.ref(w) for w in weights), extra
        e.stamp(weights)      # (before make: a writer racing the pack launch leaves the entry stale, not wrongly fresh)
        e.packed = make(*weights)
        self._entries[key] = e
        return e.packed

    def entries(self):
        """[(key, weights, extra, packed, ptrs)] of the entries whose weights are all alive -- a snapshot; ``ptrs``: the
        weights' addresses when the entry was made or last restamped."""
        out = []
        for key, e in list(self._entries.items()):
            weights = tuple(r() for r in e.refs)
            if all(w is not None for w in weights):
                out.append((key, weights, e.extra, e.packed, e.ptrs))
        return out

    def restamp(self, key) -> None:
        """``key``'s pack was refreshed in place from the weights as they are now: the entry is fresh again."""
        e = self._entries.get(key)
        weights = () if e is None else tuple(r() for r in e.refs)
        if e is not None and all(w is not None for w in weights):
            e.stamp(weights)

    def pop(self, key):
        e = self._entries.pop(key, None)
        return None if e is None else e.packed

    def sweep(self) -> None:
        """Drop the entries of which a weight is dead."""
        with _cache_lock:
            for k in [k for k, e in list(self._entries.items()) if any(r() is None for r in e.refs)]:
                self._entries.pop(k, None)


def bump_weights_epoch() -> None:
    """Invalidate every packed weight (every PackCache compares this epoch).  Called by writers that change
    parameters behind autograd's back: ``FlatAdamW.step`` (raw kernel on the flat buffer) and
    ``GraphedGANStep`` (before capture, so that the first use after each optimizer step records its
    pack kernel into the graph, and after every replay, which updates weights without touching
    ``tensor._version``)."""
    _weights_epoch[0] += 1
    caches = list(_pack_caches)
    if sum(len(c) for c in caches) > _EPOCH_SWEEP_ABOVE:
        for c in caches:
            c.sweep()
