"""Graph attention (reference src/model/layers.py:97-137,185-190): the attention core with its two backward orders and the whole
attention half of an Encoder_Block as one autograd node (float32: dg_attn_half_f32_*; bf16: dg_attn_half_*)."""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from ..options import options
from ._runtime import (_account, _alias_outputs_enabled, _c, in_second_order_forward, _inputs_only, PackCache, _reduce_batch,
                       _scratch, _weight_alias)
from .dense import (_double_backward_fallback, _join_alias_grads, lin3, lin3_supported, linear, linear_ln, _ln_bwd2_rows,
                    ln_bwd_row_gemm, ln_bwd_row_gemm_supported, _ln_bwd_rows, packed_weight, row_gemm, row_gemm_ln_bwd,
                    row_gemm_ln_bwd_supported, sum3, _wgrad_many)


# --------------------------------------------------------------------------
# graph attention core  (reference src/model/layers.py:119-134)
# --------------------------------------------------------------------------
def _attn_shapes(q, e):
    B, N, C = q.shape
    if tuple(e.shape) != (B, N, N, C):
        raise RuntimeError(f"attn_core: edge tensor {tuple(e.shape)} does not match node tensor {tuple(q.shape)}")
    return B, N, C


# dg_attn_core_* hold a row's neighbours in one wave (N <= 96); dg_attn_core_long_* spread it over a workgroup (N <= 256)
ATTN_SHORT_MAX_N = 96
ATTN_MAX_N = 256


def _check_neighbours(N: int) -> None:
    if N > ATTN_MAX_N:
        raise RuntimeError(f"graph attention: {N} neighbours (vertexes / max_atom) is above the supported maximum of "
                           f"{ATTN_MAX_N}")


def _long_workspace(q, B, N, C):
    need = int(_lib.load().dg_attn_core_long_workspace_bytes(B, N, C))
    return (_scratch(q, need, "attn_long") if need else None), need


def _core_fwd(q, k, v, e, s, o, alpha, B, N, C):
    """One attention-core forward launch: dg_attn_core_fwd up to 96 neighbours, dg_attn_core_long_fwd above."""
    _check_neighbours(N)
    _lib.launch("dg_attn_core_fwd" if N <= ATTN_SHORT_MAX_N else "dg_attn_core_long_fwd", q, _lib.ptr(q), _lib.ptr(k), _lib.ptr(v),
                _lib.ptr(e), _lib.ptr(s), _lib.ptr(o), B, N, C, alpha, _lib.dt(q))
    _account("attn_fwd", q.element_size() * B * ((2 if s is not None else 1) * N * N * C + 4 * N * C))


def _core_bwd(q, k, v, e, ws, wo, add_e, dq, dk, dv, de, alpha):
    """One first-order attention-core backward launch (dg_attn_core_bwd_add / dg_attn_core_long_bwd)."""
    B, N, C = q.shape[0], q.shape[1], q.shape[2]
    _check_neighbours(N)
    extra = 0
    if N <= ATTN_SHORT_MAX_N:
        _lib.launch("dg_attn_core_bwd_add", q, _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(e), _lib.ptr(ws), _lib.ptr(wo),
                    _lib.ptr(add_e), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(de), B, N, C, alpha, _lib.dt(q))
    else:
        work, extra = _long_workspace(q, B, N, C)
        wp = work.data_ptr() if extra else None
        _lib.launch("dg_attn_core_long_bwd", q, _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(e), _lib.ptr(ws),
                    _lib.ptr(wo), _lib.ptr(add_e), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(de), wp, extra, B, N, C,
                    alpha, _lib.dt(q))
    base = q.element_size() * B * ((2 + (ws is not None) + (add_e is not None)) * N * N * C + 7 * N * C)
    _account("attn_bwd", base + 2 * extra, floor=base)      # (long path: the column partials are written and read once)


def _core_bwd2(q, k, v, e, ws, wo, tq, tk, tv, te, gq, gk, gv, ge, gws, gwo, alpha):
    """One second-order attention-core launch (dg_attn_core_bwd2 / dg_attn_core_long_bwd2)."""
    B, N, C = q.shape[0], q.shape[1], q.shape[2]
    _check_neighbours(N)
    extra = 0
    args = [_lib.ptr(x) for x in (q, k, v, e, ws, wo, tq, tk, tv, te, gq, gk, gv, ge, gws, gwo)]
    if N <= ATTN_SHORT_MAX_N:
        _lib.launch("dg_attn_core_bwd2", q, *args, B, N, C, alpha, _lib.dt(q))
    else:
        work, extra = _long_workspace(q, B, N, C)
        wp = work.data_ptr() if extra else None
        _lib.launch("dg_attn_core_long_bwd2", q, *args, wp, extra, B, N, C, alpha, _lib.dt(q))
    base = q.element_size() * B * ((5 if ws is not None else 3) * N * N * C + 11 * N * C)
    _account("attn_bwd2", base + 2 * extra, floor=base)


def _attn_bwd_launch(q, k, v, e, ws, wo, alpha, add_e=None):
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    de = torch.empty_like(e)
    _core_bwd(q, k, v, e, ws, wo, add_e, dq, dk, dv, de, alpha)
    return dq, dk, dv, de


def _attn_bwd2_launch(q, k, v, e, ws, wo, tq, tk, tv, te, alpha):
    gq, gk, gv, gwo = (torch.empty_like(q) for _ in range(4))
    ge = torch.empty_like(e)
    gws = torch.empty_like(e) if ws is not None else None
    _core_bwd2(q, k, v, e, ws, wo, tq, tk, tv, te, gq, gk, gv, ge, gws, gwo, alpha)
    return gq, gk, gv, ge, gws, gwo


class _AttnCore(Function):
    @staticmethod
    def forward(ctx, q, k, v, e, alpha, need_s):
        q, k, v, e = _c(q), _c(k), _c(v), _c(e)
        B, N, C = _attn_shapes(q, e)
        s = torch.empty_like(e) if need_s else None
        o = torch.empty_like(q)
        _core_fwd(q, k, v, e, s, o, alpha, B, N, C)
        ctx.save_for_backward(q, k, v, e)
        ctx.alpha = alpha
        ctx.set_materialize_grads(False)
        if s is None:
            s = q.new_empty(0)
            ctx.mark_non_differentiable(s)
        return s, o

    @staticmethod
    def backward(ctx, ws, wo):
        q, k, v, e = ctx.saved_tensors
        if wo is None:
            wo = torch.zeros_like(q)
        if ws is not None and ws.numel() == 0:
            ws = None
        return (*_AttnCoreBwd.apply(q, k, v, e, ws, wo, ctx.alpha), None, None)


class _AttnCoreBwd(Function):
    @staticmethod
    def forward(ctx, q, k, v, e, ws, wo, alpha):
        _attn_shapes(q, e)
        ws, wo = (None if ws is None else _c(ws)), _c(wo)
        ctx.save_for_backward(q, k, v, e, ws, wo)
        ctx.alpha = alpha
        return _attn_bwd_launch(q, k, v, e, ws, wo, alpha)

    @staticmethod
    @once_differentiable
    def backward(ctx, tq, tk, tv, te):
        q, k, v, e, ws, wo = ctx.saved_tensors
        return (*_attn_bwd2_launch(q, k, v, e, ws, wo, _c(tq), _c(tk), _c(tv), _c(te), ctx.alpha), None)


def attn_core(q, k, v, e, alpha: float, need_s: bool = True):
    """(s, o) of the edge-modulated per-channel attention.

    s[b,i,j,c] = alpha q[b,i,c] k[b,j,c] (e^2+e)[b,i,j,c];  o = sum_j softmax_j(s) v_j.
    With ``need_s=False`` the [B,N,N,C] score tensor is not written (Discriminator's
    last block never reads it, reference models.py:202-207) and ``s`` is None.
    """
    s, o = _AttnCore.apply(q, k, v, e, float(alpha), bool(need_s))
    return (s if need_s else None), o


# --------------------------------------------------------------------------
# whole attention half of an Encoder_Block as one autograd node
# --------------------------------------------------------------------------
def _composite_attn_block(x1, y, wq, bq, wk, bk, wv, bv, we, be, woe, boe, won, bon, g3, b3, g4, b4, alpha, eps3,
                          eps4, need_edge):
    q, k, v = linear(x1, wq, bq), linear(x1, wk, bk), linear(x1, wv, bv)
    e = linear(y, we, be)
    s, o = attn_core(q, k, v, e, alpha, need_s=need_edge)
    x2 = linear_ln(o, won, bon, x1, g3, b3, eps3)
    if not need_edge:
        return x2
    return x2, linear_ln(s, woe, boe, y, g4, b4, eps4)


def attn_half_f32_supported(yf, N: int, C: int) -> bool:
    """dg_attn_half_f32_fwd (e projection + attention core + out_e + residual + ln4 as one float32 launch) serves C = 128 and
    row groups of at most 96 neighbours (above 48: two stages per row group, online softmax across them);
    options.attn_half_f32 = "off" keeps the three launches, "n48" keeps them above 48 neighbours (A/B measurements)."""
    mode = options.attn_half_f32
    return yf.is_cuda and yf.dtype == torch.float32 and C == 128 and N <= (48 if mode == "n48" else 96) and mode != "off"


def attn_half_f32_bwd1_supported(dy2f, B: int, N: int, C: int, graph: bool = False) -> bool:
    """dg_attn_half_f32_bwd1 (ln4 backward + out_e input gradient + attention-core backward as one float32 launch) serves
    C = 128 and row groups of at most 48 neighbours; its workgroups walk whole molecules, so it needs a batch that fills the
    chip (B >= 128; options.attn_half_f32_bwd = "force" lifts that for tests, "off" keeps the two launches, "nograph" keeps
    them only for passes a second order differentiates)."""
    mode = options.attn_half_f32_bwd
    return (dy2f.is_cuda and dy2f.dtype == torch.float32 and C == 128 and N <= 48 and mode != "off"
            and (B >= 128 or mode == "force") and (not graph or mode != "nograph"))


# The block nodes' inputs, outputs and saved tensors by name: each tuple is the positional order of one ``forward`` (held against
# the signatures by tests/test_attention_spec_host.py), and every position the nodes need -- a needs_input_grad look-up, the slot
# of a gradient in a ``backward`` return, a saved tensor -- is derived from them (``_by_name``, ``dict(zip(names, ...))``).
_ATTN_LINEAR = ("wq", "bq", "wk", "bk", "wv", "bv", "we", "be", "woe", "boe", "won", "bon")
_ATTN_AFFINE = ("g3", "b3", "g4", "b4")      # ln3 / ln4 affine parameters
_ATTN_TENSORS = ("x1", "y") + _ATTN_LINEAR + _ATTN_AFFINE
# the parameters that leave the penalty's forward as alias outputs (see _weight_alias), in the order of those outputs
_ATTN_ALIASES = ("wq", "wk", "wv", "we", "woe", "won", "g3", "g4")
_ATTN_ADJOINTS = ("add3", "add4", "aq", "ak", "av", "ae")      # what the second order hands back to the forward node


def _by_name(names, values):
    """A node's positional inputs, or a ``backward`` return, from {name: value}: one slot per declared name, None where the
    mapping is silent; a name that is not declared raises."""
    unknown = [n for n in values if n not in names]
    if unknown:
        raise KeyError(f"{unknown} not among {names}")
    return tuple(values.get(n) for n in names)


# The node side of the block (R = B N rows), shared by the float32 / unfused nodes, their second order and the fused bf16 node
def _qkv_fwd(x2, ws, bs):
    """q, k, v of the rows ``x2`` (``bs`` entries may be None): one launch where ``lin3_supported``, else three row GEMMs."""
    if lin3_supported(x2, ws):
        return lin3(x2, ws, bs)
    C = x2.shape[1]
    return [row_gemm(x2, packed_weight(w, 0, x2.dtype), C, C, bias=b) for w, b in zip(ws, bs)]


def _qkv_bwd_input(dqkv, ws, residual):
    """residual + dq Wq + dk Wk + dv Wv: one launch where ``lin3_supported``, else three row GEMMs, each adding in its epilogue."""
    if lin3_supported(dqkv[0], ws):
        return sum3(*dqkv, ws, residual=residual)
    C = residual.shape[1]
    for d, w in zip(dqkv, ws):
        residual = row_gemm(d, packed_weight(w, 1, d.dtype), C, C, residual=residual)
    return residual


def _attn_wgrads(ws, dqkv, x2, e, out_n, out_e, want_bias, open_batch=True):
    """{input name: gradient} of the block's projections from ONE ``_wgrad_many`` call.  q, k, v: ``dqkv`` against their shared
    input rows ``x2``, one stacked [384,128] item where ``lin3_supported``, else three.  ``e`` / ``out_n`` / ``out_e``: (output
    gradient rows, input rows), or None for a projection the caller leaves out.  ``want_bias``: the first-order form (second
    order: weights only)."""
    stacked = lin3_supported(dqkv[0], ws)
    items = [(tuple(dqkv), x2, want_bias)] if stacked else [(d, x2, want_bias) for d in dqkv]
    rest = [(n, p) for n, p in (("e", e), ("on", out_n), ("oe", out_e)) if p is not None]
    items += [(dy, x, want_bias) for _, (dy, x) in rest]
    # (out_n's weight gradient over the node rows rides in out_e's over the edge rows)
    res = _wgrad_many(items, open_batch=open_batch, pair_from=len(items) - 2 if out_e is not None else None)
    if stacked:      # rows 0..127 / 128..255 / 256..383 of the stacked gradient
        (w3, b3), *res = res
        res = [(w3[r:r + 128], None if b3 is None else b3[r:r + 128]) for r in (0, 128, 256)] + res
    out = {}
    for n, (dw, db) in zip(["q", "k", "v"] + [n for n, _ in rest], res):
        out["w" + n], out["b" + n] = dw, db
    return out


def _ln3_bwd_do(pre3, g3, mean3, rstd3, dx2f, add3, won, want_aff, inb):
    """(dz3, dgamma3, dbeta3, do): ln3's backward, then the out_n input gradient do = dz3 Won."""
    dz3, dg3, db3 = _ln_bwd_rows(pre3, g3, mean3, rstd3, dx2f, add3, want_affine=want_aff, batch_slot=0 if inb else None)
    C = dz3.shape[1]
    return dz3, dg3, db3, row_gemm(dz3, packed_weight(won, 1, dz3.dtype), C, C)


# The fused launches of the edge side: tensors in, outputs allocated, one native call, one ``_account``
def _half_f32_fwd(yf, q, k, v, we, be, woe, boe, g4, b4, B, N, C, alpha, eps4, keep):
    """e projection, scores, softmax / node output, out_e, residual, ln4: one launch (dg_attn_half_f32_fwd); e, s and the
    pre-LayerNorm sum are written for the backward only (``keep``).  Returns (e, s, o, y2, pre4, mean4, rstd4)."""
    P, F = _lib.ptr, _lib.fptr
    R = yf.shape[0]
    e, s, pre4 = (torch.empty_like(yf) if keep else None for _ in range(3))
    o, y2 = torch.empty_like(q), torch.empty_like(yf)
    mean4, rstd4 = (torch.empty(R, dtype=torch.float32, device=yf.device) for _ in range(2))
    _lib.launch("dg_attn_half_f32_fwd", q, P(yf), P(q), P(k), P(v), packed_weight(we, 0, yf.dtype).data_ptr(), F(_c(be)),
                packed_weight(woe, 0, yf.dtype).data_ptr(), F(_c(boe)), F(_c(g4)), F(_c(b4)), P(e), P(s), P(o), P(y2),
                P(pre4), P(mean4), P(rstd4), B, N, C, alpha, eps4)
    _account("attn_half_fwd", 4 * (R * C * (5 if keep else 2) + 4 * B * N * C), 4 * R * C * C,
             floor=4 * (R * C * 2 + 4 * B * N * C))
    return e, s, o, y2, pre4, mean4, rstd4


def _half_f32_bwd1(dy2f, pre4, mean4, rstd4, g4, woe, ev, qv, kv, vv, do, alpha, want_aff, keep_ds, inb):
    """ln4 backward + ds = dz4 Woe + the attention core's backward: one launch (dg_attn_half_f32_bwd1); ds stays on chip
    unless ``keep_ds``.  Returns (dz4, ds, dq, dk, dv, de, dgamma4, dbeta4)."""
    lib, P = _lib.load(), _lib.ptr
    B, N, C = qv.shape
    dev, adt = dy2f.device, dy2f.dtype
    dz4, de = torch.empty_like(dy2f), torch.empty_like(dy2f)
    ds = torch.empty_like(dy2f).view(B, N, N, C) if keep_ds else None
    dq, dk, dv = (torch.empty(B, N, C, dtype=adt, device=dev) for _ in range(3))
    dg4, db4 = (torch.empty(2, C, dtype=torch.float32, device=dev).unbind(0) if want_aff else (None, None))
    ws = _scratch(dy2f, int(lib.dg_attn_half_f32_bwd1_workspace_bytes(B)), "ahb_batch" if inb else "ahb")
    woe_t = packed_weight(woe, 1, adt).data_ptr()
    _lib.launch("dg_attn_half_f32_bwd1", dy2f, P(dy2f), P(pre4), P(mean4), P(rstd4), _lib.fptr(_c(g4)), woe_t, P(ev), P(qv),
                P(kv), P(vv), P(do), P(dz4), P(ds), P(de), P(dq), P(dk), P(dv), P(dg4), P(db4), ws.data_ptr(), ws.numel(), B,
                N, C, alpha)
    _account("attn_half_bwd", 4 * (dy2f.shape[0] * C * (5 if ds is None else 6) + 7 * B * N * C), 2 * dy2f.shape[0] * C * C)
    return dz4, ds, dq, dk, dv, de.view(B, N, N, C), dg4, db4


_half_pack_cache = PackCache(1024)


def _attn_half_packed(we, woe, dtype):
    """Fragment-order copies of (e.weight, out_e.weight) and their transposes for the fused attention-half kernels
    (dg_attn_half_pack), cached like ``packed_weight``."""
    def make(we, woe):
        lib = _lib.load()
        code = _lib.DTYPES[dtype]
        packed = torch.empty(int(lib.dg_attn_half_packed_bytes(code)), dtype=torch.uint8, device=we.device)
        _lib.launch("dg_attn_half_pack", we, _lib.fptr(_c(we.detach())), _lib.fptr(_c(woe.detach())), packed.data_ptr(), code)
        return packed
    return _half_pack_cache.get((we, woe), (dtype,), make)


def _half_fwd(yc, q, k, v, we, be, woe, boe, g4, b4, B, N, C, alpha, eps4, need_edge):
    """The whole edge side of the block in one launch (dg_attn_half_fwd): e and s never exist in HBM.  Returns
    (o, y2, pre4, mean4, rstd4); the last four are None without ``need_edge``."""
    P, F = _lib.ptr, _lib.fptr
    o = torch.empty_like(q)
    y2, pre4 = (torch.empty_like(yc) if need_edge else None for _ in range(2))
    mean4, rstd4 = (torch.empty(B * N * N, dtype=torch.float32, device=q.device) if need_edge else None for _ in range(2))
    packed = _attn_half_packed(we, woe, q.dtype)
    _lib.launch("dg_attn_half_fwd", q, P(yc), P(q), P(k), P(v), packed.data_ptr(), F(_c(be)), F(_c(boe)), F(_c(g4)),
                F(_c(b4)), P(o), P(y2), P(pre4), P(mean4), P(rstd4), B, N, C, alpha, eps4, _lib.dt(q))
    es = q.element_size()
    _account("attn_half_fwd", es * B * ((3 if need_edge else 1) * N * N * C + 4 * N * C),
             2 * B * N * N * C * C * (2 if need_edge else 1), floor=es * B * ((2 if need_edge else 1) * N * N * C + 4 * N * C))
    return o, y2, pre4, mean4, rstd4


def _half_bwd(y, dz4, q, k, v, do, we, be, woe, B, N, C, alpha, wants_w, need_edge):
    """The edge side's backward in one launch (dg_attn_half_bwd): e and s are recomputed from ``y``.  Returns (dy, dq, dk, dv,
    dwe, dbe, dwoe, dboe); the weight gradients, made inside the kernel, are None unless ``wants_w`` (out_e's: and ``need_edge``)."""
    lib, P = _lib.load(), _lib.ptr
    dy = torch.empty_like(y)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    dwe = dbe = dwoe = dboe = None
    if wants_w:
        dwe, dbe = torch.empty_like(we), torch.empty(C, dtype=torch.float32, device=q.device)
    if wants_w and need_edge:
        dwoe, dboe = torch.empty_like(woe), torch.empty(C, dtype=torch.float32, device=q.device)
    ws = _scratch(q, int(lib.dg_attn_half_bwd_workspace_bytes(B, N)), "half")
    _lib.launch("dg_attn_half_bwd", q, P(y), P(dz4), P(q), P(k), P(v), P(do), _attn_half_packed(we, woe, q.dtype).data_ptr(),
                _lib.fptr(_c(be)), P(dy), P(dq), P(dk), P(dv), P(dwe), P(dbe), P(dwoe), P(dboe), ws.data_ptr(), ws.numel(), B,
                N, C, alpha, _lib.dt(q))
    es = q.element_size()
    _account("attn_half_bwd", es * B * ((3 if need_edge else 2) * N * N * C + 8 * N * C),
             2 * B * N * N * C * C * ((3 if need_edge else 2) + (2 if wants_w and need_edge else (1 if wants_w else 0))))
    return dy, dq, dk, dv, dwe, dbe, dwoe, dboe


_LN_HANDLE = ("ppre", "pmean", "prstd", "pgamma", "pbeta")
_ATTN_IN = _ATTN_TENSORS + ("alpha", "eps3", "eps4", "need_edge") + _LN_HANDLE      # _AttnBlock.forward
# _AttnBlock.forward's outputs = the gradients its backward receives: with / without the edge output, then the aliases
_ATTN_OUT_EDGE = ("x2", "y2", "pre3", "pre4", "q", "k", "v", "e")
_ATTN_OUT_NODE = ("x2", "pre3", "q", "k", "v", "e")
# what _AttnBlock saves: always; when need_edge; when an LNHandle came in
_ATTN_SAVED = ("x1", "y") + _ATTN_ALIASES + ("q", "k", "v", "e", "s", "o", "mean3", "rstd3", "pre3")
_ATTN_SAVED_EDGE = ("mean4", "rstd4", "pre4")
_ATTN_SAVED_PREV = ("ppre", "pmean", "prstd", "pgamma")


def _attn_saved(need_edge, has_prev):
    """Names of the tensors ``_AttnBlock`` saves, in saved order."""
    return _ATTN_SAVED + (_ATTN_SAVED_EDGE if need_edge else ()) + (_ATTN_SAVED_PREV if has_prev else ())


class _AttnBlock(Function):
    """x2 = LN3(x1 + out_n(o)), y2 = LN4(y + out_e(s)) with (s, o) = attention(q(x1), k(x1), v(x1), e(y))
    -- reference layers.py:111-135 + 186-190 -- as ONE autograd node: every projection is a row-GEMM
    launch with its bias / residual / LayerNorm epilogue, and in the backward every gradient
    accumulation (y feeds e-proj and the ln4 residual; x1 feeds q, k, v and the ln3 residual) is the
    residual operand of the next GEMM's epilogue instead of a separate elementwise add."""

    @staticmethod
    def forward(ctx, x1, y, wq, bq, wk, bk, wv, bv, we, be, woe, boe, won, bon, g3, b3, g4, b4, alpha, eps3, eps4,
                need_edge, ppre=None, pmean=None, prstd=None, pgamma=None, pbeta=None):
        # ppre .. pbeta: LNHandle of the LayerNorm that produced y (or None): its backward can then run in the
        # epilogue of this node's dy GEMM, the result leaving as the gradient of `ppre` instead of `y`
        B, N, C = x1.shape
        _check_neighbours(N)
        x1f, yf = _c(x1).reshape(-1, C), _c(y).reshape(-1, C)
        adt = x1f.dtype
        pw = lambda w_, m_: packed_weight(w_, m_, adt)
        q, k, v = _qkv_fwd(x1f, (wq, wk, wv), (bq, bk, bv))
        # no input needs a gradient (the Generator's forward inside the D step): the pre-LayerNorm sums are not written
        keep = any(ctx.needs_input_grad)
        y2 = mean4 = rstd4 = pre4 = None
        fused_edge = need_edge and attn_half_f32_supported(yf, N, C)
        if fused_edge:
            e, s, o, y2, pre4, mean4, rstd4 = _half_f32_fwd(yf, q, k, v, we, be, woe, boe, g4, b4, B, N, C, alpha, eps4, keep)
        else:
            e = row_gemm(yf, pw(we, 0), C, C, bias=be)
            s = torch.empty_like(e) if need_edge else None
            o = torch.empty_like(q)
            _core_fwd(q, k, v, e, s, o, alpha, B, N, C)
        r3 = row_gemm(o, pw(won, 0), C, C, bias=bon, residual=x1f, ln=(_c(g3), _c(b3), eps3), want_pre=keep)
        x2, mean3, rstd3, pre3 = r3 if keep else (*r3, None)
        if need_edge and not fused_edge:
            r4 = row_gemm(s, pw(woe, 0), C, C, bias=boe, residual=yf, ln=(_c(g4), _c(b4), eps4), want_pre=keep)
            y2, mean4, rstd4, pre4 = r4 if keep else (*r4, None)
        have = dict(x1=x1, y=y, wq=wq, wk=wk, wv=wv, we=we, woe=woe, won=won, g3=g3, g4=g4, q=q, k=k, v=v, e=e, s=s, o=o,
                    mean3=mean3, rstd3=rstd3, pre3=pre3, mean4=mean4, rstd4=rstd4, pre4=pre4,
                    ppre=ppre, pmean=pmean, prstd=prstd, pgamma=pgamma)
        # the penalty's forward: the parameters leave as alias outputs, and the aliases are what is saved (see _weight_alias)
        ctx.alias = bool(keep and in_second_order_forward() and _alias_outputs_enabled())
        if ctx.alias:
            have.update({n: _weight_alias(have[n]) for n in _ATTN_ALIASES})
        ctx.has_prev = ppre is not None
        ctx.save_for_backward(*(have[n] for n in _attn_saved(need_edge, ctx.has_prev)))
        ctx.cfg = (alpha, eps3, eps4, need_edge, (B, N, C))
        ctx.extra = (bq, bk, bv, be, boe, bon, b3, b4)
        ctx.set_materialize_grads(False)
        # pre3 / pre4 / q / k / v / e are outputs only so that the second order of the gradient penalty
        # can return their adjoints to THIS node, where they join the first-order gradients inside one
        # backward pass (see _AttnBlockBwd.backward); module code never sees them.
        have.update(x2=x2.view(B, N, C), y2=y2.view(B, N, N, C) if need_edge else None)
        return tuple(have[n] for n in (_ATTN_OUT_EDGE if need_edge else _ATTN_OUT_NODE) + (_ATTN_ALIASES if ctx.alias else ()))

    @staticmethod
    def backward(ctx, *gouts):
        alpha, eps3, eps4, need_edge, (B, N, C) = ctx.cfg
        # gradients of the outputs by output name; the aliases' are the second-order gradients of the parameters (or None each)
        g = dict(zip((_ATTN_OUT_EDGE if need_edge else _ATTN_OUT_NODE) + (_ATTN_ALIASES if ctx.alias else ()), gouts))
        sv = dict(zip(_attn_saved(need_edge, ctx.has_prev), ctx.saved_tensors))
        bq, bk, bv, be, boe, bon, b3, b4 = ctx.extra
        needs = dict(zip(_ATTN_IN, ctx.needs_input_grad))
        dx2 = g["x2"] if g["x2"] is not None else torch.zeros_like(sv["pre3"])
        dy2 = g.get("y2")
        if need_edge and dy2 is None:
            dy2 = torch.zeros_like(sv["pre4"])
        adjoints = dict(add3=g["pre3"], add4=g.get("pre4"), aq=g["q"], ak=g["k"], av=g["v"], ae=g["e"])
        wants_w = needs["wq"] and not _inputs_only()
        want_aff = any(needs[n] for n in _ATTN_AFFINE) and not _inputs_only()
        # y is the output of a LayerNorm whose handle came with it, and no graph is being recorded: that LayerNorm's
        # backward runs as the epilogue of the dy GEMM (its result is the gradient of `ppre`, y itself gets none)
        # (not in the last pass of a double backward -- recognisable by the adjoints of this node's extra outputs: there
        # the producing feed-forward node's `pre` ALSO receives the second-order adjoint, and autograd would join the
        # two with an edge-level add that costs more than the fused LayerNorm backward saves)
        second_pass = any(t is not None for t in adjoints.values())
        fuse_prev = bool(ctx.has_prev and not torch.is_grad_enabled() and not second_pass and needs["y"]
                         and needs["ppre"] and row_gemm_ln_bwd_supported(sv["q"], C)
                         and tuple(sv["ppre"].shape) == (B * N * N, C))
        ins = dict(sv, **adjoints, bq=bq, bk=bk, bv=bv, be=be, boe=boe, bon=bon, dx2=dx2, dy2=dy2, alpha=alpha,
                   need_edge=need_edge, want_x=needs["x1"], want_y=needs["y"], wants_w=wants_w, want_aff=want_aff,
                   no_graph=not torch.is_grad_enabled())      # (no graph is being recorded: see _AttnBlockBwd)
        if not fuse_prev:
            ins["ppre"] = None
        outs = _AttnBlockBwd.apply(*_by_name(_ATTN_BWD_IN, ins))
        grads = dict(zip(_ATTN_BWD_OUT, outs))
        galias = [g.get(n) for n in _ATTN_ALIASES]
        if any(t is not None for t in galias):
            grads.update(zip(_ATTN_ALIASES, _join_alias_grads([grads[n] for n in _ATTN_ALIASES], galias)))
        if not (needs["pgamma"] and not _inputs_only()):
            grads["pgamma"] = grads["pbeta"] = None
        return _by_name(_ATTN_IN, grads)


# _AttnBlockBwd.forward's inputs, and its outputs: the gradients of these inputs of _AttnBlock.forward
_ATTN_BWD_IN = (("x1", "y") + _ATTN_LINEAR + ("g3", "g4", "q", "k", "v", "e", "s", "o", "mean3", "rstd3", "pre3", "mean4", "rstd4",
                                              "pre4", "dx2", "dy2") + _ATTN_ADJOINTS
                + ("alpha", "need_edge", "want_x", "want_y", "wants_w", "ppre", "pmean", "prstd", "pgamma", "want_aff", "no_graph"))
_ATTN_BWD_OUT = _ATTN_TENSORS + ("ppre", "pgamma", "pbeta")


class _AttnBlockBwd(Function):
    """Backward of ``_AttnBlock`` as a differentiable node; its own backward (second order of the
    gradient penalty) chains the same kernels: row GEMMs for every projection (forward packs where the
    first backward used the input-gradient packs and vice versa), dg_attn_core_bwd2 for the attention
    core, dg_ln_residual_bwd2 for ln3 / ln4.  The adjoints that reach the forward intermediates
    (pre-LayerNorm sums, q, k, v, e) are handed to the forward node as gradients of its extra outputs;
    they come back in as add3 / add4 / aq / ak / av / ae and are summed into the single first-order
    pass of that node."""

    @staticmethod
    def forward(ctx, *args):
        # one reduce launch for the block: six weight gradients + two LayerNorms' dgamma / dbeta
        named = dict(zip(_ATTN_BWD_IN, args))
        wants_w = named["wants_w"] or named.get("want_aff")      # weight gradients or LayerNorm affine gradients
        with _reduce_batch(named["x1"], on=bool(wants_w)) as inb:
            return _AttnBlockBwd._forward(ctx, inb, *args)

    @staticmethod
    def _forward(ctx, inb, x1, y, wq, bq, wk, bk, wv, bv, we, be, woe, boe, won, bon, g3, g4, q, k, v, e, s, o,
                 mean3, rstd3, pre3, mean4, rstd4, pre4, dx2, dy2, add3, add4, aq, ak, av, ae,
                 alpha, need_edge, want_x, want_y, wants_w, ppre=None, pmean=None, prstd=None, pgamma=None, want_aff=None,
                 no_graph=False):
        if want_aff is None:
            want_aff = wants_w
        B, N, C = x1.shape
        adt = q.dtype
        pw = lambda w_, m_: packed_weight(w_, m_, adt)
        cast = lambda t: t if t.dtype == adt else t.to(adt)
        x1f, yf = _c(x1).reshape(-1, C), _c(y).reshape(-1, C)
        dx2f = _c(cast(dx2)).reshape(-1, C)
        cadd = lambda t: None if t is None else _c(cast(t)).reshape(-1, C)
        dz3, dg3, db3, do = _ln3_bwd_do(pre3, g3, mean3, rstd3, dx2f, cadd(add3), won, want_aff, inb)
        do = do.view(B, N, C)
        ds = dz4 = dg4 = db4 = dy2f = None
        qv, kv, vv, ev = q.view(B, N, C), k.view(B, N, C), v.view(B, N, C), e.view(B, N, N, C)
        fused1 = None
        if need_edge:
            dy2f = _c(cast(dy2)).reshape(-1, C)
            if (add4 is None and all(t is None for t in (aq, ak, av, ae))
                    and attn_half_f32_bwd1_supported(dy2f, B, N, C, graph=not no_graph)):
                # one launch; ds stays on chip unless a graph is being recorded (the penalty's first backward: its second
                # order reads ds)
                dz4, ds, *fused1, dg4, db4 = _half_f32_bwd1(dy2f, pre4, mean4, rstd4, g4, woe, ev, qv, kv, vv, do, alpha,
                                                            want_aff, not no_graph, inb)
            elif add4 is None and dy2f.shape[0] >= _lib.edge_rows() and ln_bwd_row_gemm_supported(dy2f, C, C):
                # ln4's backward runs in the producer waves of the out_e input-gradient GEMM (edge-level launches only:
                # at node level the three small launches it replaces are faster)
                dz4, ds, dg4, db4 = ln_bwd_row_gemm(pre4, g4, mean4, rstd4, dy2f, pw(woe, 1), want_affine=want_aff,
                                                    batch_slot=1 if inb else None)
                ds = ds.view(B, N, N, C)
            else:
                dz4, dg4, db4 = _ln_bwd_rows(pre4, g4, mean4, rstd4, dy2f, cadd(add4), want_affine=want_aff,
                                             batch_slot=1 if inb else None)
                ds = row_gemm(dz4, pw(woe, 1), C, C).view(B, N, N, C)
        # fp32: the adjoint of e joins de inside the kernel (one read stream instead of a 3-pass add).  The bf16
        # variant of that kernel is latency-bound at 2 waves / SIMD and the extra operand set costs more than the add
        # it saves (configs[2], A/B on one box: 217.2 vs 213.7 ms per step): bf16 adds afterwards.
        fold = ae is not None and adt == torch.float32
        aef = _c(cast(ae)).view(B, N, N, C) if fold else None      # joins de inside the kernel
        dq, dk, dv, de = fused1 if fused1 is not None else _attn_bwd_launch(qv, kv, vv, ev, ds, do, alpha, add_e=aef)
        pairs = [(got, extra.view(got.shape)) for got, extra in ((dq, aq), (dk, ak), (dv, av)) if extra is not None]
        if pairs:      # the node-level adjoints of q, k, v (second pass of the penalty): one multi-tensor launch
            torch._foreach_add_([g_ for g_, _ in pairs], [e_ if e_.dtype == g_.dtype else e_.to(g_.dtype) for g_, e_ in pairs])
        if ae is not None and not fold:
            de.add_(ae.view(de.shape))
        ctx.third = any(t is not None for t in (add3, add4, aq, ak, av, ae))
        dqf, dkf, dvf, def_ = dq.view(-1, C), dk.view(-1, C), dv.view(-1, C), de.view(-1, C)
        dy = dx1 = dzp = dgp = dbp = None
        if want_y and ppre is not None:      # + ln4 residual path, then the backward of the LayerNorm that made y
            dzp, dgp, dbp = row_gemm_ln_bwd(def_, pw(we, 1), C, dz4, ppre, pgamma, pmean, prstd)
        elif want_y:
            dy = row_gemm(def_, pw(we, 1), C, C, residual=dz4).view(y.shape)      # + ln4 residual path
        if want_x:
            dx1 = _qkv_bwd_input((dqf, dkf, dvf), (wq, wk, wv), dz3).view(x1.shape)      # + ln3 residual path
        gw = {}
        if wants_w:
            gw = _attn_wgrads((wq, wk, wv), (dqf, dkf, dvf), x1f, (def_, yf), (dz3, o), (dz4, s) if need_edge else None,
                              want_bias=True, open_batch=not inb)
        ctx.save_for_backward(x1, y, wq, wk, wv, we, woe, won, g3, g4, q, k, v, e, s, o, mean3, rstd3, pre3,
                              mean4, rstd4, pre4, dx2f, dy2f, dz3, dz4, do, ds, dq, dk, dv, de)
        ctx.cfg = (alpha, need_edge, (B, N, C), dx2.shape, None if dy2 is None else dy2.shape)
        ctx.set_materialize_grads(False)
        return _by_name(_ATTN_BWD_OUT, dict(gw, x1=dx1, y=dy, g3=dg3, b3=db3, g4=dg4, b4=db4, ppre=dzp, pgamma=dgp, pbeta=dbp))

    @staticmethod
    @once_differentiable
    def backward(ctx, t1, ty, *rest):
        if any(r is not None for r in rest):
            raise RuntimeError("attn_block: second-order terms through parameter gradients are not implemented")
        if ctx.third:
            raise RuntimeError("attn_block: third-order differentiation is not implemented")
        alpha, need_edge, (B, N, C), dx2_shape, dy2_shape = ctx.cfg
        (x1, y, wq, wk, wv, we, woe, won, g3, g4, q, k, v, e, s, o, mean3, rstd3, pre3, mean4, rstd4, pre4,
         dx2f, dy2f, dz3, dz4, do, ds, dq, dk, dv, de) = ctx.saved_tensors
        adt = q.dtype
        pw = lambda w_, m_: packed_weight(w_, m_, adt)
        cast = lambda t: t if t.dtype == adt else t.to(adt)
        t1f = _c(cast(t1)).reshape(-1, C) if t1 is not None else torch.zeros(B * N, C, dtype=adt, device=q.device)
        tyf = _c(cast(ty)).reshape(-1, C) if ty is not None else torch.zeros(B * N * N, C, dtype=adt, device=q.device)
        dqf, dkf, dvf, def_ = dq.view(-1, C), dk.view(-1, C), dv.view(-1, C), de.view(-1, C)
        # adjoints of dq, dk, dv, de (dx1 = dz3 + dq Wq + dk Wk + dv Wv ; dy = dz4 + de We)
        tq, tk, tv = _qkv_fwd(t1f, (wq, wk, wv), (None, None, None))
        te = row_gemm(tyf, pw(we, 0), C, C)
        qv, kv, vv, ev = q.view(B, N, C), k.view(B, N, C), v.view(B, N, C), e.view(B, N, N, C)
        gq, gk, gv, ge, gws, gwo = _attn_bwd2_launch(qv, kv, vv, ev, ds, do, tq.view(B, N, C), tk.view(B, N, C),
                                                     tv.view(B, N, C), te.view(B, N, N, C), alpha)
        # adjoints of dz3 / dz4 (do = dz3 Won, ds = dz4 Woe, plus the direct residual terms)
        adz3 = row_gemm(gwo.view(-1, C), pw(won, 0), C, C, residual=t1f)
        z3bar, dx2bar, g3bar = _ln_bwd2_rows(pre3, g3, mean3, rstd3, dx2f, adz3)
        z4bar = dy2bar = g4bar = None
        if need_edge:
            adz4 = row_gemm(gws.view(-1, C), pw(woe, 0), C, C, residual=tyf)
            z4bar, dy2bar, g4bar = _ln_bwd2_rows(pre4, g4, mean4, rstd4, dy2f, adz4)
        gW = {}
        if not _inputs_only():
            gW = _attn_wgrads((wq, wk, wv), (dqf, dkf, dvf), t1f, (def_, tyf), (dz3, gwo.view(-1, C)),
                              (dz4, gws.view(-1, C)) if need_edge else None, want_bias=False)
        # The outputs depend on x1 / y only through the forward intermediates: their adjoints
        # (z3bar, z4bar at the pre-LayerNorm sums; gq, gk, gv, ge) go to the forward node.
        return _by_name(_ATTN_BWD_IN, dict(gW, g3=g3bar, g4=g4bar, q=gq.view_as(q), k=gk.view_as(k), v=gv.view_as(v),
                                           e=ge.view_as(e), pre3=z3bar, pre4=z4bar, dx2=dx2bar.view(dx2_shape),
                                           dy2=None if dy2bar is None else dy2bar.view(dy2_shape)))


def _fused_attn_half_enabled() -> bool:
    """options.attn_half = "unfused" keeps the bf16 attention half on the separate launches (A/B measurements)."""
    return options.attn_half != "unfused"


def attn_half_supported(dtype, N: int, C: int) -> bool:
    """Shapes the module path routes to the fused attention-half kernels.  The kernels accept N <= 96, but above 48 the
    backward keeps 6 row blocks of accumulators per lane and spills (N = 90, B = 64: 633 vs 645 molecules/s for the
    separate launches), so BASELINE configs[4] stays on those; options.attn_half = "force" routes every N <= 96 (tests)."""
    limit = 96 if options.attn_half == "force" else 48
    return dtype == torch.bfloat16 and C == 128 and 1 <= N <= limit


_ATTN_FUSED_IN = _ATTN_TENSORS + ("alpha", "eps3", "eps4", "need_edge")      # _AttnBlockFused.forward


class _AttnBlockFused(Function):
    """The same block as ``_AttnBlock`` with the whole EDGE side -- e-projection, Hadamard score, softmax over j, AV,
    out_e, residual, ln4 (reference layers.py:116-135,186-190) -- in ONE kernel per direction (csrc/attn_half.hip):
    ``e`` and ``s`` never exist in HBM, the backward recomputes them from the saved layer input ``y`` and accumulates
    the weight gradients of e / out_e inside the kernel.  The node side (q, k, v, out_n + ln3; R = B N rows) stays on
    the row GEMMs.  First order only: graphs that will be differentiated twice are built from ``_AttnBlock``."""

    @staticmethod
    def forward(ctx, x1, y, wq, bq, wk, bk, wv, bv, we, be, woe, boe, won, bon, g3, b3, g4, b4, alpha, eps3, eps4,
                need_edge):
        B, N, C = x1.shape
        x1f = _c(x1).reshape(-1, C)
        yc = _c(y)
        q, k, v = _qkv_fwd(x1f, (wq, wk, wv), (bq, bk, bv))
        o, y2, pre4, mean4, rstd4 = _half_fwd(yc, q, k, v, we, be, woe, boe, g4, b4, B, N, C, alpha, eps4, need_edge)
        x2, mean3, rstd3, pre3 = row_gemm(o, packed_weight(won, 0, x1f.dtype), C, C, bias=bon, residual=x1f,
                                          ln=(_c(g3), _c(b3), eps3), want_pre=True)
        ctx.save_for_backward(x1, yc, wq, wk, wv, we, woe, won, g3, g4, be, q, k, v, o, mean3, rstd3, pre3, mean4, rstd4, pre4)
        ctx.cfg = (alpha, need_edge, (B, N, C))
        ctx.extra = (bq, bk, bv, boe, bon, b3, b4, eps3, eps4)
        ctx.set_materialize_grads(False)
        return (x2.view(B, N, C), y2) if need_edge else x2.view(B, N, C)

    @staticmethod
    def backward(ctx, dx2, dy2=None):
        needs = dict(zip(_ATTN_FUSED_IN, ctx.needs_input_grad))
        alpha, need_edge, (B, N, C) = ctx.cfg
        x1, y, wq, wk, wv, we, woe, won, g3, g4, be, q, k, v, o, mean3, rstd3, pre3, mean4, rstd4, pre4 = ctx.saved_tensors
        if torch.is_grad_enabled():      # create_graph=True outside second_order_forward(): composite graph
            bq, bk, bv, boe, bon, b3, b4, eps3, eps4 = ctx.extra
            ins = (x1, y, wq, bq, wk, bk, wv, bv, we, be, woe, boe, won, bon, g3, b3, g4, b4)
            gouts = (dx2, dy2) if need_edge else dx2
            return _by_name(_ATTN_FUSED_IN, dict(zip(_ATTN_TENSORS, _double_backward_fallback(
                lambda *t: _composite_attn_block(*t, alpha, eps3, eps4, need_edge), ins, gouts))))
        rows = lambda t: _c(t if t.dtype == q.dtype else t.to(q.dtype)).reshape(-1, C)
        wants_w = needs["wq"] and not _inputs_only()
        want_aff = any(needs[n] for n in _ATTN_AFFINE) and not _inputs_only()
        with _reduce_batch(x1, on=bool(wants_w or want_aff)) as inb:      # one reduce launch for the block
            dz3, dg3, db3, do = _ln3_bwd_do(pre3, g3, mean3, rstd3, rows(torch.zeros_like(pre3) if dx2 is None else dx2), None,
                                            won, want_aff, inb)
            dz4 = dg4 = db4 = None
            if need_edge:
                dz4, dg4, db4 = _ln_bwd_rows(pre4.view(-1, C), g4, mean4, rstd4, rows(torch.zeros_like(pre4) if dy2 is None else dy2),
                                             want_affine=want_aff, batch_slot=1 if inb else None)
            dy, dq, dk, dv, dwe, dbe, dwoe, dboe = _half_bwd(y, dz4, q, k, v, do, we, be, woe, B, N, C, alpha, wants_w, need_edge)
            dx1 = None
            if needs["x1"]:
                dx1 = _qkv_bwd_input((dq, dk, dv), (wq, wk, wv), dz3).view(x1.shape)      # + ln3 residual path
            gw = {}
            if wants_w:      # (e / out_e: their gradients come out of the kernel)
                gw = _attn_wgrads((wq, wk, wv), (dq, dk, dv), _c(x1).reshape(-1, C), None, (dz3, o), None, want_bias=True,
                                  open_batch=not inb)
                gw.update(we=dwe, be=dbe, woe=dwoe, boe=dboe)
        return _by_name(_ATTN_FUSED_IN, dict(gw, x1=dx1, y=dy if needs["y"] else None, g3=dg3, b3=db3, g4=dg4, b4=db4))


def attn_block(x1, y, attn, ln3, ln4, need_edge=True, y_ln=None):
    """Attention half of an encoder block for ``attn`` (an MHA module): returns
    (LN3(x1 + out_n(o)), LN4(y + out_e(s)) or None).  ``y_ln``: the LNHandle of the LayerNorm whose output y is
    (``ffn_ln(..., want_handle=True)``), or None."""
    C = x1.shape[-1]
    alpha = 1.0 / (attn.d_k ** 0.5)
    args = (x1, y, attn.q.weight, attn.q.bias, attn.k.weight, attn.k.bias, attn.v.weight, attn.v.bias,
            attn.e.weight, attn.e.bias, attn.out_e.weight, attn.out_e.bias, attn.out_n.weight, attn.out_n.bias,
            ln3.weight, ln3.bias, ln4.weight, ln4.bias)
    fused = (x1.is_cuda and x1.dtype in _lib.DTYPES and y.dtype == x1.dtype and C == 128 and x1.dim() == 3
             and all(t is not None for t in args))
    if not fused:
        out = _composite_attn_block(*args, alpha, ln3.eps, ln4.eps, need_edge)
        return out if need_edge else (out, None)
    if (not in_second_order_forward() and attn_half_supported(x1.dtype, x1.shape[1], C) and _fused_attn_half_enabled()
            and tuple(y.shape) == (x1.shape[0], x1.shape[1], x1.shape[1], C)):
        out = _AttnBlockFused.apply(*args, alpha, ln3.eps, ln4.eps, need_edge)
        return tuple(out) if need_edge else (out, None)
    prev = (None,) * len(_LN_HANDLE) if y_ln is None else (y_ln.pre, y_ln.mean, y_ln.rstd, y_ln.gamma, y_ln.beta)
    out = _AttnBlock.apply(*args, alpha, ln3.eps, ln4.eps, need_edge, *prev)
    if need_edge:
        x2, y2, *_ = out      # _ATTN_OUT_EDGE
        return x2, y2
    x2, *_ = out              # _ATTN_OUT_NODE
    return x2, None
