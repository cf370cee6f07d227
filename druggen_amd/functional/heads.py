"""The small layers at both ends of the networks: the Generator's readouts, the node embedding chain and the Discriminator's head
(reference src/model/models.py:63-66,95-101,165-171,200-207)."""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from ._runtime import _account, _c, in_second_order_forward, _inputs_only, _scratch
from .dense import _double_backward_fallback, linear, _wgrad


def _readout_entries(N):
    """(prefix of the _fwd / _dgrad / _wgrad entries, their workspace query) of a readout with N classes."""
    if N <= 16:
        return "dg_skinny_linear", "dg_linear_wgrad_workspace_bytes"
    return "dg_wide_linear", "dg_wide_linear_wgrad_workspace_bytes"      # readout_n of a --features model (N = m_dim)


class _Readout(Function):
    """nn.Linear(128 -> N <= 255) over edge / node rows with float32 logits whatever the activation dtype (reference
    models.py:67-68,100-101: readout_e / readout_n): one streaming kernel per direction (N <= 16: dg_skinny_linear_fwd /
    _dgrad / _wgrad; wider: dg_wide_linear_*) instead of `x.float()` + a library GEMM.  First order; a graph that is
    differentiated again goes through the composite."""

    @staticmethod
    def forward(ctx, x, w, b):
        N, K = w.shape
        x2 = _c(x).reshape(-1, K)
        R = x2.shape[0]
        y = torch.empty(R, N, dtype=torch.float32, device=x.device)
        _lib.launch(_readout_entries(N)[0] + "_fwd", x2, _lib.ptr(x2), _lib.fptr(_c(w)), _lib.fptr(None if b is None else _c(b)),
                    _lib.ptr(y), R, N, K, _lib.dt(x2))
        _account("readout", x2.element_size() * R * K + 4 * R * N)
        ctx.save_for_backward(x, w, b)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _double_backward_fallback(lambda x_, w_, b_: torch.nn.functional.linear(x_.float(), w_, b_),
                                             (x, w, b), dy)
        N, K = w.shape
        entry, ws_query = _readout_entries(N)
        dy2 = _c(dy.float()).reshape(-1, N)
        x2 = _c(x).reshape(-1, K)
        R = x2.shape[0]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2)
            _lib.launch(entry + "_dgrad", x2, _lib.ptr(dy2), _lib.fptr(_c(w)), _lib.ptr(dx), R, N, K, _lib.dt(x2))
            _account("readout", x2.element_size() * R * K + 4 * R * N)
        if ctx.needs_input_grad[1] and not _inputs_only():
            dw = torch.empty_like(w)
            db = torch.empty(N, dtype=torch.float32, device=x.device) if b is not None else None
            ws = _scratch(x2, int(getattr(_lib.load(), ws_query)(R, N, K)), "wgrad")
            _lib.launch(entry + "_wgrad", x2, _lib.ptr(dy2), _lib.ptr(x2), _lib.ptr(dw), _lib.ptr(db), ws.data_ptr(),
                        ws.numel(), R, N, K, _lib.dt(x2))
            _account("linear_wgrad", x2.element_size() * R * K + 4 * R * N)
        return (None if dx is None else dx.view(x.shape)), dw, db


_HEAD_ACTS = {"relu": 0, "leaky": 1, "sigmoid": 2, "tanh": 3}
_SMOOTH_ACT_FNS = {2: torch.sigmoid, 3: torch.tanh}      # first order on the chain kernels; a second order takes the composite


def _composite_node_embed(z, w1, b1, w2, b2, act):
    f = _SMOOTH_ACT_FNS[act]
    return f(linear(f(linear(z, w1, b1)), w2, b2))


def _composite_head_tail(z1, w2, b2, w3, b3, w4, b4, act):
    f, lin = _SMOOTH_ACT_FNS[act], torch.nn.functional.linear
    return lin(f(lin(f(lin(f(z1), w2, b2)), w3, b3)), w4, b4)


def _node_entry(E, which):
    """dg_embed_node_chain / _bwd for E <= 16 (the launches of a model without --features, unchanged), the wide entries above."""
    return ("dg_embed_node_" if E <= 16 else "dg_embed_node_wide_") + which


def _node_wgrad1(g1, z2, want_bias):
    """Weight gradient of the chain's first Linear, dW1 [64,E] = g1^T z2 (+ db1): E <= 16 as before (``_wgrad``'s swapped
    skinny kernel), wider on dg_embed_node_wide_wgrad."""
    R, E = z2.shape
    if E <= 16:
        return _wgrad(g1, z2, want_bias)
    dw = torch.empty(64, E, dtype=torch.float32, device=g1.device)
    db = torch.empty(64, dtype=torch.float32, device=g1.device) if want_bias else None
    ws = _scratch(g1, int(_lib.load().dg_embed_node_wide_wgrad_workspace_bytes(R, E)), "wgrad")
    _lib.launch("dg_embed_node_wide_wgrad", g1, _lib.ptr(g1), _lib.ptr(z2), _lib.ptr(dw), _lib.ptr(db), ws.data_ptr(), ws.numel(),
                R, E)
    _account("linear_wgrad", 4 * R * (64 + E), 2 * R * 64 * E)
    return dw, db


class _NodeEmbed(Function):
    """Linear(E, 64) - act - Linear(64, 128) - act over the node rows (reference models.py:52-56, 154-158) as ONE launch
    (dg_embed_node_chain, E > 16: dg_embed_node_wide_chain); backward: one launch for g2 / g1 / dz (dg_embed_node_bwd /
    dg_embed_node_wide_bwd) + the two weight gradients (dg_linear_wgrad; E > 16: the first Linear's on
    dg_embed_node_wide_wgrad); differentiable again (``_NodeEmbedBwd``: the penalty's second order is the chain kernel with the
    activation pattern as a mask; sigmoid / tanh, act'' != 0: the composite graph)."""

    @staticmethod
    def forward(ctx, z, w1, b1, w2, b2, act):
        E = z.shape[-1]
        z2 = _c(z).reshape(-1, E)
        R = z2.shape[0]
        a1 = torch.empty(R, 64, dtype=torch.float32, device=z.device)
        a2 = torch.empty(R, 128, dtype=torch.float32, device=z.device)
        _lib.launch(_node_entry(E, "chain"), z2, _lib.ptr(z2), None, None, _lib.fptr(_c(w1)), _lib.fptr(_c(b1)),
                    _lib.fptr(_c(w2)), _lib.fptr(_c(b2)), _lib.ptr(a1), _lib.ptr(a2), R, E, act)
        ctx.save_for_backward(z2, a1, a2, w1, w2, *((z, b1, b2) if act in _SMOOTH_ACT_FNS else ()))
        ctx.act, ctx.zshape = act, z.shape
        return a2.view(*z.shape[:-1], 128)

    @staticmethod
    def backward(ctx, g):
        z2, a1, a2, w1, w2 = ctx.saved_tensors[:5]
        if ctx.act in _SMOOTH_ACT_FNS and torch.is_grad_enabled():
            z, b1, b2 = ctx.saved_tensors[5:]
            act = ctx.act
            return _double_backward_fallback(lambda *t: _composite_node_embed(*t, act), (z, w1, b1, w2, b2), g) + (None,)
        need_w = any(ctx.needs_input_grad[1:5]) and not _inputs_only()
        dz, dw1, db1, dw2, db2 = _NodeEmbedBwd.apply(g, z2, a1, a2, w1, w2, ctx.needs_input_grad[0], need_w, ctx.act)
        return (None if dz is None else dz.view(ctx.zshape)), dw1, db1, dw2, db2, None


class _NodeEmbedBwd(Function):
    @staticmethod
    def forward(ctx, g, z2, a1, a2, w1, w2, need_z, need_w, act):
        gshape = g.shape
        g = _c(g.float()).reshape(-1, 128)
        R, E = z2.shape
        dev = z2.device
        g2 = torch.empty(R, 128, dtype=torch.float32, device=dev)
        g1 = torch.empty(R, 64, dtype=torch.float32, device=dev)
        dz = torch.empty(R, E, dtype=torch.float32, device=dev) if need_z else None
        _lib.launch(_node_entry(E, "bwd"), z2, _lib.ptr(g), _lib.ptr(a1), _lib.ptr(a2), _lib.fptr(_c(w1)), _lib.fptr(_c(w2)),
                    _lib.ptr(g2), _lib.ptr(g1), _lib.ptr(dz), R, E, act)
        dw1 = db1 = dw2 = db2 = None
        if need_w:
            dw2, db2 = _wgrad(g2, a1, True)
            dw1, db1 = _node_wgrad1(g1, z2, True)
        ctx.save_for_backward(z2, a1, a2, w1, w2, g1, g2)
        ctx.act, ctx.gshape = act, gshape
        ctx.set_materialize_grads(False)
        return dz, dw1, db1, dw2, db2

    @staticmethod
    @once_differentiable
    def backward(ctx, t_dz, *tw):
        if any(t is not None for t in tw):
            raise RuntimeError("node_embed: second-order terms through parameter gradients are not implemented")
        if t_dz is None:
            return (None,) * 9
        z2, a1, a2, w1, w2, g1, g2 = ctx.saved_tensors
        R, E = z2.shape
        t = _c(t_dz.float()).reshape(-1, E)
        dev = z2.device
        u1 = torch.empty(R, 64, dtype=torch.float32, device=dev)
        u2 = torch.empty(R, 128, dtype=torch.float32, device=dev)
        _lib.launch(_node_entry(E, "chain"), z2, _lib.ptr(t), _lib.ptr(a1), _lib.ptr(a2), _lib.fptr(_c(w1)), None,
                    _lib.fptr(_c(w2)), None, _lib.ptr(u1), _lib.ptr(u2), R, E, ctx.act)
        gw1 = gw2 = None
        if not _inputs_only():
            gw1, _ = _node_wgrad1(g1, t, False)
            gw2, _ = _wgrad(g2, u1, False)
        # act'' = 0: nothing reaches the forward's activations or z
        return u2.view(ctx.gshape), None, None, None, gw1, gw2, None, None, None


def _chain_act_ok(act_name) -> bool:
    """relu / leaky in every order; sigmoid / tanh outside ``second_order_forward()`` only (the chains' second order is the
    masked form, act'' = 0)."""
    return act_name in _HEAD_ACTS and not (_HEAD_ACTS[act_name] in _SMOOTH_ACT_FNS and in_second_order_forward())


def node_embed_supported(z, l1, l2, act_name) -> bool:
    return (z.is_cuda and z.dtype == torch.float32 and _chain_act_ok(act_name) and 1 <= z.shape[-1] <= 255
            and tuple(l1.weight.shape) == (64, z.shape[-1]) and tuple(l2.weight.shape) == (128, 64)
            and l1.bias is not None and l2.bias is not None and l1.weight.dtype == torch.float32)


def node_embed(z, l1, l2, act_name):
    """act(Linear(64, 128)(act(Linear(E, 64)(z)))) over the last dimension of ``z``: float32 [..., 128]."""
    return _NodeEmbed.apply(z, l1.weight, l1.bias, l2.weight, l2.bias, _HEAD_ACTS[act_name])


class _HeadTail(Function):
    """Tail of the Discriminator head after its first Linear (reference models.py:173-178, 207): act - Linear(64, 32) - act -
    Linear(32, 16) - act - Linear(16, 1) over the rows of ``z1`` as ONE launch (dg_head_chain); the backward is one launch
    for the input gradient (dg_head_bwd) and one for the six parameter gradients (dg_head_wgrad), itself differentiable
    (``_HeadTailBwd``: the gradient penalty's second order is the same chain kernel with the activation pattern as a mask;
    sigmoid / tanh, act'' != 0: the composite graph)."""

    @staticmethod
    def forward(ctx, z1, w2, b2, w3, b3, w4, b4, act):
        z_in, z1 = z1, _c(z1)
        R = z1.shape[0]
        dev = z1.device
        a1, a2, a3 = (torch.empty(R, n, dtype=torch.float32, device=dev) for n in (64, 32, 16))
        out = torch.empty(R, 1, dtype=torch.float32, device=dev)
        _lib.launch("dg_head_chain", z1, _lib.ptr(z1), None, None, None, _lib.fptr(_c(w2)), _lib.fptr(_c(b2)),
                    _lib.fptr(_c(w3)), _lib.fptr(_c(b3)), _lib.fptr(_c(w4)), _lib.fptr(_c(b4)), _lib.ptr(a1), _lib.ptr(a2),
                    _lib.ptr(a3), _lib.ptr(out), R, act)
        ctx.save_for_backward(a1, a2, a3, w2, w3, w4, *((z_in, b2, b3, b4) if act in _SMOOTH_ACT_FNS else ()))
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, g_out):
        a1, a2, a3, w2, w3, w4 = ctx.saved_tensors[:6]
        if ctx.act in _SMOOTH_ACT_FNS and torch.is_grad_enabled():
            z1, b2, b3, b4 = ctx.saved_tensors[6:]
            act = ctx.act
            return _double_backward_fallback(lambda *t: _composite_head_tail(*t, act), (z1, w2, b2, w3, b3, w4, b4),
                                             g_out) + (None,)
        need_w = any(ctx.needs_input_grad[1:7]) and not _inputs_only()
        g1, dw2, db2, dw3, db3, dw4, db4 = _HeadTailBwd.apply(g_out, a1, a2, a3, w2, w3, w4, need_w, ctx.act)
        return g1, dw2, db2, dw3, db3, dw4, db4, None


class _HeadTailBwd(Function):
    @staticmethod
    def forward(ctx, g_out, a1, a2, a3, w2, w3, w4, need_w, act):
        g_out = _c(g_out.float()).reshape(-1, 1)
        R = a1.shape[0]
        dev = a1.device
        g3, g2, g1 = (torch.empty(R, n, dtype=torch.float32, device=dev) for n in (16, 32, 64))
        dws = [None] * 6
        _lib.launch("dg_head_bwd", a1, _lib.ptr(g_out), _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(a3), _lib.fptr(_c(w2)),
                    _lib.fptr(_c(w3)), _lib.fptr(_c(w4)), _lib.ptr(g3), _lib.ptr(g2), _lib.ptr(g1), R, act)
        if need_w:
            dw2, dw3, dw4 = torch.empty_like(w2), torch.empty_like(w3), torch.empty_like(w4)
            db2, db3, db4 = (torch.empty(n, dtype=torch.float32, device=dev) for n in (32, 16, 1))
            _lib.launch("dg_head_wgrad", a1, _lib.ptr(g_out), _lib.ptr(a3), _lib.ptr(g3), _lib.ptr(a2), _lib.ptr(g2),
                        _lib.ptr(a1), _lib.ptr(dw4), _lib.ptr(db4), _lib.ptr(dw3), _lib.ptr(db3), _lib.ptr(dw2),
                        _lib.ptr(db2), R)
            dws = [dw2, db2, dw3, db3, dw4, db4]
        ctx.save_for_backward(g_out, a1, a2, a3, w2, w3, w4, g2, g3)
        ctx.act = act
        ctx.set_materialize_grads(False)
        return (g1, *dws)

    @staticmethod
    @once_differentiable
    def backward(ctx, t1, *tw):
        if any(t is not None for t in tw):
            raise RuntimeError("head_tail: second-order terms through parameter gradients are not implemented")
        if t1 is None:
            return (None,) * 9
        g_out, a1, a2, a3, w2, w3, w4, g2, g3 = ctx.saved_tensors
        t1 = _c(t1.float())
        R = a1.shape[0]
        dev = a1.device
        u1, u2, u3 = (torch.empty(R, n, dtype=torch.float32, device=dev) for n in (64, 32, 16))
        uo = torch.empty(R, 1, dtype=torch.float32, device=dev)
        gw2 = gw3 = gw4 = None
        _lib.launch("dg_head_chain", a1, _lib.ptr(t1), _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(a3), _lib.fptr(_c(w2)), None,
                    _lib.fptr(_c(w3)), None, _lib.fptr(_c(w4)), None, _lib.ptr(u1), _lib.ptr(u2), _lib.ptr(u3), _lib.ptr(uo),
                    R, ctx.act)
        if not _inputs_only():
            gw2, gw3, gw4 = torch.empty_like(w2), torch.empty_like(w3), torch.empty_like(w4)
            _lib.launch("dg_head_wgrad", a1, _lib.ptr(g_out), _lib.ptr(u3), _lib.ptr(g3), _lib.ptr(u2), _lib.ptr(g2),
                        _lib.ptr(u1), _lib.ptr(gw4), None, _lib.ptr(gw3), None, _lib.ptr(gw2), None, R)
        # act'' = 0: nothing reaches the forward's activations
        return uo, None, None, None, gw2, gw3, gw4, None, None


def head_tail_supported(z1, layers, act_name) -> bool:
    """``layers`` = the three Linears after the head's first one."""
    return (z1.is_cuda and z1.dtype == torch.float32 and z1.dim() == 2 and _chain_act_ok(act_name)
            and [tuple(l.weight.shape) for l in layers] == [(32, 64), (16, 32), (1, 16)]
            and all(l.bias is not None and l.weight.dtype == torch.float32 for l in layers))


def head_tail(z1, layers, act_name):
    """act(z1) -> Linear(64, 32) -> act -> Linear(32, 16) -> act -> Linear(16, 1): [R, 64] -> [R, 1]."""
    l2, l3, l4 = layers
    return _HeadTail.apply(z1, l2.weight, l2.bias, l3.weight, l3.bias, l4.weight, l4.bias, _HEAD_ACTS[act_name])


def readout(x, weight, bias=None):
    """float32 ``F.linear(x.float(), weight, bias)`` for the Generator's readouts (dim 128 -> edge / node classes)."""
    ok = (x.is_cuda and x.dtype in _lib.DTYPES and weight.dim() == 2 and weight.shape[1] == 128 and 1 <= weight.shape[0] <= 255
          and weight.dtype == torch.float32)
    if not ok:
        return linear(x.float(), weight, bias)
    return _Readout.apply(x, weight, bias)
