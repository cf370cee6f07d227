"""Sigmoid / tanh on the HIP path: the second order of the edge embedding (csrc/embed_sym_smooth.hip,
dg_embed_sym_bwd2_smooth), its autograd route, and the first order of the node / head chain kernels.

The reference is torch float64 autograd of Linear - act - Linear - act - symmetrise on the CPU, on the float32-valued
inputs the kernel gets.  Second-order outputs are held to 2e-4 relative L2 per tensor, the bar test_embed_sym_all_orders
holds this kernel family's second order to; no row is left out (smooth activations have no kinks).  Beside every measured
error the test prints the error of the same composite evaluated by torch in float32 on the CPU.

Measured on MI355X, worst case per tensor over the eight cases of each activation (relative L2 against float64; in
brackets float32 torch on the CPU):
    tanh      gg 2.6e-7 (2.6e-7)  ga 4.6e-5 (4.9e-7)  gw1 2.8e-5 (1.1e-6)  gb1 3.4e-5 (5.0e-7)  gw2 2.9e-5 (3.9e-7)  gb2 3.5e-7 (4.0e-7)
    sigmoid   gg 2.8e-7 (2.9e-7)  ga 3.0e-5 (6.9e-7)  gw1 2.8e-5 (1.3e-6)  gb1 2.8e-5 (6.0e-7)  gw2 2.8e-5 (3.4e-7)  gb2 3.3e-7 (3.4e-7)
gg and gb2 pass only the layer-2 recomputation (six bf16 cross products per fp32 product).  ga, gw1, gb1 and gw2 pass the
gradient stages dh_stage / aw2_stage, which take the three leading cross products (2^-16 of a product left out: DESIGN
3.16): 2.6e-5, the figure dg_embed_sym_bwd's da, dw1, db1, dw2 have on the same inputs (2.4e-5 .. 2.8e-5).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

F = torch.nn.functional
TOL2 = 2e-4          # second order of the embedding kernels against float64 (test_embed_sym_all_orders)
TOL = 2e-5           # chain kernels, forward and first order (test_discriminator_head_tail_all_orders)
TOL_IO = 4e-3        # one bf16 store (tests/test_hip_bf16.py)
ACT_ID = {"relu": 0, "leaky": 1, "sigmoid": 2, "tanh": 3}
ACT_FN = {"sigmoid": torch.sigmoid, "tanh": torch.tanh}
E_ARG, E_WORKSPACE = -2, -3
GUARD = 256
SENTINEL = 12345.0
NAMES = "gg ga gw1 gb1 gw2 gb2".split()

# (B, N, E, scale of a): one diagonal pair in a padded tile; 3 pairs; 21 pairs of three molecules; two tiles, the second
# partial, EP = 8 full; EP = 16; kMaxE; the headline geometry (33 tiles per molecule); saturated units
SHAPES = [(1, 1, 3, 1.0), (2, 2, 5, 1.0), (3, 6, 5, 1.0), (2, 9, 8, 1.0), (1, 9, 9, 1.0), (1, 8, 16, 1.0), (2, 45, 5, 1.0),
          (2, 9, 5, 6.0)]


def _lib():
    from druggen_amd import _lib as lib
    return lib


def _gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float()


def _rel(got, want):
    want = want.double().cpu()
    den = want.norm().item()
    return (got.double().cpu() - want).norm().item() / (den if den > 0 else 1.0)


def _p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def _inputs(B, N, E, scale):
    """a, w1, b1, w2, b2, g, t: CPU float32, scaled as in test_embed_sym_all_orders, never written afterwards."""
    return (_gen((B, N, N, E), 1, scale), _gen((64, E), 2, 0.5), _gen((64,), 3, 0.3), _gen((128, 64), 4, 0.2),
            _gen((128,), 5, 0.3), _gen((B, N, N, 128), 6), _gen((B, N, N, E), 7))


def _second_order(ins, act, dtype):
    """gg, ga, gw1, gb1, gw2, gb2 of <t, d out / d a . g> by torch autograd on the CPU in ``dtype``."""
    f = ACT_FN[act]
    a, w1, b1, w2, b2, g = (x.to(dtype).requires_grad_(True) for x in ins[:6])
    t = ins[6].to(dtype)
    y = f(F.linear(f(F.linear(a, w1, b1)), w2, b2))
    out = (y + y.permute(0, 2, 1, 3)) / 2
    (da,) = torch.autograd.grad(out, a, g, create_graph=True)
    return [x.detach() for x in torch.autograd.grad((da * t).sum(), [g, a, w1, b1, w2, b2])]


@functools.lru_cache(maxsize=None)
def _reference(B, N, E, scale, act):
    ins = _inputs(B, N, E, scale)
    want = _second_order(ins, act, torch.float64)
    torch32 = [_rel(x, y) for x, y in zip(_second_order(ins, act, torch.float32), want)]
    return want, torch32


def _guarded(shape, dtype=torch.float32):
    """A NaN-filled tensor of ``shape`` with GUARD sentinel elements behind it in the same allocation."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")
    buf[n:] = SENTINEL
    return buf[:n].view(shape), buf[n:]


class _Call:
    """Device operands of one case and one call of dg_embed_sym_bwd2_smooth through ``_lib``."""

    def __init__(self, B, N, E, scale, act, odt=torch.float32):
        from druggen_amd import functional as dgf
        self.B, self.N, self.E, self.act = B, N, E, ACT_ID[act]
        self.lib = _lib().load()
        a, w1, b1, w2, b2, g, t = (x.cuda() for x in _inputs(B, N, E, scale))
        self.a, self.w1, self.b1, self.w2, self.b2, self.t = a, w1, b1, w2, b2, t
        self.g = g.to(odt)
        self.w2p, self.w2d = dgf._embed_packed_w2(w2), dgf._embed_packed_w2(w2, True)
        self.ws = torch.empty(int(self.lib.dg_embed_sym_workspace_bytes(B, N)), dtype=torch.uint8, device="cuda")

    def run(self, want_ga=True, want_w=True, act=None, ws_bytes=None, drop=None):
        """-> (status, [gg, ga, gw1, gb1, gw2, gb2], guards of gg and ga).  ``drop``: one weight output passed as NULL."""
        gg, guard_gg = _guarded(self.g.shape, self.g.dtype)
        ga, guard_ga = _guarded(self.a.shape) if want_ga else (None, None)
        gw = [torch.full_like(x, float("nan")) if want_w else None for x in (self.w1, self.b1, self.w2, self.b2)]
        if drop is not None:
            gw[drop] = None
        ws = self.ws if want_w else None
        st = self.lib.dg_embed_sym_bwd2_smooth(
            _p(self.a), _p(self.w1), _p(self.b1), _p(self.w2p), _p(self.w2d), _p(self.b2), _p(self.g), _p(self.t), _p(gg),
            _p(ga), *[_p(x) for x in gw], _p(ws), (self.ws.numel() if ws_bytes is None else ws_bytes) if want_w else 0,
            self.B, self.N, self.E, 64, 128, self.act if act is None else act, _lib().dt(self.g), None)
        torch.cuda.synchronize()
        return st, [gg, ga] + gw, (guard_gg, guard_ga)


@functools.lru_cache(maxsize=None)
def _full(B, N, E, scale, act):
    call = _Call(B, N, E, scale, act)
    st, outs, guards = call.run()
    assert st == 0, (st, call.lib.dg_last_error_string())
    return call, outs, guards


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("B,N,E,scale", SHAPES)
def test_every_output_against_float64(B, N, E, scale, act):
    want, torch32 = _reference(B, N, E, scale, act)
    _, outs, _ = _full(B, N, E, scale, act)
    errs = [_rel(x, y) for x, y in zip(outs, want)]
    print(f"\nembed_smooth {act} B={B} N={N} E={E} a*{scale:g}: "
          + "  ".join(f"{n} {e:.2e} (torch32 {r:.2e})" for n, e, r in zip(NAMES, errs, torch32)))
    for name, err in zip(NAMES, errs):
        assert err < TOL2, (name, err)


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("B,N,E,scale", SHAPES)
def test_every_row_written_once_nothing_else(B, N, E, scale, act):
    """gg and ga start as NaN with sentinels behind them: every element ends finite, the sentinels stay, and the diagonal
    rows (i, i) -- one pair held by both halves of its tile with half weight -- agree with the reference by absolute
    error: 2e-4 of the largest reference magnitude on those rows, where a half counted once or twice would be off by half
    of it or all of it."""
    want, _ = _reference(B, N, E, scale, act)
    _, outs, guards = _full(B, N, E, scale, act)
    idx = torch.arange(N)
    for name, got, ref, guard in zip(NAMES[:2], outs[:2], want[:2], guards):
        assert torch.isfinite(got).all(), name
        assert (guard == SENTINEL).all(), name
        d_got, d_ref = got[:, idx, idx].double().cpu(), ref[:, idx, idx]
        assert (d_got - d_ref).abs().max().item() <= TOL2 * d_ref.abs().max().item(), name
    for name, got in zip(NAMES[2:], outs[2:]):
        assert torch.isfinite(got).all(), name


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("B,N,E,scale", [(1, 1, 3, 1.0), (2, 9, 8, 1.0), (1, 9, 9, 1.0), (2, 45, 5, 1.0)])
def test_null_outputs_leave_the_rest_bit_identical(B, N, E, scale, act):
    call, full, _ = _full(B, N, E, scale, act)
    for want_ga, want_w in ((False, True), (True, False), (False, False)):
        st, outs, guards = call.run(want_ga, want_w)
        assert st == 0, call.lib.dg_last_error_string()
        for name, got, ref in zip(NAMES, outs, full):
            if got is not None:
                assert torch.equal(got, ref), (name, want_ga, want_w)
        assert (guards[0] == SENTINEL).all()


def test_refusals_before_any_launch():
    call = _Call(2, 9, 5, 1.0, "tanh")
    lib = call.lib

    def untouched(outs):
        return all(x is None or torch.isnan(x).all() for x in outs)

    for act in (0, 1):      # relu / leaky have dg_embed_sym_bwd2
        st, outs, _ = call.run(act=act)
        assert st == E_ARG and b"smooth" in lib.dg_last_error_string() and untouched(outs)
    st, outs, _ = call.run(ws_bytes=call.ws.numel() - 1)
    assert st == E_WORKSPACE and b"workspace" in lib.dg_last_error_string() and untouched(outs)
    for drop in range(4):      # gw1, gb1, gw2, gb2: all or none
        st, outs, _ = call.run(drop=drop)
        assert st == E_ARG and b"all given or all NULL" in lib.dg_last_error_string() and untouched(outs)
    st, outs, _ = call.run()
    assert st == 0 and all(torch.isfinite(x).all() for x in outs)


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("B,N,E", [(2, 9, 5), (1, 9, 9)])
def test_bf16_gradient_matches_the_float32_instance(B, N, E, act):
    """As test_embed_sym_bf16_output_matches_fp32_kernel: with one bf16-valued upstream gradient the float32 outputs of the
    bf16 instance agree with the float32 instance's to 1e-4 (same arithmetic on the same values), gg to one bf16 store."""
    c16 = _Call(B, N, E, 1.0, act, torch.bfloat16)
    c32 = _Call(B, N, E, 1.0, act)
    c32.g = c16.g.float()
    st16, o16, g16 = c16.run()
    st32, o32, _ = c32.run()
    assert st16 == 0 and st32 == 0
    assert o16[0].dtype == torch.bfloat16 and torch.isfinite(o16[0].float()).all() and (g16[0] == SENTINEL).all()
    assert _rel(o16[0], o32[0]) < TOL_IO
    for name, x16, x32 in zip(NAMES[1:], o16[1:], o32[1:]):
        assert _rel(x16, x32) < 1e-4, name


def test_penalty_pattern_through_autograd():
    """dgf.embed_sym under second_order_forward() / inputs_only_backward(), tanh: the parameters' and the upstream
    gradient's adjoints against float64, two runs bit for bit, and the launches are the library's (the composite route
    counts none under "embed_sym")."""
    from druggen_amd import functional as dgf
    B, N, E, act = 2, 9, 5, "tanh"
    ins = _inputs(B, N, E, 1.0)
    want, _ = _reference(B, N, E, 1.0, act)      # gg, ga, gw1, gb1, gw2, gb2
    L = _lib()

    def run():
        a, w1, b1, w2, b2, g = (x.cuda().requires_grad_(True) for x in ins[:6])
        t = ins[6].cuda()
        with dgf.second_order_forward():
            out = dgf.embed_sym(a, w1, b1, w2, b2, act)
        with dgf.inputs_only_backward():
            (da,) = torch.autograd.grad(out, a, g, create_graph=True)
        return torch.autograd.grad((da * t).sum(), [g, a, w1, b1, w2, b2])

    L.prof_reset()
    L.prof_enable(True, kernels=["embed_sym"])
    try:
        got = run()
        torch.cuda.synchronize()
        launches = L.prof_read("embed_sym")[0]
    finally:
        L.prof_enable(False)
        L.prof_reset()
    assert launches >= 3, launches      # forward, first backward, second order
    for name, x, y in zip(NAMES, got, want):
        assert _rel(x, y) < TOL2, name
    again = run()
    assert all(torch.equal(x, y) for x, y in zip(got, again))


# ------------------------------------------------------------------------------------------------ the two small chains
def _head(act):
    import torch.nn as nn
    mk = {"tanh": nn.Tanh, "sigmoid": nn.Sigmoid}[act]
    torch.manual_seed(3)
    ref = nn.Sequential(mk(), nn.Linear(64, 32), mk(), nn.Linear(32, 16), mk(), nn.Linear(16, 1)).double()
    lay = [nn.Linear(64, 32), nn.Linear(32, 16), nn.Linear(16, 1)]
    for l, i in zip(lay, (1, 3, 5)):
        l.weight.data.copy_(ref[i].weight.data.float())
        l.bias.data.copy_(ref[i].bias.data.float())
        ref[i].weight.data.copy_(l.weight.data.double())
        ref[i].bias.data.copy_(l.bias.data.double())
        l.cuda()
    return ref, lay


def _node(act, E):
    import torch.nn as nn
    mk = {"tanh": nn.Tanh, "sigmoid": nn.Sigmoid}[act]
    torch.manual_seed(5)
    l1, l2 = nn.Linear(E, 64), nn.Linear(64, 128)
    ref = nn.Sequential(nn.Linear(E, 64), mk(), nn.Linear(64, 128), mk()).double()
    for l, i in ((l1, 0), (l2, 2)):
        ref[i].weight.data.copy_(l.weight.data.double())
        ref[i].bias.data.copy_(l.bias.data.double())
        l.cuda()
    return ref, l1, l2


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_chains_support_smooth_activations_in_first_order_only(act):
    from druggen_amd import functional as dgf
    _, lay = _head(act)
    _, l1, l2 = _node(act, 5)
    z1, z = torch.zeros(4, 64, device="cuda"), torch.zeros(2, 3, 5, device="cuda")
    assert dgf.head_tail_supported(z1, lay, act) and dgf.node_embed_supported(z, l1, l2, act)
    with dgf.second_order_forward():
        assert not dgf.head_tail_supported(z1, lay, act) and not dgf.node_embed_supported(z, l1, l2, act)
        assert dgf.head_tail_supported(z1, lay, "relu") and dgf.node_embed_supported(z, l1, l2, "leaky")
    assert dgf.head_tail_supported(z1, lay, act) and dgf.node_embed_supported(z, l1, l2, act)


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("R", [1, 5, 64, 300])
def test_head_tail_forward_and_first_order(R, act):
    from druggen_amd import functional as dgf
    ref, lay = _head(act)
    z, up = _gen((R, 64), 600 + R), _gen((R, 1), 601 + R)
    zc, zd = z.cuda().requires_grad_(True), z.double().requires_grad_(True)
    out, outd = dgf.head_tail(zc, lay, act), ref(zd)
    assert out.grad_fn is not None and "HeadTail" in type(out.grad_fn).__name__
    assert _rel(out.detach(), outd.detach()) < TOL
    params = [p for l in lay for p in (l.weight, l.bias)]
    paramsd = [p for i in (1, 3, 5) for p in (ref[i].weight, ref[i].bias)]
    got = torch.autograd.grad(out, [zc] + params, up.cuda())
    want = torch.autograd.grad(outd, [zd] + paramsd, up.double())
    for x, y in zip(got, want):
        assert _rel(x, y) < TOL
    out2 = dgf.head_tail(zc, lay, act)
    assert torch.equal(out, out2) and all(torch.equal(x, y) for x, y in zip(got, torch.autograd.grad(out2, [zc] + params, up.cuda())))


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("R", [1, 5, 64, 300])
def test_node_embed_forward_and_first_order(R, act):
    from druggen_amd import functional as dgf
    E = 13 if R == 64 else 5
    ref, l1, l2 = _node(act, E)
    z, up = _gen((R, E), 700 + R), _gen((R, 128), 701 + R)
    zc, zd = z.cuda().requires_grad_(True), z.double().requires_grad_(True)
    out, outd = dgf.node_embed(zc, l1, l2, act), ref(zd)
    assert "NodeEmbed" in type(out.grad_fn).__name__
    assert out.shape == (R, 128) and _rel(out.detach(), outd.detach()) < TOL
    params = [l1.weight, l1.bias, l2.weight, l2.bias]
    paramsd = [ref[0].weight, ref[0].bias, ref[2].weight, ref[2].bias]
    got = torch.autograd.grad(out, [zc] + params, up.cuda())
    want = torch.autograd.grad(outd, [zd] + paramsd, up.double())
    for x, y in zip(got, want):
        assert _rel(x, y) < TOL
    assert torch.equal(out, dgf.node_embed(zc, l1, l2, act))


def test_masked_chain_calls_refuse_smooth_activations():
    """The second-order form of the chain kernels is "the same chain with a mask" only for act'' = 0."""
    lib = _lib().load()
    x = torch.zeros(4 * 128, device="cuda")
    p = x.data_ptr()
    for act in (2, 3):
        assert lib.dg_embed_node_chain(p, p, p, p, None, p, None, p, p, 4, 5, act, None) == E_ARG
        assert b"second-order" in lib.dg_last_error_string()
        assert lib.dg_head_chain(p, p, p, p, p, None, p, None, p, None, p, p, p, p, 4, act, None) == E_ARG
        assert b"second-order" in lib.dg_last_error_string()
    assert lib.dg_embed_node_chain(p, None, None, p, p, p, p, p, p, 4, 5, 4, None) == E_ARG      # no such activation
    assert lib.dg_head_bwd(p, p, p, p, p, p, p, p, p, p, 4, 4, None) == E_ARG


@pytest.mark.parametrize("chain", ["node", "head"])
def test_create_graph_backward_through_a_chain_takes_the_composite(chain):
    """A forward outside second_order_forward() that is differentiated twice after all: the backward under grad mode
    rebuilds the composite, and the penalty pattern matches float64 (the bars of the relu tests of both chains)."""
    from druggen_amd import functional as dgf
    act, R = "tanh", 37
    if chain == "node":
        ref, l1, l2 = _node(act, 5)
        z, up = _gen((R, 5), 800), _gen((R, 128), 801)
        fwd = lambda zc: dgf.node_embed(zc, l1, l2, act)
        ws, wsd = [l1.weight, l2.weight], [ref[0].weight, ref[2].weight]
    else:
        ref, lay = _head(act)
        z, up = _gen((R, 64), 802), torch.ones(R, 1)
        fwd = lambda zc: dgf.head_tail(zc, lay, act)
        ws, wsd = [l.weight for l in lay], [ref[i].weight for i in (1, 3, 5)]
    zc, zd = z.cuda().requires_grad_(True), z.double().requires_grad_(True)
    (gz,) = torch.autograd.grad(fwd(zc), zc, up.cuda(), create_graph=True)
    (gzd,) = torch.autograd.grad(ref(zd), zd, up.double(), create_graph=True)
    assert _rel(gz.detach(), gzd.detach()) < TOL
    pen, pend = ((gz.norm(dim=-1) - 1) ** 2).mean(), ((gzd.norm(dim=-1) - 1) ** 2).mean()
    assert abs(pen.item() - pend.item()) < 1e-4 * max(1.0, abs(pend.item()))
    for x, y in zip(torch.autograd.grad(pen, ws + [zc]), torch.autograd.grad(pend, wsd + [zd])):
        assert _rel(x, y) < 5e-5
