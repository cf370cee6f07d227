"""The node-side layers of a --features model on their HIP kernels (csrc/node_wide.hip, include/druggen_hip.h,
functional/heads.py): the node embedding chain for input widths 17..255 in every order the narrow chain serves, its first
Linear's weight gradient, and the node readout for 17..255 classes -- against the narrow kernels bit for bit where both run,
against float64 on the CPU elsewhere, through the autograd nodes and through one whole GAN step."""

import numpy as np
import pytest
import torch

import harness
from oracle import druggen_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 2e-5      # fp32 kernels vs fp64 closed form, relative L2: the bar of tests/test_hip_kernels.py
ACTS = {"relu": 0, "leaky": 1, "sigmoid": 2, "tanh": 3}


def _rel(got, want):
    want = want.double()
    den = want.norm().item()
    return (got.double().cpu() - want).norm().item() / (den if den > 0 else 1.0)


def _gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _features_rows(shape, seed):
    """0 / 1 rows as a --features store makes them: a one-hot prefix (up to 13 atom types), then coins; the last row all ones
    behind the prefix."""
    E = shape[-1]
    A = min(13, max(1, E - 1))
    rng = np.random.default_rng([seed, E])
    x = np.zeros(shape, dtype=np.float64)
    np.put_along_axis(x, rng.integers(0, A, size=shape[:-1] + (1,)), 1.0, axis=-1)
    x[..., A:] = rng.integers(0, 2, size=shape[:-1] + (E - A,))
    x.reshape(-1, E)[-1, A:] = 1.0
    return torch.from_numpy(x)


def _lib():
    from druggen_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------------------------------------------------------
# bit identity with the narrow kernels where both run
# --------------------------------------------------------------------------------------------------------------------------
def _chain_operands(R, E, seed):
    f = lambda shape, k, s=1.0: (_gen(shape, seed + k) * s).float().cuda()
    return dict(z=f((R, E), 0), w1=f((64, E), 1, 0.4), b1=f((64,), 2, 0.3), w2=f((128, 64), 3, 0.2), b2=f((128,), 4, 0.3),
                g=f((R, 128), 5), t=f((R, E), 6))


def _raw_chain(entry, inp, m1, m2, o, R, E, act):
    o1 = torch.full((R, 64), float("nan"), device="cuda")
    o2 = torch.full((R, 128), float("nan"), device="cuda")
    bias = (None, None) if m1 is not None else (o["b1"], o["b2"])
    st = getattr(_lib().load(), entry)(_p(inp), _p(m1), _p(m2), _p(o["w1"]), _p(bias[0]), _p(o["w2"]), _p(bias[1]), _p(o1), _p(o2),
                                       R, E, act, _stream())
    assert st == 0, _lib().load().dg_last_error_string()
    return o1, o2


def _raw_bwd(entry, o, a1, a2, R, E, act, want_dz=True):
    g2 = torch.full((R, 128), float("nan"), device="cuda")
    g1 = torch.full((R, 64), float("nan"), device="cuda")
    dz = torch.full((R, E), float("nan"), device="cuda") if want_dz else None
    st = getattr(_lib().load(), entry)(_p(o["g"]), _p(a1), _p(a2), _p(o["w1"]), _p(o["w2"]), _p(g2), _p(g1), _p(dz), R, E, act,
                                       _stream())
    assert st == 0, _lib().load().dg_last_error_string()
    return g2, g1, dz


@pytest.mark.parametrize("R", [1, 33])
@pytest.mark.parametrize("E", [1, 5, 16])
def test_wide_entries_equal_the_narrow_ones_bit_for_bit(E, R):
    """Same summation order (bias first, one accumulator per output, ascending inputs, fmaf; the padding adds fmaf(0, 0, acc)):
    the forward for all four activations, the masked second-order form for relu / leaky, the backward with and without dz."""
    o = _chain_operands(R, E, 40 + E + R)
    for act in range(4):
        n1, n2 = _raw_chain("dg_embed_node_chain", o["z"], None, None, o, R, E, act)
        w1, w2 = _raw_chain("dg_embed_node_wide_chain", o["z"], None, None, o, R, E, act)
        assert torch.isfinite(n2).all() and torch.equal(n1, w1) and torch.equal(n2, w2), act
        if act < 2:
            nu = _raw_chain("dg_embed_node_chain", o["t"], n1, n2, o, R, E, act)
            wu = _raw_chain("dg_embed_node_wide_chain", o["t"], n1, n2, o, R, E, act)
            assert torch.isfinite(nu[1]).all() and torch.equal(nu[0], wu[0]) and torch.equal(nu[1], wu[1]), act
        for want_dz in (True, False):
            nb = _raw_bwd("dg_embed_node_bwd", o, n1, n2, R, E, act, want_dz)
            wb = _raw_bwd("dg_embed_node_wide_bwd", o, n1, n2, R, E, act, want_dz)
            for a_, b_ in zip(nb, wb):
                assert (a_ is None and b_ is None) or (torch.isfinite(a_).all() and torch.equal(a_, b_)), (act, want_dz)


# --------------------------------------------------------------------------------------------------------------------------
# the chain through its autograd nodes against nn.Sequential in float64
# --------------------------------------------------------------------------------------------------------------------------
# (E, B, N): every E of the issue and R = B N in {1, 31, 32, 33, 300} -- one below, at and one above the 32-row tile and several
# tiles -- each at least once; E = 31, 32, 33 and 255 sit at the slab edges of layer 1 (32 columns) and of dz (128 columns)
CHAIN_SHAPES = [(17, 1, 1), (17, 4, 75), (31, 3, 11), (32, 2, 16), (33, 1, 31), (67, 4, 75), (255, 3, 11), (129, 1, 31)]


@pytest.mark.parametrize("kind", ["randn", "features"])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("E,B,N", CHAIN_SHAPES)
def test_wide_node_embedding_all_orders(E, B, N, act, kind):
    """tests/test_hip_kernels.py::test_node_embedding_all_orders at E > 16, with its bars: output, dz and the four parameter
    gradients at TOL for all four activations; for relu / leaky the gradient-penalty pattern -- ((|d out / d z| - 1)^2).mean() to
    1e-4 max(1, |.|), its gradients with respect to both weights to 5e-5.  (Plain float32 torch on these shapes and inputs stays
    at or below 8e-7 in every quantity: float32 against float64 alone is inside the bars with a factor of 25 to spare.)"""
    import torch.nn as nn
    from druggen_amd import functional as dgf
    torch.manual_seed(11 + B + E)
    mk = {"relu": nn.ReLU, "leaky": nn.LeakyReLU, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh}[act]
    l1, l2 = nn.Linear(E, 64), nn.Linear(64, 128)
    ref = nn.Sequential(nn.Linear(E, 64), mk(), nn.Linear(64, 128), mk()).double()
    for l, i in ((l1, 0), (l2, 2)):
        ref[i].weight.data.copy_(l.weight.data.double())
        ref[i].bias.data.copy_(l.bias.data.double())
        l.cuda()
    z = (_gen((B, N, E), 700 + B) if kind == "randn" else _features_rows((B, N, E), 700 + B)).float()
    up = _gen((B, N, 128), 701 + B).float()
    zc, zd = z.cuda().requires_grad_(True), z.double().requires_grad_(True)
    assert dgf.node_embed_supported(zc, l1, l2, act)
    out, outd = dgf.node_embed(zc, l1, l2, act), ref(zd)
    assert type(out.grad_fn).__name__.startswith("_NodeEmbed")
    errs = {"out": _rel(out.detach(), outd.detach())}
    assert out.shape == (B, N, 128)
    params = [l1.weight, l1.bias, l2.weight, l2.bias]
    paramsd = [ref[0].weight, ref[0].bias, ref[2].weight, ref[2].bias]
    got = torch.autograd.grad(out, [zc] + params, up.cuda(), retain_graph=True)
    want = torch.autograd.grad(outd, [zd] + paramsd, up.double(), retain_graph=True)
    for name, a_, b_ in zip(("dz", "dw1", "db1", "dw2", "db2"), got, want):
        errs[name] = _rel(a_, b_)
    print(E, B, N, act, kind, " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), errs
    out2 = dgf.node_embed(zc, l1, l2, act)
    got_again = torch.autograd.grad(out2, [zc] + params, up.cuda())
    assert torch.equal(out, out2) and all(torch.equal(a_, b_) for a_, b_ in zip(got, got_again))
    if act not in ("relu", "leaky"):
        return
    with dgf.second_order_forward():
        out = dgf.node_embed(zc, l1, l2, act)
    with dgf.inputs_only_backward():
        (gz,) = torch.autograd.grad(out, zc, up.cuda(), create_graph=True)
    (gzd,) = torch.autograd.grad(outd, zd, up.double(), create_graph=True)
    pen, pend = ((gz.norm(dim=-1) - 1) ** 2).mean(), ((gzd.norm(dim=-1) - 1) ** 2).mean()
    print("  penalty", pen.item(), pend.item())
    assert abs(pen.item() - pend.item()) < 1e-4 * max(1.0, abs(pend.item()))
    got2 = torch.autograd.grad(pen, [l1.weight, l2.weight])
    want2 = torch.autograd.grad(pend, [ref[0].weight, ref[2].weight])
    e2 = [_rel(a_, b_) for a_, b_ in zip(got2, want2)]
    print("  penalty gradients", e2)
    assert all(e < 5e-5 for e in e2), e2


def test_wide_chain_routing():
    """E = 67 is served like E = 5: every activation outside second_order_forward(), relu / leaky inside it; sigmoid / tanh go
    to the composite there (as tests/test_hip_embed_smooth.py pins for the narrow chain); E = 256 is not served."""
    import torch.nn as nn
    from druggen_amd import functional as dgf
    for E in (5, 67, 255):
        l1, l2 = nn.Linear(E, 64).cuda(), nn.Linear(64, 128).cuda()
        z = torch.zeros(2, 3, E, device="cuda")
        for act in ACTS:
            assert dgf.node_embed_supported(z, l1, l2, act)
            with dgf.second_order_forward():
                assert dgf.node_embed_supported(z, l1, l2, act) == (act in ("relu", "leaky")), (E, act)
        assert not dgf.node_embed_supported(z.bfloat16(), l1, l2, "relu")
    l1, l2 = nn.Linear(256, 64).cuda(), nn.Linear(64, 128).cuda()
    assert not dgf.node_embed_supported(torch.zeros(2, 3, 256, device="cuda"), l1, l2, "relu")


def test_smooth_activations_take_the_composite_for_a_second_order_at_width_67():
    """tanh at E = 67 differentiated twice: the chain kernels run forward and the graph falls back to the composite, as at
    E <= 16; the penalty pattern against float64 at the bars of the piecewise-linear activations."""
    import torch.nn as nn
    from druggen_amd import functional as dgf
    torch.manual_seed(5)
    E, B, N = 67, 2, 17
    l1, l2 = nn.Linear(E, 64), nn.Linear(64, 128)
    ref = nn.Sequential(nn.Linear(E, 64), nn.Tanh(), nn.Linear(64, 128), nn.Tanh()).double()
    for l, i in ((l1, 0), (l2, 2)):
        ref[i].weight.data.copy_(l.weight.data.double())
        ref[i].bias.data.copy_(l.bias.data.double())
        l.cuda()
    z, up = _gen((B, N, E), 1).float(), _gen((B, N, 128), 2).float()
    zc, zd = z.cuda().requires_grad_(True), z.double().requires_grad_(True)
    out = dgf.node_embed(zc, l1, l2, "tanh")
    assert type(out.grad_fn).__name__.startswith("_NodeEmbed")
    (gz,) = torch.autograd.grad(out, zc, up.cuda(), create_graph=True)
    (gzd,) = torch.autograd.grad(ref(zd), zd, up.double(), create_graph=True)
    pen, pend = ((gz.norm(dim=-1) - 1) ** 2).mean(), ((gzd.norm(dim=-1) - 1) ** 2).mean()
    assert abs(pen.item() - pend.item()) < 1e-4 * max(1.0, abs(pend.item()))
    for a_, b_ in zip(torch.autograd.grad(pen, [l1.weight, l2.weight]), torch.autograd.grad(pend, [ref[0].weight, ref[2].weight])):
        assert _rel(a_, b_) < 5e-5


# --------------------------------------------------------------------------------------------------------------------------
# readout
# --------------------------------------------------------------------------------------------------------------------------
def _readout_case(rows, N, dtype, bias=True, seed=0):
    x0 = _gen((rows, 128), 1 + seed).to(dtype)
    w0, b0 = _gen((N, 128), 2 + seed) * 0.2, (_gen((N,), 3 + seed) if bias else None)
    dy = _gen((rows, N), 4 + seed)
    return x0, w0, b0, dy


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows", [1, 2, 3, 301])
@pytest.mark.parametrize("N", [17, 64, 67, 255])
def test_wide_readout_matches_linear_on_float32_logits(N, rows, dtype):
    """dgf.readout at 17..255 classes with the bars of test_skinny_readout_matches_linear_on_float32_logits: float32 logits from
    float32 or bf16 activations; y, dw, db at TOL, dx at TOL (float32) or 4e-3 (bf16 store), against F.linear in float64 on the
    same (already rounded) activations."""
    from druggen_amd import functional as dgf
    x0, w0, b0, dy = _readout_case(rows, N, dtype)
    xr, wr, br = x0.double().requires_grad_(True), w0.double().requires_grad_(True), b0.double().requires_grad_(True)
    y_ref = torch.nn.functional.linear(xr, wr, br)
    g_ref = torch.autograd.grad(y_ref, [xr, wr, br], dy)
    xd = x0.cuda().requires_grad_(True)
    wd, bd = w0.float().cuda().requires_grad_(True), b0.float().cuda().requires_grad_(True)
    y = dgf.readout(xd, wd, bd)
    assert type(y.grad_fn).__name__.startswith("_Readout") and y.dtype == torch.float32 and y.shape == (rows, N)
    gx, gw, gb = torch.autograd.grad(y, [xd, wd, bd], dy.float().cuda())
    assert gx.dtype == dtype
    errs = dict(y=_rel(y.detach(), y_ref.detach()), dx=_rel(gx.float(), g_ref[0]), dw=_rel(gw, g_ref[1]), db=_rel(gb, g_ref[2]))
    print(N, rows, dtype, errs)
    assert errs["y"] < TOL and errs["dw"] < TOL and errs["db"] < TOL
    assert errs["dx"] < (TOL if dtype == torch.float32 else 4e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_readout_without_bias_and_over_leading_dimensions(dtype):
    from druggen_amd import functional as dgf
    N = 67
    x0, w0, _, dy = _readout_case(2 * 3 * 7, N, dtype, bias=False, seed=10)
    x0, dy = x0.reshape(2, 3, 7, 128), dy.reshape(2, 3, 7, N)
    xr, wr = x0.double().requires_grad_(True), w0.double().requires_grad_(True)
    y_ref = torch.nn.functional.linear(xr, wr)
    g_ref = torch.autograd.grad(y_ref, [xr, wr], dy)
    xd, wd = x0.cuda().requires_grad_(True), w0.float().cuda().requires_grad_(True)
    y = dgf.readout(xd, wd)
    assert y.shape == (2, 3, 7, N) and _rel(y.detach(), y_ref.detach()) < TOL
    gx, gw = torch.autograd.grad(y, [xd, wd], dy.float().cuda())
    assert gx.shape == x0.shape and _rel(gx.float(), g_ref[0]) < (TOL if dtype == torch.float32 else 4e-3)
    assert _rel(gw, g_ref[1]) < TOL


def test_wide_readout_differentiated_again_takes_the_composite():
    """create_graph=True: the first backward is rebuilt from twice-differentiable pieces (``_double_backward_fallback``), as for
    the skinny readout; a function of dy/dx differentiated with respect to the weight, against float64."""
    from druggen_amd import functional as dgf
    N, rows = 67, 5
    x0, w0, b0, dy = _readout_case(rows, N, torch.float32, seed=20)
    xr, wr, br = x0.double().requires_grad_(True), w0.double().requires_grad_(True), b0.double().requires_grad_(True)
    (gr,) = torch.autograd.grad(torch.nn.functional.linear(xr, wr, br), xr, dy, create_graph=True)
    (want,) = torch.autograd.grad((gr ** 2).sum(), wr)
    xd = x0.float().cuda().requires_grad_(True)
    wd, bd = w0.float().cuda().requires_grad_(True), b0.float().cuda().requires_grad_(True)
    y = dgf.readout(xd, wd, bd)
    assert type(y.grad_fn).__name__.startswith("_Readout")
    (gx,) = torch.autograd.grad(y, xd, dy.float().cuda(), create_graph=True)
    assert gx.requires_grad and _rel(gx.detach(), gr.detach()) < TOL
    (got,) = torch.autograd.grad((gx ** 2).sum(), wd)
    assert _rel(got, want) < TOL


# --------------------------------------------------------------------------------------------------------------------------
# memory safety, reproducibility, capture: R = 33, E = 67, N = 67
# --------------------------------------------------------------------------------------------------------------------------
SENTINEL = 12345.0


class _Arena:
    """Outputs cut from the middle of sentinel-filled allocations, inputs from the middle of NaN-filled ones: a store outside an
    output shows as a changed sentinel, a load outside an input as a non-finite result."""
    PAD = 4096      # elements on each side (keeps every cut 16-byte aligned)

    def __init__(self):
        self.outs = []

    def inp(self, t):
        buf = torch.full((t.numel() + 2 * self.PAD,), float("nan"), dtype=t.dtype, device="cuda")
        cut = buf[self.PAD:self.PAD + t.numel()].view(t.shape)
        cut.copy_(t)
        return cut

    def out(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * self.PAD,), SENTINEL, dtype=dtype, device="cuda")
        self.outs.append((buf, n))
        return buf[self.PAD:self.PAD + n].view(shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.outs:
            assert (buf[:self.PAD] == SENTINEL).all() and (buf[self.PAD + n:] == SENTINEL).all()
            assert torch.isfinite(buf[self.PAD:self.PAD + n].float()).all()
            assert not (buf[self.PAD:self.PAD + n] == SENTINEL).all()


def _run_all_entries(R=33, E=67, N=67, seed=3, arena=None):
    """Every wide entry once on operands of its own; returns all outputs."""
    L, lib = _lib(), _lib().load()
    inp = arena.inp if arena else (lambda t: t)
    out = arena.out if arena else (lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda"))
    o = {k: inp(v) for k, v in _chain_operands(R, E, seed).items()}
    res = {}
    for act in (0, 3):
        a1, a2 = out((R, 64)), out((R, 128))
        assert lib.dg_embed_node_wide_chain(_p(o["z"]), None, None, _p(o["w1"]), _p(o["b1"]), _p(o["w2"]), _p(o["b2"]), _p(a1),
                                            _p(a2), R, E, act, _stream()) == 0
        g2, g1, dz = out((R, 128)), out((R, 64)), out((R, E))
        assert lib.dg_embed_node_wide_bwd(_p(o["g"]), _p(a1), _p(a2), _p(o["w1"]), _p(o["w2"]), _p(g2), _p(g1), _p(dz), R, E, act,
                                          _stream()) == 0
        res.update({f"a1_{act}": a1, f"a2_{act}": a2, f"g2_{act}": g2, f"g1_{act}": g1, f"dz_{act}": dz})
    u1, u2 = out((R, 64)), out((R, 128))
    assert lib.dg_embed_node_wide_chain(_p(o["t"]), _p(res["a1_0"]), _p(res["a2_0"]), _p(o["w1"]), None, _p(o["w2"]), None, _p(u1),
                                        _p(u2), R, E, 0, _stream()) == 0
    dw1, db1 = out((64, E)), out((64,))
    need = lib.dg_embed_node_wide_wgrad_workspace_bytes(R, E)
    ws = out((need // 4,))
    assert lib.dg_embed_node_wide_wgrad(_p(res["g1_0"]), _p(o["z"]), _p(dw1), _p(db1), _p(ws), need, R, E, _stream()) == 0
    res.update(u1=u1, u2=u2, dw1=dw1, db1=db1)
    for dtype in (torch.float32, torch.bfloat16):
        x0, w0, b0, dy0 = _readout_case(R, N, dtype, seed=seed)
        x, w, b, dy = inp(x0.cuda()), inp(w0.float().cuda()), inp(b0.float().cuda()), inp(dy0.float().cuda())
        code = L.DTYPES[dtype]
        y, dx, dw, db = out((R, N)), out((R, 128), dtype), out((N, 128)), out((N,))
        assert lib.dg_wide_linear_fwd(_p(x), _p(w), _p(b), _p(y), R, N, 128, code, _stream()) == 0
        assert lib.dg_wide_linear_dgrad(_p(dy), _p(w), _p(dx), R, N, 128, code, _stream()) == 0
        need = lib.dg_wide_linear_wgrad_workspace_bytes(R, N, 128)
        ws = out((need // 4,))
        assert lib.dg_wide_linear_wgrad(_p(dy), _p(x), _p(dw), _p(db), _p(ws), need, R, N, 128, code, _stream()) == 0
        res.update({f"y_{code}": y, f"dx_{code}": dx, f"dw_{code}": dw, f"db_{code}": db})
    torch.cuda.synchronize()
    return res


def test_no_entry_writes_outside_its_outputs_or_reads_outside_its_inputs():
    arena = _Arena()
    res = _run_all_entries(arena=arena)
    arena.check()
    plain = _run_all_entries()
    for k, v in res.items():
        assert torch.equal(v, plain[k]), k      # ... and the surroundings change no result


def test_every_entry_is_bit_reproducible():
    a, b = _run_all_entries(R=300, seed=7), _run_all_entries(R=300, seed=7)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_chain_and_readout_replay_from_a_captured_graph():
    """Forward and backward of the chain and of the readout recorded in one torch.cuda.graph; the replay equals eager."""
    import torch.nn as nn
    from druggen_amd import functional as dgf
    torch.manual_seed(3)
    E, B, N = 67, 3, 11
    l1, l2, ro = nn.Linear(E, 64).cuda(), nn.Linear(64, 128).cuda(), nn.Linear(128, E).cuda()
    params = list(l1.parameters()) + list(l2.parameters()) + list(ro.parameters())
    z = _features_rows((B, N, E), 9).float().cuda().requires_grad_(True)
    up = _gen((B, N, E), 10).float().cuda()

    def run():
        y = dgf.readout(dgf.node_embed(z, l1, l2, "relu"), ro.weight, ro.bias)
        return (y,) + torch.autograd.grad(y, [z] + params, up)
    # Warm-up on the capture stream, and nothing of this graph on the default stream before the capture: autograd binds the
    # gradient accumulators of z and of the parameters to the stream of their first use, and a backward that has to hand its
    # results over to the default stream cannot be captured.
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = run()
    static = [t.detach() for t in static]      # (same storage; y carries a grad_fn)
    for t in static:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    torch.cuda.synchronize()
    assert len(static) == len(eager) == 8
    for a_, b_ in zip(static, eager):
        assert torch.isfinite(a_).all() and a_.abs().sum() > 0 and torch.equal(a_, b_)


# --------------------------------------------------------------------------------------------------------------------------
# whole model
# --------------------------------------------------------------------------------------------------------------------------
M_N, M_A, M_F, M_B, M_E = 6, 5, 54, 3, 5
BLOCKS = (5, 9, 6, 9, 1, 1, 5, 5, 5, 1, 7)      # the reference's descriptor blocks (dataset.py:161-185): 54 columns


def _feature_graphs(n, seed):
    from types import SimpleNamespace
    rng = np.random.default_rng([n, seed])
    graphs = []
    for _ in range(n):
        x = np.zeros((M_N, M_A + M_F), dtype=np.float32)
        x[np.arange(M_N), rng.integers(0, M_A, size=M_N)] = 1.0
        start = M_A
        for width in BLOCKS:
            if width == 1:
                x[:, start] = rng.integers(0, 2, size=M_N)
            else:
                x[np.arange(M_N), start + rng.integers(0, width, size=M_N)] = 1.0
            start += width
        upper = np.triu((rng.random((M_N, M_N)) < 0.4) * rng.integers(1, M_E, size=(M_N, M_N)), 1)
        src, dst = np.nonzero(upper + upper.T)
        graphs.append(SimpleNamespace(x=x, edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=(upper + upper.T)[src, dst]))
    return graphs


class _Spy:
    """Records the entry names that pass through ``_lib.launch``."""

    def __init__(self, monkeypatch):
        self.names = []
        L = _lib()
        real = L.launch

        def launch(name, ref, *args):
            self.names.append(name)
            return real(name, ref, *args)
        monkeypatch.setattr(L, "launch", launch)


WIDE = {"dg_embed_node_wide_chain", "dg_embed_node_wide_bwd", "dg_embed_node_wide_wgrad", "dg_wide_linear_fwd",
        "dg_wide_linear_dgrad", "dg_wide_linear_wgrad"}
NARROW_NODE = {"dg_embed_node_chain", "dg_embed_node_bwd"}


def _models(m_dim, seed):
    from druggen_amd import synth
    from druggen_amd.model import Discriminator, Generator
    cfg = orc.NetConfig(act="relu", vertexes=M_N, edges=M_E, nodes=m_dim, dropout=0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
    gp = synth.fill_parameters(orc.generator_schema(cfg), seed, 1.7)
    dp = synth.fill_parameters(orc.discriminator_schema(cfg), seed + 1, 1.7)
    args = (cfg.act, cfg.vertexes, cfg.edges, cfg.nodes, cfg.dropout)
    kw = dict(dim=cfg.dim, depth=cfg.depth, heads=cfg.heads, mlp_ratio=cfg.mlp_ratio)
    G, D = Generator(*args, **kw), Discriminator(*args, **kw)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in gp.items()})
    D.load_state_dict({k: torch.from_numpy(v) for k, v in dp.items()})
    return cfg, gp, dp, G.cuda(), D.cuda()


def _table_errors(mod, onet):
    """Per-tensor error of the goldens' comparison (tests/harness.py::grad_table_errors on full tensors): ||got - want|| /
    max(||want||, ||all grads|| / sqrt(n_tensors)); the None-gradient sets must agree."""
    want = dict(zip(onet.names, onet.flat))
    live = [k for k, p in want.items() if p.grad is not None]
    floor = sum(float((want[k].grad ** 2).sum()) for k in live) ** 0.5 / len(live) ** 0.5
    errs = []
    for k, p in mod.named_parameters():
        assert (p.grad is None) == (want[k].grad is None), k
        if p.grad is not None:
            w = want[k].grad.numpy()
            errs.append((float(np.linalg.norm(harness._np(p.grad) - w) / max(np.linalg.norm(w), floor)), k))
    return sorted(errs, reverse=True)


def test_features_model_step_against_fp64_oracle_on_the_wide_kernels(monkeypatch):
    """A --features Generator and Discriminator (N = 6, atom_dim = 5, F = 54, dim 128, depth 1, B = 3, relu) on a batch from a
    feature store: one GANStep iteration launches the wide chain, the wide weight gradient and the wide readout and no narrow
    chain entry; the D step and the G step against the float64 oracle at the goldens' 1e-3 per tensor."""
    from druggen_amd import synth
    from druggen_amd.model import discriminator_loss, generator_loss
    from druggen_amd.resident import ResidentMolecules
    from druggen_amd.trainer import GANStep
    M = M_A + M_F
    cfg, gp, dp, G, D = _models(M, 901)
    mols = ResidentMolecules.from_graphs(_feature_graphs(7, 1), device="cuda", b_dim=M_E, atom_dim=M_A)
    drugs = ResidentMolecules.from_graphs(_feature_graphs(5, 2), device="cuda", b_dim=M_E, atom_dim=M_A)
    assert mols.m_dim == M and mols.bits is not None
    _, a, x = mols.batch([6, 0, 3])
    _, da, dx = drugs.batch([1, 4, 4])
    ee, en = (torch.from_numpy(t) for t in synth.interpolation_eps(M_B, 905))
    OG = orc.OracleNet("G", cfg, {k: torch.from_numpy(v).double() for k, v in gp.items()})
    OD = orc.OracleNet("D", cfg, {k: torch.from_numpy(v).double() for k, v in dp.items()})
    c64 = lambda t: t.detach().double().cpu()
    # the D step and the G step, one backward each, against the oracle
    _, _, d_loss = discriminator_loss(G, D, da, dx, a, x, M_B, "cuda", 10.0, eps=(ee.cuda(), en.cuda()))
    d_loss.backward()
    _, _, od = orc.discriminator_loss(OG, OD, c64(da), c64(dx), c64(a), c64(x), 10.0, ee.double(), en.double())
    od.backward()
    harness.compare_scalar(d_loss, float(od.detach()), 1e-3, "d_loss")
    assert all(p.grad is None for p in G.parameters()), "generator received gradients in the D step"
    worst_d = _table_errors(D, OD)
    for net in (D, G):
        net.zero_grad(set_to_none=True)
    for p in list(OD.flat) + list(OG.flat):
        p.grad = None
    g_loss = generator_loss(G, D, a, x, M_B)[0]
    g_loss.backward()
    og = orc.generator_loss(OG, OD, c64(a), c64(x))[0]
    og.backward()
    harness.compare_scalar(g_loss, float(og.detach()), 1e-3, "g_loss")
    worst_g = _table_errors(G, OG)
    print("worst D", worst_d[:2], "worst G", worst_g[:2])
    assert worst_d[0][0] <= 1e-3 and worst_g[0][0] <= 1e-3
    assert {k for _, k in worst_g} >= {"node_layers.0.weight", "readout_n.weight", "readout_n.bias"}
    # one iteration of the trainer: what it launches
    for net in (D, G):
        net.zero_grad(set_to_none=True)
    spy = _Spy(monkeypatch)
    st = GANStep(G, D, g_lr=1e-5, d_lr=1e-5)
    losses = st.step(da, dx, a, x, eps=(ee.cuda(), en.cuda()))
    torch.cuda.synchronize()
    harness.compare_scalar(losses[0], float(od.detach()), 1e-3, "d_loss of the step")
    assert torch.isfinite(torch.stack(losses)).all()
    seen = set(spy.names)
    assert WIDE <= seen, sorted(WIDE - seen)
    assert not (NARROW_NODE & seen), sorted(NARROW_NODE & seen)
    assert "dg_skinny_linear_fwd" in seen      # readout_e (5 classes) stays where it was


def test_model_without_features_launches_none_of_the_new_entries(monkeypatch):
    from druggen_amd import synth
    from druggen_amd.trainer import GANStep
    cfg, _, _, G, D = _models(M_A, 911)
    a, x, _, _ = synth.molecule_batch(M_B, M_N, M_E, M_A, seed=3)
    da, dx, _, _ = synth.molecule_batch(M_B, M_N, M_E, M_A, seed=4)
    ee, en = (torch.from_numpy(t).cuda() for t in synth.interpolation_eps(M_B, 5))
    spy = _Spy(monkeypatch)
    t = lambda v: torch.from_numpy(v).cuda()
    losses = GANStep(G, D, g_lr=1e-5, d_lr=1e-5).step(t(da), t(dx), t(a), t(x), eps=(ee, en))
    torch.cuda.synchronize()
    assert torch.isfinite(torch.stack(losses)).all()
    seen = set(spy.names)
    assert NARROW_NODE <= seen and not any("wide" in n for n in seen), sorted(n for n in seen if "wide" in n)
