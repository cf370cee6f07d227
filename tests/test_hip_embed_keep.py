"""The edge embedding on KEPT signs (csrc/embed_sym_keep.hip): dg_embed_sym_fwd_keep / _bwd_keep / _bwd2_keep against the
entries they stand in for (dg_embed_sym_fwd / _bwd / _bwd2, which recompute the forward for its ReLU masks).  Same tiles,
products and summation orders, so every comparison here is bit for bit; the sign bits themselves are checked against a
float64 evaluation of both pre-activations."""
import functools
import math

import pytest
import torch

import cases
import harness

pytestmark = pytest.mark.gpu

# (1,1,5): one diagonal pair in an otherwise empty tile; (3,8,5): 36 pairs = a second tile with 4 pairs; (2,45,5): the
# headline's N, 1035 = 32 * 32 + 11 pairs; (1,49,16): kMaxE, N > 48
SHAPES = [(1, 1, 5), (3, 8, 5), (2, 9, 10), (2, 45, 5), (1, 49, 16), (1, 97, 5)]
ACTS = ["relu", "leaky"]
DTYPES = ["f32", "bf16"]
ACT_ID = {"relu": 0, "leaky": 1, "sigmoid": 2, "tanh": 3}
E_ARG = -2
SENTINEL = 0x5A5A5A5A
GUARD = 64


def _lib():
    from druggen_amd import _lib as lib
    return lib


def _bits(x):
    return x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def _same(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))


def _p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def _inputs(B, N, E):
    """The inputs of every test at one shape (CPU float32, never written afterwards)."""
    torch.manual_seed(7)
    a = torch.rand(B, N, N, E)
    a = a / a.sum(-1, keepdim=True)
    w1, b1 = torch.randn(64, E) / math.sqrt(E), 0.1 * torch.randn(64)
    w2, b2 = torch.randn(128, 64) / 8, 0.1 * torch.randn(128)
    g = torch.randn(B, N, N, 128)
    t = torch.randn(B, N, N, E)
    return a, w1, b1, w2, b2, g, t


class _Case:
    """Device tensors of one (shape, activation, dtype) and the results of the recomputing entries -- the yardstick."""

    def __init__(self, B, N, E, act, dt):
        from druggen_amd import functional as dgf
        self.B, self.N, self.E, self.act, self.dt = B, N, E, ACT_ID[act], dt
        self.odt = torch.float32 if dt == "f32" else torch.bfloat16
        self.lib = _lib().load()
        a, w1, b1, w2, b2, g, t = (x.cuda() for x in _inputs(B, N, E))
        self.a, self.w1, self.b1, self.w2, self.b2, self.t = a, w1, b1, w2, b2, t
        self.g = g.to(self.odt)
        self.w2p, self.w2d = dgf._embed_packed_w2(w2), dgf._embed_packed_w2(w2, True)
        self.code = _lib().dt(self.g)
        self.tail = (B, N, E, 64, 128, self.act, self.code, None)
        self.ws = torch.empty(int(self.lib.dg_embed_sym_workspace_bytes(B, N)), dtype=torch.uint8, device="cuda")
        self.words = int(self.lib.dg_embed_sym_sign_words(B, N))
        # yardstick: forward, backward with and without the input gradient, second order
        self.out = torch.empty(B, N, N, 128, dtype=self.odt, device="cuda")
        self._ok(self.lib.dg_embed_sym_fwd(_p(a), _p(w1), _p(b1), _p(self.w2p), _p(b2), _p(self.out), *self.tail))
        self.ref = self.old_bwd(True)
        self.ref_noda = self.old_bwd(False)
        self.ref2 = self.old_bwd2()
        self.signs = self.fwd_keep(0)[1]

    def _ok(self, status):
        assert status == 0, (status, self.lib.dg_last_error_string())

    def weights(self):
        return [torch.empty_like(x) for x in (self.w1, self.b1, self.w2, self.b2)]

    def old_bwd(self, want_da):
        da = torch.empty_like(self.a) if want_da else None
        dw = self.weights()
        self._ok(self.lib.dg_embed_sym_bwd(_p(self.a), _p(self.w1), _p(self.b1), _p(self.w2p), _p(self.w2d), _p(self.b2),
                                           _p(self.g), _p(da), *[_p(x) for x in dw], _p(self.ws), self.ws.numel(), *self.tail))
        return [da] + dw

    def old_bwd2(self):
        gg, gw1, gw2 = torch.empty_like(self.g), torch.empty_like(self.w1), torch.empty_like(self.w2)
        self._ok(self.lib.dg_embed_sym_bwd2(_p(self.a), _p(self.w1), _p(self.b1), _p(self.w2p), _p(self.w2d), _p(self.b2),
                                            _p(self.g), _p(self.t), _p(gg), _p(gw1), _p(gw2), _p(self.ws), self.ws.numel(),
                                            *self.tail))
        return gg, gw1, gw2

    def fwd_keep(self, fill):
        """(output, sign words, guard words behind them) of dg_embed_sym_fwd_keep into a buffer pre-filled with ``fill``
        (0: all bits clear, -1: all bits set)."""
        buf = torch.full((self.words + GUARD,), fill, dtype=torch.int32, device="cuda")
        buf[self.words:] = SENTINEL
        out = torch.empty_like(self.out)
        self._ok(self.lib.dg_embed_sym_fwd_keep(_p(self.a), _p(self.w1), _p(self.b1), _p(self.w2p), _p(self.b2), _p(out),
                                                _p(buf), *self.tail))
        return out, buf[:self.words], buf[self.words:]

    def bwd_keep(self, signs, want_da, want_w, ws=None):
        da = torch.empty_like(self.a) if want_da else None
        dw = self.weights() if want_w else [None] * 4
        ws = self.ws if ws is None else ws
        self._ok(self.lib.dg_embed_sym_bwd_keep(_p(self.a), _p(self.w1), _p(self.b1), _p(self.w2p), _p(self.w2d),
                                                _p(self.b2), _p(self.g), _p(signs), _p(da), *[_p(x) for x in dw], _p(ws),
                                                ws.numel(), *self.tail))
        return [da] + dw

    def bwd2_keep(self, signs, want_w, ws=None):
        gg = torch.empty_like(self.g)
        gw1, gw2 = (torch.empty_like(self.w1), torch.empty_like(self.w2)) if want_w else (None, None)
        ws = self.ws if ws is None else ws
        self._ok(self.lib.dg_embed_sym_bwd2_keep(_p(self.a), _p(self.w1), _p(self.b1), _p(self.w2p), _p(self.w2d),
                                                 _p(self.b2), _p(self.g), _p(self.t), _p(signs), _p(gg), _p(gw1), _p(gw2),
                                                 _p(ws), ws.numel(), *self.tail))
        return gg, gw1, gw2


@functools.lru_cache(maxsize=None)
def _case(B, N, E, act, dt):
    return _Case(B, N, E, act, dt)


def _grid(f):
    for name, values in (("dt", DTYPES), ("act", ACTS)):
        f = pytest.mark.parametrize(name, values)(f)
    return pytest.mark.parametrize("B,N,E", SHAPES)(f)


@_grid
def test_forward_is_bit_identical_and_writes_every_sign_word(B, N, E, act, dt):
    c = _case(B, N, E, act, dt)
    out0, s0, guard0 = c.fwd_keep(0)
    out1, s1, guard1 = c.fwd_keep(-1)
    assert _same(out0, c.out) and _same(out1, c.out)
    assert torch.equal(s0, s1), "a sign word was left as the buffer held it"
    assert torch.equal(s0, c.signs)
    for guard in (guard0, guard1):
        assert bool((guard == SENTINEL).all()), "wrote behind the sign buffer"


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B,N,E", SHAPES)
def test_sign_bits_are_the_signs_of_the_float64_pre_activations(B, N, E, act):
    """Bit set <=> pre-activation > 0, wherever the float64 pre-activation is at least 1e-5 from zero (float32 is within
    3.5e-7 of float64 for these inputs, so a disagreement outside the band is a defect); the band leaves out at most 1e-3
    of the elements.  Both output dtypes keep the same signs: they are taken before the output is rounded."""
    c = _case(B, N, E, act, "f32")
    assert torch.equal(c.signs, _case(B, N, E, act, "bf16").signs)
    a, w1, b1, w2, b2 = (x.double() for x in _inputs(B, N, E)[:5])
    F = torch.nn.functional
    f = torch.relu if act == "relu" else (lambda x: F.leaky_relu(x, 0.01))
    pre1 = F.linear(a, w1, b1)
    pre2 = F.linear(f(pre1), w2, b2)
    words = c.signs.cpu().view(B, N, N, 6).to(torch.int64) & 0xFFFFFFFF
    shifts = torch.arange(32)
    got = ((words.unsqueeze(-1) >> shifts) & 1).bool()          # [B,N,N,6,32]
    got2, got1 = got[..., :4, :].reshape(B, N, N, 128), got[..., 4:, :].reshape(B, N, N, 64)
    for name, bits, pre in (("layer 2", got2, pre2), ("layer 1", got1, pre1)):
        clear = pre.abs() >= 1e-5
        assert (~clear).sum().item() <= 1e-3 * clear.numel(), name
        assert torch.equal(bits[clear], (pre > 0)[clear]), name


@_grid
def test_backward_wanted_outputs_are_bit_identical(B, N, E, act, dt):
    c = _case(B, N, E, act, dt)
    names = "da dw1 db1 dw2 db2".split()
    for want_da, want_w in ((True, False), (True, True), (False, True)):
        ref = c.ref if want_da else c.ref_noda
        ws = c.ws
        if not want_w:      # the workspace belongs to the weight gradients: it must stay as it was
            ws = torch.full_like(c.ws, 0x5A)
        got = c.bwd_keep(c.signs, want_da, want_w, ws)
        for name, x, y in zip(names, got, ref):
            if x is not None:
                assert _same(x, y), (name, want_da, want_w)
        if not want_w:
            assert bool((ws == 0x5A).all())
    # the weight gradients come all four or not at all
    dw = c.weights()
    lib = c.lib
    for k in range(4):
        mixed = [_p(x) for x in dw]
        mixed[k] = None
        st = lib.dg_embed_sym_bwd_keep(_p(c.a), _p(c.w1), _p(c.b1), _p(c.w2p), _p(c.w2d), _p(c.b2), _p(c.g), _p(c.signs),
                                       None, *mixed, _p(c.ws), c.ws.numel(), *c.tail)
        assert st == E_ARG and b"all given or all NULL" in lib.dg_last_error_string()
    # nothing wanted: no launch, no error
    assert lib.dg_embed_sym_bwd_keep(_p(c.a), _p(c.w1), _p(c.b1), _p(c.w2p), _p(c.w2d), _p(c.b2), _p(c.g), _p(c.signs),
                                     None, None, None, None, None, None, 0, *c.tail) == 0


@_grid
def test_second_order_is_bit_identical(B, N, E, act, dt):
    c = _case(B, N, E, act, dt)
    gg, gw1, gw2 = c.bwd2_keep(c.signs, True)
    assert _same(gg, c.ref2[0]) and _same(gw1, c.ref2[1]) and _same(gw2, c.ref2[2])
    ws = torch.full_like(c.ws, 0x5A)
    gg, gw1, gw2 = c.bwd2_keep(c.signs, False, ws)
    assert _same(gg, c.ref2[0]) and gw1 is None and gw2 is None
    assert bool((ws == 0x5A).all())


@_grid
def test_every_consumed_sign_bit_was_written_and_launches_repeat(B, N, E, act, dt):
    """Signs written into a zero-filled and into a one-filled buffer give the same gradients; so does a second launch."""
    c = _case(B, N, E, act, dt)
    s0, s1 = c.fwd_keep(0)[1], c.fwd_keep(-1)[1]
    runs = []
    for signs in (s0, s1, s1):
        outs = c.bwd_keep(signs, True, True) + list(c.bwd_keep(signs, True, False)[:1]) + list(c.bwd2_keep(signs, True))
        runs.append(outs)
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert _same(x, y)


def test_keep_entries_refuse_smooth_activations():
    """Signs describe relu / leaky only: sigmoid / tanh are refused like dg_embed_sym_bwd2 refuses them."""
    lib = _lib().load()
    x = torch.zeros(4096, device="cuda")
    p = x.data_ptr()
    shape = (1, 9, 5, 64, 128)
    for act in (2, 3):
        assert lib.dg_embed_sym_fwd_keep(*[p] * 7, *shape, act, 0, None) == E_ARG
        assert b"piecewise-linear" in lib.dg_last_error_string()
        assert lib.dg_embed_sym_bwd_keep(*[p] * 13, p, 1 << 30, *shape, act, 0, None) == E_ARG
        assert b"piecewise-linear" in lib.dg_last_error_string()
        assert lib.dg_embed_sym_bwd2_keep(*[p] * 12, p, 1 << 30, *shape, act, 0, None) == E_ARG
        assert b"piecewise-linear" in lib.dg_last_error_string()
    assert lib.dg_embed_sym_sign_words(3, 8) == 3 * 8 * 8 * 6


def _autograd_results(B, N, E, act, odt, keep):
    """Forward, first-order gradients in the three patterns a step uses, and the create_graph second order of
    ``dgf.embed_sym`` (as in test_hip_kernels.py::test_embed_sym_all_orders) with the hook ``embed_keep`` set to ``keep``."""
    from druggen_amd import functional as dgf
    from druggen_amd.options import options
    a, w1, b1, w2, b2, g, t = (x.cuda() for x in _inputs(B, N, E))
    g = g.to(odt)
    res = {}
    with options.override(embed_keep=keep):
        ins = [x.clone().requires_grad_(True) for x in (a, w1, b1, w2, b2)]
        out = dgf.embed_sym(*ins, act, odt)
        res["out"] = out.detach()
        for k, v in zip("da dw1 db1 dw2 db2".split(), torch.autograd.grad(out, ins, g)):
            res[k] = v
        # parameters only (D(fake) in the D step) / input only (the G step's pass through D)
        out = dgf.embed_sym(a, *ins[1:], act, odt)
        for k, v in zip("p.dw1 p.db1 p.dw2 p.db2".split(), torch.autograd.grad(out, ins[1:], g)):
            res[k] = v
        out = dgf.embed_sym(ins[0], w1, b1, w2, b2, act, odt)
        res["i.da"] = torch.autograd.grad(out, ins[0], g)[0]
        with dgf.inputs_only_backward():
            out = dgf.embed_sym(*ins, act, odt)
            res["io.da"] = torch.autograd.grad(out, ins[0], g)[0]
        # the gradient penalty's pattern
        gd = g.clone().requires_grad_(True)
        ga = torch.autograd.grad(dgf.embed_sym(*ins, act, odt), ins[0], gd, create_graph=True)[0]
        res["ga"] = ga.detach()
        for k, v in zip("gw1 gw2 gg".split(), torch.autograd.grad((ga * t).sum(), [ins[1], ins[3], gd], allow_unused=True)):
            res[k] = v
        # ... as the trainer runs it: the forward declared as one a second order follows, the first backward inputs-only
        with dgf.second_order_forward():
            out = dgf.embed_sym(*ins, act, odt)
        with dgf.inputs_only_backward():
            ga = torch.autograd.grad(out, ins[0], gd, create_graph=True)[0]
        res["so.ga"] = ga.detach()
        for k, v in zip("so.gw1 so.gw2 so.gg".split(), torch.autograd.grad((ga * t).sum(), [ins[1], ins[3], gd], allow_unused=True)):
            res[k] = v
        with dgf.inputs_only_backward():
            ga = torch.autograd.grad(dgf.embed_sym(*ins, act, odt), ins[0], gd, create_graph=True)[0]
            res["io.gg"] = torch.autograd.grad((ga * t).sum(), gd)[0]
    return res


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B,N,E", [(3, 8, 5), (2, 45, 5), (1, 49, 16)])
def test_autograd_results_do_not_depend_on_the_hook(B, N, E, act, dt):
    odt = torch.float32 if dt == "f32" else torch.bfloat16
    old = _autograd_results(B, N, E, act, odt, False)
    new = _autograd_results(B, N, E, act, odt, True)
    assert old.keys() == new.keys()
    for k in old:
        if old[k] is None:
            assert new[k] is None, k
        else:
            assert new[k] is not None and _same(old[k], new[k]), k


def test_whole_step_does_not_depend_on_the_hook():
    """One GANStep.step at dim 128, depth 1, N = 9, B = 4: the same losses and the same G and D parameters, bit for bit."""
    from druggen_amd.model import Discriminator, Generator
    from druggen_amd.options import options
    from druggen_amd.trainer import GANStep
    case = cases.CASES["c1_b4"]
    cfg = cases.net_config(case)
    assert (cfg.dim, cfg.depth, cfg.vertexes, case["batch"]) == (128, 1, 9, 4)
    gp, dp = cases.build_params(case)
    inp = harness.torch_inputs(case, torch.float32, "cuda")
    runs = []
    for keep in (False, True):
        args = (cfg.act, cfg.vertexes, cfg.edges, cfg.nodes, cfg.dropout)
        kw = dict(dim=cfg.dim, depth=cfg.depth, heads=cfg.heads, mlp_ratio=cfg.mlp_ratio)
        G, D = Generator(*args, **kw), Discriminator(*args, **kw)
        G.load_state_dict({k: torch.from_numpy(v) for k, v in gp.items()})
        D.load_state_dict({k: torch.from_numpy(v) for k, v in dp.items()})
        G, D = G.cuda(), D.cuda()
        with options.override(embed_keep=keep):
            st = GANStep(G, D, lambda_gp=case["lambda_gp"])
            d_loss, g_loss = st.step(inp["disc_edge"], inp["disc_node"], inp["gen_edge"], inp["gen_node"],
                                     eps=(inp["eps_edge"], inp["eps_node"]))
        runs.append([d_loss.detach().clone(), g_loss.detach().clone()]
                    + [p.detach().clone() for p in list(G.parameters()) + list(D.parameters())])
    assert len(runs[0]) == len(runs[1])
    for x, y in zip(*runs):
        assert _same(x, y)
