"""GPU tests of the any-width row GEMM (dg_row_gemm_any, csrc/row_gemm_any.hip) and of the --dim / --mlp_ratio models it carries:
the kernel against float64, its row scales, determinism and tiling, agreement with dg_row_gemm on that kernel's three shapes, the
route in functional.dense, pack freshness, whole models against the float64 oracle and against the BLAS route, graph capture."""
import functools

import pytest
import torch

import harness
from oracle import druggen_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 2e-5          # tests/test_hip_kernels.py: fp32 kernels vs fp64, relative L2
TOL_ROUTES = 2e-6   # tests/test_hip_kernels.py: two float32 routes to the same product
TOL_STEP = 1e-3     # north_star: losses and gradients of a step, per tensor
TOL_SWITCH = 1e-4   # the same model on the BLAS route, per tensor

SHAPES = [(32, 32), (32, 1024), (1024, 32), (64, 64), (64, 192), (192, 64), (96, 160), (256, 768), (768, 256), (1024, 1024)]
# beyond the list above: both sides of the width at which the tile changes from 64 to 32 rows (K = 256 | 288), the widest row of
# at most two chunks per lane group (K = 512), a chunk count that is no multiple of the groups' stride (K = 544)
EXTRA_SHAPES = [(288, 96), (512, 160), (544, 64)]
ROWS = (1, 63, 64, 65, 130)


def _rel(got, want):
    want = want.double()
    den = want.norm().item()
    return (got.double().cpu() - want).norm().item() / (den if den > 0 else 1.0)


def _gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _pack(w, mode):
    """The packed operand of the float32 CUDA weight ``w`` [rows, cols] -> (packed, K, N)."""
    from druggen_amd import _lib
    lib = _lib.load()
    rows, cols = w.shape
    n_out, k = (rows, cols) if mode == 0 else (cols, rows)
    packed = torch.empty(int(lib.dg_row_gemm_any_packed_bytes(n_out, k)), dtype=torch.uint8, device=w.device)
    _lib.launch("dg_row_gemm_any_pack", w, w.data_ptr(), packed.data_ptr(), rows, cols, mode)
    return packed, k, n_out


def _gemm(a, packed, bias, K, N):
    from druggen_amd import _lib
    y = torch.empty(a.shape[0], N, dtype=torch.float32, device=a.device)
    _lib.launch("dg_row_gemm_any", a, a.data_ptr(), packed.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(),
                a.shape[0], K, N)
    return y


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K,N", SHAPES + EXTRA_SHAPES)
def test_kernel_against_float64(K, N, mode):
    """y = a W^T + b (mode 0, W [N,K]) and y = a W (mode 1, W [K,N]) for every row count of ROWS, with and without a bias."""
    w64 = _gen((N, K) if mode == 0 else (K, N), 1000 + K + N, K ** -0.5)
    b64 = _gen((N,), 2000 + K + N, 0.3)
    w, b = w64.float().cuda(), b64.float().cuda()
    w64, b64 = w.double().cpu(), b.double().cpu()
    packed, k, n = _pack(w, mode)
    assert (k, n) == (K, N)
    for R in ROWS:
        a = _gen((R, K), 3000 + R, 1.5).float().cuda()
        want = a.double().cpu() @ (w64.t() if mode == 0 else w64)
        for bias in (b, None):
            got = _gemm(a, packed, bias, K, N)
            err = _rel(got, want + b64 if bias is not None else want)
            assert err < TOL, (R, bias is not None, err)


def _scaled_rows(K, N):
    """N(0,1) rows times factors from 1e-20 to 1e+20, an all-zero row and a row with one non-zero element."""
    R = 41
    a = _gen((R, K), 77).float()
    a[:39] *= torch.logspace(-20, 20, 39, dtype=torch.float64).float()[:, None]
    a[39] = 0.0
    a[40] = 0.0
    a[40, K // 3] = -2.75
    w = _gen((N, K), 78, K ** -0.5).float()
    b = _gen((N,), 79, 0.3).float()
    return a, w, b


def test_row_scale():
    """Rows N(0,1) x 10^-20 ... 10^+20 (39 factors, one per row), an all-zero row, a row with a single non-zero element: every row on
    its own is within TOL of float64, the zero row gives exactly the bias, nothing is non-finite.  The factor range is the full
    1e-20 .. 1e+20: the float32 ``F.linear`` on the CPU stays inside TOL on every row of these inputs (asserted below), so the
    range needed no narrowing."""
    K, N = 96, 160
    a, w, b = _scaled_rows(K, N)
    prod = a.double() @ w.double().t()
    want = prod + b.double()
    cpu32 = torch.nn.functional.linear(a, w, b)
    for r in range(a.shape[0]):
        assert _rel(cpu32[r], want[r]) < TOL, ("float32 F.linear on the CPU", r)
    packed, _, _ = _pack(w.cuda(), 0)
    got = _gemm(a.cuda(), packed, b.cuda(), K, N).cpu()
    assert torch.isfinite(got).all()
    for r in range(a.shape[0]):
        assert _rel(got[r], want[r]) < TOL, (r, _rel(got[r], want[r]))
    assert torch.equal(got[39], b)
    nob = _gemm(a.cuda(), packed, None, K, N).cpu()
    assert torch.isfinite(nob).all() and torch.equal(nob[39], torch.zeros(N))
    for r in range(a.shape[0]):
        assert _rel(nob[r], prod[r]) < TOL, (r, _rel(nob[r], prod[r]))


@pytest.mark.parametrize("K,N", [(64, 192), (96, 160), (288, 96), (768, 256), (1024, 32)])
def test_determinism_and_tiling(K, N):
    """Two launches agree bit for bit; rows 0..63 of an R = 130 launch equal an R = 64 launch on those rows bit for bit (the order
    of the sums does not depend on R or on the tile a row falls in)."""
    a = _gen((130, K), 5).float().cuda()
    w = _gen((N, K), 6, K ** -0.5).float().cuda()
    b = _gen((N,), 7).float().cuda()
    packed, _, _ = _pack(w, 0)
    y0 = _gemm(a, packed, b, K, N)
    y1 = _gemm(a, packed, b, K, N)
    assert torch.equal(y0, y1)
    y64 = _gemm(a[:64].contiguous(), packed, b, K, N)
    assert torch.equal(y0[:64], y64)
    y65 = _gemm(a[65:].contiguous(), packed, b, K, N)      # the same rows at other positions of other tiles
    assert torch.equal(y0[65:], y65)


@pytest.mark.parametrize("K,N", [(128, 128), (128, 384), (384, 128)])
def test_agrees_with_the_three_shape_kernel(K, N):
    from druggen_amd import functional as dgf
    a = _gen((130, K), 11).float().cuda()
    w = _gen((N, K), 12, K ** -0.5).float().cuda()
    b = _gen((N,), 13, 0.3).float().cuda()
    packed, _, _ = _pack(w, 0)
    got = _gemm(a, packed, b, K, N)
    ref = dgf.row_gemm(a, dgf.packed_weight(w, 0), K, N, bias=b)
    assert _rel(got, ref.cpu()) < TOL_ROUTES, _rel(got, ref.cpu())
    want = a.double().cpu() @ w.double().cpu().t() + b.double().cpu()
    assert _rel(got, want) < TOL and _rel(ref, want) < TOL


def test_routing():
    from druggen_amd import functional as dgf
    from druggen_amd.options import options
    assert dgf.any_gemm_supported(64, 192)
    assert not dgf.any_gemm_supported(128, 384) and dgf.row_gemm_supported(128, 384)      # _mm_rows picks row_gemm for it
    x = _gen((3, 7, 64), 21).float().cuda()
    w = _gen((64, 64), 22, 0.125).float().cuda()
    b = _gen((64,), 23).float().cuda()
    want = x.double().cpu() @ w.double().cpu().t() + b.double().cpu()
    dgf.traffic_reset()
    y = dgf.linear(x, w, b)
    assert dgf.traffic_bytes("row_gemm_any") == 4 * 21 * 128 and dgf.traffic_flops("row_gemm_any") == 2 * 21 * 64 * 64
    assert y.shape == (3, 7, 64) and _rel(y, want) < TOL
    dgf.traffic_reset()
    with options.override(row_gemm_any=False):
        y_blas = dgf.linear(x, w, b)
    assert dgf.traffic_bytes("row_gemm_any") == 0
    assert _rel(y_blas, want) < TOL
    assert dgf.linear(x[:0], w, b).shape == (0, 7, 64)      # no rows: nothing is launched
    # the three shapes stay where they were
    dgf.traffic_reset()
    dgf.linear(_gen((5, 128), 24).float().cuda(), _gen((384, 128), 25, 0.1).float().cuda(), None)
    assert dgf.traffic_bytes("row_gemm_any") == 0 and dgf.traffic_bytes("row_gemm") > 0
    # bf16 activations at other widths stay on the BLAS
    dgf.traffic_reset()
    xb = x.bfloat16()
    yb = dgf.linear(xb, w, b)
    assert dgf.traffic_bytes("row_gemm_any") == 0
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, torch.nn.functional.linear(xb, w.bfloat16(), b.bfloat16()))


def test_gradients_through_the_route():
    """dgf.linear at (96 -> 160): forward, input gradient (pack mode 1) and weight gradients against float64 autograd."""
    from druggen_amd import functional as dgf
    x = _gen((70, 96), 31).float().cuda().requires_grad_()
    w = _gen((160, 96), 32, 0.1).float().cuda().requires_grad_()
    b = _gen((160,), 33).float().cuda().requires_grad_()
    dy = _gen((70, 160), 34).float().cuda()
    dgf.traffic_reset()
    y = dgf.linear(x, w, b)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), dy)
    assert dgf.traffic_flops("row_gemm_any") == 2 * (2 * 70 * 96 * 160)      # forward + input gradient
    x64, w64, b64 = (t.detach().double().cpu().requires_grad_() for t in (x, w, b))
    y64 = torch.nn.functional.linear(x64, w64, b64)
    want = torch.autograd.grad(y64, (x64, w64, b64), dy.double().cpu())
    assert _rel(y, y64.detach()) < TOL
    for got, ref in zip((gx, gw, gb), want):
        assert _rel(got, ref) < TOL


def test_pack_freshness():
    """After an in-place weight update behind autograd's back and ``bump_weights_epoch()`` the next launch uses the new weight; an
    update that autograd sees (``_version``) needs no bump."""
    from druggen_amd import functional as dgf
    x = _gen((9, 64), 41).float().cuda()
    w = torch.nn.Parameter(_gen((192, 64), 42, 0.1).float().cuda())
    y0 = dgf.linear(x, w)
    assert _rel(y0, x.double().cpu() @ w.detach().double().cpu().t()) < TOL
    w.data.mul_(-3.0)      # (.data: the version counter does not move)
    dgf.bump_weights_epoch()
    y1 = dgf.linear(x, w)
    assert _rel(y1, x.double().cpu() @ w.detach().double().cpu().t()) < TOL
    assert _rel(y1, -3.0 * y0.double().cpu()) < TOL
    with torch.no_grad():
        w.add_(0.25)
    y2 = dgf.linear(x, w)
    assert _rel(y2, x.double().cpu() @ w.detach().double().cpu().t()) < TOL


# ---- whole models -------------------------------------------------------------------------------------------------------
# (dim, heads, mlp_ratio, depth) -> seed.  Seeds are fixed here; a seed whose G gradient sits on a ReLU threshold of D (as the
# golden case c5_b2 does, tests/test_hip_model.py) would be replaced by another one, never met by a wider bar.
MODELS = {"dim64": (dict(dim=64, heads=4, mlp_ratio=2, depth=2), 501), "dim32": (dict(dim=32, heads=8, mlp_ratio=4, depth=1), 521)}
B, N_ATOMS = 3, 9


def _config(name):
    kw, seed = MODELS[name]
    return orc.NetConfig(act="relu", vertexes=N_ATOMS, edges=5, nodes=13, dropout=0.0, **kw), seed


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Weights, batch and the float64 oracle's losses / gradients of one D step and one G step -- computed once, never changed."""
    from druggen_amd import synth
    cfg, seed = _config(name)
    gp = synth.fill_parameters(orc.generator_schema(cfg), seed, 1.7)
    dp = synth.fill_parameters(orc.discriminator_schema(cfg), seed + 1, 1.7)
    a, x, _, _ = synth.molecule_batch(B, cfg.vertexes, cfg.edges, cfg.nodes, seed=seed + 2)
    da, dx, _, _ = synth.molecule_batch(B, cfg.vertexes, cfg.edges, cfg.nodes, seed=seed + 3)
    ee, en = synth.interpolation_eps(B, seed + 4)
    OG = orc.OracleNet("G", cfg, {k: torch.from_numpy(v).double() for k, v in gp.items()})
    OD = orc.OracleNet("D", cfg, {k: torch.from_numpy(v).double() for k, v in dp.items()})
    t64 = lambda v: torch.from_numpy(v).double()

    def grads(onet):
        return {k: (None if p.grad is None else p.grad.clone()) for k, p in zip(onet.names, onet.flat)}
    _, _, od = orc.discriminator_loss(OG, OD, t64(da), t64(dx), t64(a), t64(x), 10.0, t64(ee), t64(en))
    od.backward()
    assert all(p.grad is None for p in OG.flat)
    ref = {"d_loss": float(od.detach()), "D": grads(OD)}
    for p in list(OD.flat) + list(OG.flat):
        p.grad = None
    og = orc.generator_loss(OG, OD, t64(a), t64(x))[0]
    og.backward()
    ref.update(g_loss=float(og.detach()), G=grads(OG))
    return dict(cfg=cfg, gp=gp, dp=dp, batch=(da, dx, a, x), eps=(ee, en), ref=ref)


def _nets(name):
    from druggen_amd.model import Discriminator, Generator
    pr = _problem(name)
    cfg = pr["cfg"]
    args = (cfg.act, cfg.vertexes, cfg.edges, cfg.nodes, cfg.dropout)
    kw = dict(dim=cfg.dim, depth=cfg.depth, heads=cfg.heads, mlp_ratio=cfg.mlp_ratio)
    G, D = Generator(*args, **kw), Discriminator(*args, **kw)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in pr["gp"].items()})
    D.load_state_dict({k: torch.from_numpy(v) for k, v in pr["dp"].items()})
    return G.cuda(), D.cuda()


def _hip_step(name):
    """The D step (with the gradient penalty's double backward) and the G step of the HIP modules -> losses, gradients."""
    from druggen_amd.model import discriminator_loss, generator_loss
    pr = _problem(name)
    G, D = _nets(name)
    t32 = lambda v: torch.from_numpy(v).cuda()
    da, dx, a, x = map(t32, pr["batch"])
    ee, en = map(t32, pr["eps"])

    def grads(mod):
        return {k: (None if p.grad is None else p.grad.detach().double().cpu()) for k, p in mod.named_parameters()}
    _, _, d_loss = discriminator_loss(G, D, da, dx, a, x, B, "cuda", 10.0, eps=(ee, en))
    d_loss.backward()
    assert all(p.grad is None for p in G.parameters()), "generator received gradients in the D step"
    out = {"d_loss": float(d_loss.detach()), "D": grads(D)}
    for net in (D, G):
        net.zero_grad(set_to_none=True)
    g_loss = generator_loss(G, D, a, x, B)[0]
    g_loss.backward()
    out.update(g_loss=float(g_loss.detach()), G=grads(G))
    return out


def _worst(got, want, tol, what):
    """Per-tensor error as tests/test_hip_model.py measures it: relative L2, the denominator floored at
    ||all gradients|| / sqrt(n tensors); the None sets must be equal."""
    live = [k for k, v in want.items() if v is not None]
    tot = sum(float((want[k].double() ** 2).sum()) for k in live) ** 0.5
    worst = (0.0, None)
    for k, v in want.items():
        assert (v is None) == (got[k] is None), (what, k)
        if v is None:
            continue
        err = (got[k].double() - v.double()).norm().item() / max(v.double().norm().item(), tot / len(live) ** 0.5)
        worst = max(worst, (err, k))
    assert worst[0] <= tol, (what, worst)
    return worst


@pytest.mark.parametrize("name", list(MODELS))
def test_whole_model_against_fp64_oracle_and_the_blas_route(name):
    """Generator and Discriminator at dim 64 / 32 (B = 3, N = 9): D step and G step against the float64 oracle at 1e-3 per tensor;
    the same model with ``options.row_gemm_any`` off agrees at 1e-4 per tensor."""
    from druggen_amd import functional as dgf
    from druggen_amd.options import options
    ref = _problem(name)["ref"]
    dgf.traffic_reset()
    routed = _hip_step(name)
    assert dgf.traffic_flops("row_gemm_any") > 0, "the model's nn.Linear layers did not reach dg_row_gemm_any"
    for key in ("d_loss", "g_loss"):
        harness.compare_scalar(routed[key], ref[key], TOL_STEP, key)
    print("worst vs fp64", _worst(routed["D"], ref["D"], TOL_STEP, "D"), _worst(routed["G"], ref["G"], TOL_STEP, "G"))
    dgf.traffic_reset()
    with options.override(row_gemm_any=False):
        blas = _hip_step(name)
    assert dgf.traffic_flops("row_gemm_any") == 0
    for key in ("d_loss", "g_loss"):
        harness.compare_scalar(blas[key], routed[key], TOL_SWITCH, key)
    print("worst vs BLAS route", _worst(blas["D"], routed["D"], TOL_SWITCH, "D/blas"), _worst(blas["G"], routed["G"], TOL_SWITCH, "G/blas"))


def test_graphed_step_equals_eager_step_bit_for_bit():
    """``GraphedGANStep`` on the dim = 64 model: the losses of three replays equal those of three eager steps from the same state
    (two steps in: the graph's warm-up) bit for bit."""
    from druggen_amd import functional as dgf
    from druggen_amd.model import discriminator_loss
    from druggen_amd.trainer import GANStep, GraphedGANStep
    pr = _problem("dim64")
    t32 = lambda v: torch.from_numpy(v).cuda()
    batch = tuple(map(t32, pr["batch"]))
    eps = tuple(map(t32, pr["eps"]))
    fixed_eps = lambda *a, **k: discriminator_loss(*a, **{**k, "eps": eps})
    losses = []
    for graphed in (False, True):
        G, D = _nets("dim64")
        st = GANStep(G, D, g_lr=1e-3, d_lr=1e-3, lambda_gp=10.0, d_loss_fn=fixed_eps, share_generator_forward=False)
        run = []
        if graphed:
            dgf.traffic_reset()
            gs = GraphedGANStep(st, *batch, warmup=2)
            assert dgf.traffic_flops("row_gemm_any") > 0
            for _ in range(3):
                d, g = gs.step(*batch)
                run.append((float(d), float(g)))
        else:
            for i in range(5):
                d, g = st.step(*batch)
                if i >= 2:
                    run.append((float(d), float(g)))
        torch.cuda.synchronize()
        losses.append(run)
    print(losses)
    assert losses[0] == losses[1], losses
    assert len({l for l in losses[0]}) == 3      # the steps moved the weights
