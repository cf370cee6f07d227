"""Molecules with more than 96 atoms (reference --max_atom up to 256): the long attention core (dg_attn_core_long_*,
csrc/attn_core_long.hip) against the fp64 closed forms of tests/kernel_math.py and against the short kernels where both
run, its reproducibility, and the model, the loss with its gradient penalty and the training step at N = 128 / 256."""
import math

import pytest
import torch

import kernel_math as km
import test_hip_model as thm
from oracle import druggen_oracle as orc

gpu = pytest.mark.gpu

TOL = 2e-5          # fp32 kernels vs fp64 closed form, relative L2 (as tests/test_hip_kernels.py)
TOL_IO = 4e-3       # bf16 activations (as tests/test_hip_bf16.py)
# long entry vs short entry on the same float32 inputs: the sums run in another order (online-softmax merge of four
# waves, reformulated second-order row sums), so the two agree to float32 rounding, not bit for bit
TOL_SHORT = 1e-6
TOL_SHORT2 = 1e-5


def _rel(got, want):
    want = want.double().cpu()
    den = want.norm().item()
    return (got.double().cpu() - want).norm().item() / (den if den > 0 else 1.0)


def _gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _operands(B, N, C):
    q, k, v = (_gen((B, N, C), s) for s in (1, 2, 3))
    e = _gen((B, N, N, C), 4, 0.8)
    ws, wo = _gen((B, N, N, C), 5), _gen((B, N, C), 6)
    t = [_gen((B, N, C), 7), _gen((B, N, C), 8), _gen((B, N, C), 9), _gen((B, N, N, C), 10)]
    return q, k, v, e, ws, wo, t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _long_launch(op, *tensors, B, N, C, alpha):
    """Direct call of a dg_attn_core_long_* entry (the modules route N <= 96 to the short kernels)."""
    from druggen_amd import _lib
    lib = _lib.load()
    ref = tensors[0]
    dt = 1 if ref.dtype == torch.bfloat16 else 0
    st = torch.cuda.current_stream().cuda_stream
    if op == "fwd":
        code = lib.dg_attn_core_long_fwd(*map(_ptr, tensors), B, N, C, alpha, dt, st)
    else:
        need = int(lib.dg_attn_core_long_workspace_bytes(B, N, C))
        work = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
        fn = lib.dg_attn_core_long_bwd if op == "bwd" else lib.dg_attn_core_long_bwd2
        code = fn(*map(_ptr, tensors), work.data_ptr(), need, B, N, C, alpha, dt, st)
    _lib.check(code, "dg_attn_core_long_" + op)


# ------------------------------------------------------------------------------------------ kernels vs fp64
LONG_SHAPES = [(2, 97, 128), (1, 128, 128), (2, 113, 12), (1, 160, 64), (1, 200, 32), (1, 256, 128)]


@gpu
@pytest.mark.parametrize("B,N,C", LONG_SHAPES)
def test_long_attn_core_forward_backward_second_order(B, N, C):
    from druggen_amd import functional as dgf
    alpha = 1.0 / math.sqrt(C // 4)
    q, k, v, e, ws, wo, t = _operands(B, N, C)
    s_ref, o_ref = km.attn_core_fwd(q, k, v, e, alpha)
    g_ref = km.attn_core_bwd(q, k, v, e, ws, wo, alpha)
    h_ref = km.attn_core_bwd2(q, k, v, e, ws, wo, *t, alpha)
    f = lambda x: x.float().cuda().requires_grad_(True)
    qd, kd, vd, ed, wsd, wod = map(f, (q, k, v, e, ws, wo))
    s, o = dgf.attn_core(qd, kd, vd, ed, alpha)
    assert _rel(s, s_ref) < TOL and _rel(o, o_ref) < TOL
    grads = torch.autograd.grad([s, o], [qd, kd, vd, ed], [wsd, wod], create_graph=True)
    for name, got, want in zip("dq dk dv de".split(), grads, g_ref):
        assert _rel(got, want) < TOL, name
    phi = sum((g * tt.float().cuda()).sum() for g, tt in zip(grads, t))
    second = torch.autograd.grad(phi, [qd, kd, vd, ed, wsd, wod])
    for name, got, want in zip("gq gk gv ge gws gwo".split(), second, h_ref):
        assert _rel(got, want) < 5 * TOL, name


# The geometry switches of DESIGN 3.18 (forward slots per thread 4 / 6 / 8 above N = 96 / 128 / 192; backward 8-quad slices up
# to N = 128; second order 4-quad slices up to N = 192; C < 20 on 4-quad slices; G = ceil(N / 32) row groups, no workspace for
# N <= 32), the short shapes through the long entries, and batches past the first group of 8 molecules (place() pads the
# grid to a multiple of 8 and gives molecule b the XCD residue b % 8; the reverse walk mirrors over the padded count).
BOUNDARY_SHAPES = [(1, 1, 128), (1, 32, 128), (1, 33, 128), (1, 96, 128), (1, 129, 128), (1, 192, 128), (1, 193, 128),
                   (1, 255, 128), (1, 256, 16), (1, 161, 48), (9, 97, 32), (17, 97, 32), (9, 193, 32), (17, 193, 32)]
SENTINEL = -1.5e38


def _guarded(B, shape):
    """[Bpad, *shape] float32 buffer filled with SENTINEL, Bpad = B rounded up to a multiple of 8 (the molecules place()
    pads the grid with): the launch gets its first B molecules, the rest is the guard region."""
    return torch.full(((B + 7) // 8 * 8,) + tuple(shape), SENTINEL, dtype=torch.float32, device="cuda")


def _closed_forms_per_molecule(ops, t, alpha, b):
    q, k, v, e, ws, wo = (x[b:b + 1] for x in ops)
    s, o = km.attn_core_fwd(q, k, v, e, alpha)
    g = km.attn_core_bwd(q, k, v, e, ws, wo, alpha)
    h = km.attn_core_bwd2(q, k, v, e, ws, wo, *(x[b:b + 1] for x in t), alpha)
    return dict(zip("s o dq dk dv de gq gk gv ge gws gwo".split(), (s, o) + tuple(g) + tuple(h)))


@gpu
@pytest.mark.parametrize("B,N,C", BOUNDARY_SHAPES)
def test_long_attn_core_at_its_geometry_switches_per_molecule(B, N, C):
    """dg_attn_core_long_fwd / _bwd / _bwd2 called directly (N <= 96 included) against the fp64 closed forms, molecule by
    molecule, so that a dropped, duplicated or misplaced molecule fails by name.  Outputs live in buffers padded to a
    multiple of 8 molecules and pre-filled with a sentinel: every molecule < B must be written, none past B.  The three
    launches run twice: when B N^2 reaches DG_EDGE_ROWS, consecutive launches alternate direction (csrc/traversal.h), so
    every kernel walks the molecules both ways."""
    from druggen_amd import _lib
    alpha = 1.0 / math.sqrt(max(C // 4, 1))
    ops64 = _operands(B, N, C)
    t64 = ops64[6]
    q, k, v, e, ws, wo = (x.float().cuda() for x in ops64[:6])
    tq, tk, tv, te = (x.float().cuda() for x in t64)
    lib = _lib.load()
    assert (lib.dg_attn_core_long_workspace_bytes(B, N, C) == 0) == (N <= 32)
    row, edge = (N, C), (N, N, C)
    runs = []
    for _ in range(2):
        out = dict(s=_guarded(B, edge), o=_guarded(B, row))
        out.update(dq=_guarded(B, row), dk=_guarded(B, row), dv=_guarded(B, row), de=_guarded(B, edge))
        out.update(gq=_guarded(B, row), gk=_guarded(B, row), gv=_guarded(B, row), ge=_guarded(B, edge),
                   gws=_guarded(B, edge), gwo=_guarded(B, row))
        _long_launch("fwd", q, k, v, e, out["s"], out["o"], B=B, N=N, C=C, alpha=alpha)
        _long_launch("bwd", q, k, v, e, ws, wo, None, *(out[n] for n in "dq dk dv de".split()), B=B, N=N, C=C, alpha=alpha)
        _long_launch("bwd2", q, k, v, e, ws, wo, tq, tk, tv, te, *(out[n] for n in "gq gk gv ge gws gwo".split()),
                     B=B, N=N, C=C, alpha=alpha)
        torch.cuda.synchronize()
        runs.append({n: x.cpu() for n, x in out.items()})
        del out
    for name in runs[0]:
        for r, run in enumerate(runs):
            guard = run[name][B:]
            assert bool((guard == SENTINEL).all()), f"{name}: written past molecule {B - 1} (run {r})"
    for b in range(B):
        want = _closed_forms_per_molecule(ops64[:6], t64, alpha, b)
        for name, ref in want.items():
            tol = TOL if name in ("s", "o", "dq", "dk", "dv", "de") else 5 * TOL
            for r, run in enumerate(runs):
                err = _rel(run[name][b:b + 1], ref)
                assert err < tol, f"molecule {b}: {name} rel err {err:.3g} (run {r})"


@gpu
def test_long_attn_core_without_score_output_and_null_ws():
    from druggen_amd import functional as dgf
    B, N, C, alpha = 2, 128, 64, 0.25
    q, k, v, e, _, wo, t = _operands(B, N, C)
    _, o_ref = km.attn_core_fwd(q, k, v, e, alpha)
    g_ref = km.attn_core_bwd(q, k, v, e, torch.zeros_like(e), wo, alpha)
    h_ref = km.attn_core_bwd2(q, k, v, e, torch.zeros_like(e), wo, *t, alpha)
    f = lambda x: x.float().cuda().requires_grad_(True)
    qd, kd, vd, ed = map(f, (q, k, v, e))
    s, o = dgf.attn_core(qd, kd, vd, ed, alpha, need_s=False)
    assert s is None and _rel(o, o_ref) < TOL
    grads = torch.autograd.grad(o, [qd, kd, vd, ed], wo.float().cuda(), create_graph=True)
    for got, want in zip(grads, g_ref):
        assert _rel(got, want) < TOL
    phi = sum((g * tt.float().cuda()).sum() for g, tt in zip(grads, t))
    second = torch.autograd.grad(phi, [qd, kd, vd, ed])
    for got, want in zip(second, h_ref[:4]):
        assert _rel(got, want) < 5 * TOL


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N,C", [(2, 128, 128), (1, 129, 128), (1, 193, 128)])   # 8-quad, 4-quad (N > 128) backward slices
def test_long_attn_core_backward_adds_an_outside_adjoint_of_e(B, N, C, dtype):
    from druggen_amd import functional as dgf
    f = lambda shape, s, sc=1.0: (_gen(shape, s) * sc).to(dtype).cuda()
    q, k, v, wo = f((B, N, C), 1), f((B, N, C), 2), f((B, N, C), 3), f((B, N, C), 6)
    e, ws, ae = f((B, N, N, C), 4, 0.8), f((B, N, N, C), 5), f((B, N, N, C), 11, 0.5)
    plain = dgf._attn_bwd_launch(q, k, v, e, ws, wo, 0.25)
    fused = dgf._attn_bwd_launch(q, k, v, e, ws, wo, 0.25, add_e=ae)
    for a, b in zip(plain[:3], fused[:3]):
        assert torch.equal(a, b)
    tol = 1e-6 if dtype == torch.float32 else 4e-3
    assert _rel(fused[3], plain[3].double() + ae.double()) < tol
    p2 = dgf._attn_bwd_launch(q, k, v, e, None, wo, 0.25)
    f2 = dgf._attn_bwd_launch(q, k, v, e, None, wo, 0.25, add_e=ae)
    assert _rel(f2[3], p2[3].double() + ae.double()) < tol


# ------------------------------------------------------------------------------- long vs short entries
@gpu
@pytest.mark.parametrize("B,N,C", [(3, 45, 128), (1, 90, 128), (2, 45, 12), (1, 33, 8), (1, 49, 16)])
def test_long_entries_match_the_short_ones_where_both_run(B, N, C):
    from druggen_amd import functional as dgf
    alpha = 0.25
    ops = [x.float().cuda() for x in _operands(B, N, C)[:6]]
    q, k, v, e, ws, wo = ops
    tq, tk, tv, te = (x.float().cuda() for x in _operands(B, N, C)[6])
    like = lambda x: torch.empty_like(x)
    # forward
    s0, o0 = dgf.attn_core(q, k, v, e, alpha)
    s1, o1 = like(e), like(q)
    _long_launch("fwd", q, k, v, e, s1, o1, B=B, N=N, C=C, alpha=alpha)
    assert _rel(s1, s0) < TOL_SHORT and _rel(o1, o0) < TOL_SHORT
    # first order, with and without add_e
    for add in (None, _gen((B, N, N, C), 11).float().cuda()):
        short = dgf._attn_bwd_launch(q, k, v, e, ws, wo, alpha, add_e=add)
        got = [like(q), like(q), like(q), like(e)]
        _long_launch("bwd", q, k, v, e, ws, wo, add, *got, B=B, N=N, C=C, alpha=alpha)
        for name, a, b in zip("dq dk dv de".split(), got, short):
            assert _rel(a, b) < TOL_SHORT, name
    # second order
    short = dgf._attn_bwd2_launch(q, k, v, e, ws, wo, tq, tk, tv, te, alpha)
    got = [like(q), like(q), like(q), like(e), like(e), like(q)]
    _long_launch("bwd2", q, k, v, e, ws, wo, tq, tk, tv, te, *got, B=B, N=N, C=C, alpha=alpha)
    for name, a, b in zip("gq gk gv ge gws gwo".split(), got, short):
        assert _rel(a, b) < TOL_SHORT2, name


# ---------------------------------------------------------------------------------------- reproducibility
@gpu
@pytest.mark.parametrize("B,N,C", [(4, 128, 128), (9, 193, 32)])
def test_long_attn_core_is_bit_reproducible_in_both_directions(B, N, C):
    """B N^2 >= 65536 rows: every launch is edge-level, so consecutive launches walk the molecules in opposite directions
    (csrc/traversal.h); three launches per repetition put each kernel on both directions across the repetitions.  B = 9:
    the reverse walk mirrors over the padded count of 16 molecules."""
    from druggen_amd import functional as dgf
    alpha = 0.25
    f = lambda shape, s: _gen(shape, s).float().cuda().requires_grad_(True)
    q, k, v, e = f((B, N, C), 1), f((B, N, C), 2), f((B, N, C), 3), f((B, N, N, C), 4)
    ws, wo = f((B, N, N, C), 5), f((B, N, C), 6)
    t = [_gen((B, N, C), 7 + i).float().cuda() for i in range(3)] + [_gen((B, N, N, C), 10).float().cuda()]
    outs = []
    for _ in range(3):
        s, o = dgf.attn_core(q, k, v, e, alpha)
        g = torch.autograd.grad([s, o], [q, k, v, e], [ws, wo], create_graph=True)
        phi = sum((a * b).sum() for a, b in zip(g, t))
        h = torch.autograd.grad(phi, [q, k, v, e, ws, wo])
        outs.append([s.detach().clone(), o.detach().clone()] + [x.detach().clone() for x in g] + [x.clone() for x in h])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------- bf16 vs fp32
@gpu
@pytest.mark.parametrize("B,N,C", [(2, 128, 128), (9, 193, 32), (9, 256, 32)])
def test_long_attn_core_bf16_against_float32(B, N, C):
    from druggen_amd import functional as dgf
    alpha = 0.25
    base = [x.to(torch.bfloat16) for x in _operands(B, N, C)[:6]]
    tb = [x.to(torch.bfloat16) for x in _operands(B, N, C)[6]]
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        q, k, v, e, ws, wo = (x.to(dt).cuda().requires_grad_(True) for x in base)
        s, o = dgf.attn_core(q, k, v, e, alpha)
        g = torch.autograd.grad([s, o], [q, k, v, e], [ws, wo], create_graph=True)
        phi = sum((a * b.to(dt).cuda()).sum() for a, b in zip(g, tb))
        h = torch.autograd.grad(phi, [q, k, v, e, ws, wo])
        res[dt] = ([s, o] + list(g), list(h))
    for a, b in zip(res[torch.bfloat16][0], res[torch.float32][0]):
        assert a.dtype == torch.bfloat16 and _rel(a, b) < TOL_IO
    for a, b in zip(res[torch.bfloat16][1], res[torch.float32][1]):
        assert _rel(a, b) < 2 * TOL_IO
    for m in range(B):      # molecule by molecule
        for tol, got, want in ((TOL_IO, res[torch.bfloat16][0], res[torch.float32][0]),
                               (2 * TOL_IO, res[torch.bfloat16][1], res[torch.float32][1])):
            for i, (a, b) in enumerate(zip(got, want)):
                err = _rel(a[m], b[m])
                assert err < tol, f"molecule {m}: output {i} rel err {err:.3g}"


# ----------------------------------------------------------------------------------------------- limits
@gpu
def test_above_256_neighbours_fails_with_a_clear_error():
    from druggen_amd import _lib
    from druggen_amd import functional as dgf
    from druggen_amd.model import Generator
    B, N, C = 1, 257, 16
    x = torch.zeros(B, N, C, device="cuda")
    e = torch.zeros(B, N, N, C, device="cuda")
    with pytest.raises(RuntimeError, match="maximum of 256"):
        dgf.attn_core(x, x, x, e, 0.5)
    G = Generator("relu", N, 5, 13, 0.0, dim=16, depth=1, heads=4, mlp_ratio=2).cuda()
    with pytest.raises(RuntimeError, match="maximum of 256"):
        G(torch.zeros(B, N, N, 5, device="cuda"), torch.zeros(B, N, 13, device="cuda"))
    lib = _lib.load()
    st = lib.dg_attn_core_long_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), e.data_ptr(), e.data_ptr(), x.data_ptr(),
                                   B, N, C, 0.5, 0, None)
    assert st == -1 and b"unsupported shape" in lib.dg_last_error_string()


def test_long_entries_validate_arguments_without_a_gpu():
    from druggen_amd import _lib
    lib = _lib.load()
    for name in ("dg_attn_core_long_fwd", "dg_attn_core_long_bwd", "dg_attn_core_long_bwd2",
                 "dg_attn_core_long_workspace_bytes"):
        assert hasattr(lib, name), name
    fake = 1 << 20      # never dereferenced: every call below fails before it enqueues anything
    assert lib.dg_attn_core_long_fwd(None, None, None, None, None, None, 1, 128, 128, 0.25, 0, None) == -2
    assert b"null pointer" in lib.dg_last_error_string()
    assert lib.dg_attn_core_long_bwd(*[None] * 12, 0, 1, 128, 128, 0.25, 0, None) == -2
    assert lib.dg_attn_core_long_bwd2(*[None] * 17, 0, 1, 128, 128, 0.25, 0, None) == -2
    for N in (0, 257):
        assert lib.dg_attn_core_long_fwd(*[fake] * 6, 1, N, 128, 0.25, 0, None) == -1
        assert b"unsupported shape" in lib.dg_last_error_string()
        assert lib.dg_attn_core_long_bwd(*[fake] * 12, 1 << 30, 1, N, 128, 0.25, 0, None) == -1
        assert lib.dg_attn_core_long_bwd2(*[fake] * 17, 1 << 30, 1, N, 128, 0.25, 0, None) == -1
    assert lib.dg_attn_core_long_fwd(*[fake] * 6, 1, 128, 6, 0.25, 0, None) == -1     # C % 4 != 0
    need = lib.dg_attn_core_long_workspace_bytes(2, 128, 128)
    assert need > 0 and lib.dg_attn_core_long_workspace_bytes(2, 32, 128) == 0
    for B, C in ((1, 8), (9, 48), (17, 128)):    # one row group (no column partials) exactly up to 32 neighbours
        for N in range(1, 257):
            assert (lib.dg_attn_core_long_workspace_bytes(B, N, C) == 0) == (N <= 32), (B, N, C)
    assert lib.dg_attn_core_long_bwd(*[fake] * 12, need - 1, 2, 128, 128, 0.25, 0, None) == -3
    assert b"workspace too small" in lib.dg_last_error_string()
    assert lib.dg_attn_core_long_bwd2(*[fake] * 16, None, need, 2, 128, 128, 0.25, 0, None) == -3
    assert lib.dg_attn_core_long_bwd2(*[fake] * 17, need - 1, 2, 128, 128, 0.25, 0, None) == -3


# ----------------------------------------------------------------------------------- end to end vs fp64
@gpu
def test_vertexes_128_two_layers_against_fp64_oracle():
    """D step and G step at N = 128 (E = 5, M = 13, L = 2, B = 3): losses at 1e-3, every gradient tensor at 1e-3."""
    cfg = orc.NetConfig(act="relu", vertexes=128, edges=5, nodes=13, dropout=0.0, dim=128, depth=2, heads=8, mlp_ratio=3)
    print("worst per-tensor error", thm._step_against_fp64_oracle(cfg, 3, 501, with_g_step=True))


@gpu
def test_vertexes_256_one_layer_against_fp64_oracle():
    cfg = orc.NetConfig(act="relu", vertexes=256, edges=5, nodes=13, dropout=0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
    print("worst per-tensor error", thm._step_against_fp64_oracle(cfg, 1, 511, with_g_step=False))


# --------------------------------------------------------------------------------------- training at size
def _nets(N, depth, seed):
    from druggen_amd.model import Discriminator, Generator
    torch.manual_seed(seed)
    kw = dict(dim=128, depth=depth, heads=8, mlp_ratio=3)
    return (Generator("relu", N, 5, 13, 0.0, **kw).cuda(), Discriminator("relu", N, 5, 13, 0.0, **kw).cuda())


def _batch(B, N, seed):
    from druggen_amd import synth
    a, x, _, _ = synth.molecule_batch(B, N, 5, 13, seed=seed)
    return torch.from_numpy(a).cuda(), torch.from_numpy(x).cuda()


def _eps(B):
    return (torch.rand(B, 1, 1, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)),
            torch.rand(B, 1, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)))


@gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_gan_step_at_128_atoms_is_finite_and_reproducible(dtype):
    from druggen_amd import functional as dgf
    from druggen_amd.trainer import GANStep
    B, N = 16, 128
    a, x = _batch(B, N, 21)
    da, dx = _batch(B, N, 22)
    eps = _eps(B)
    runs = []
    with dgf.activations(dtype):
        for _ in range(2):
            G, D = _nets(N, 2, seed=7)
            st = GANStep(G, D, lambda_gp=10.0)
            d_loss, g_loss = st.step(da, dx, a, x, eps=eps)
            assert torch.isfinite(d_loss) and torch.isfinite(g_loss)
            runs.append((float(d_loss), float(g_loss),
                         torch.cat([p.detach().reshape(-1) for p in list(G.parameters()) + list(D.parameters())]).clone()))
            del st, G, D
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2], runs[1][2])


@gpu
def test_graphed_step_equals_eager_step_at_128_atoms():
    """As tests/test_hip_aux.py::test_graphed_step_equals_eager_step (N = 45), at N = 128."""
    from druggen_amd.model import discriminator_loss
    from druggen_amd.trainer import GANStep, GraphedGANStep
    B, N = 4, 128
    a, x = _batch(B, N, 31)
    da, dx = _batch(B, N, 32)
    eps = _eps(B)
    fixed_eps = lambda *args, **kw: discriminator_loss(*args, **{**kw, "eps": eps})
    outs = []
    for graphed in (False, True):
        G, D = _nets(N, 2, seed=9)
        st = GANStep(G, D, lambda_gp=10.0, d_loss_fn=fixed_eps, share_generator_forward=False)
        if graphed:
            gs = GraphedGANStep(st, da, dx, a, x, warmup=2)
            for _ in range(2):
                gs.step(da, dx, a, x)
        else:
            for _ in range(4):
                st.step(da, dx, a, x)
        torch.cuda.synchronize()
        outs.append([p.detach().clone() for p in list(G.parameters()) + list(D.parameters())])
    worst, mean = 0.0, 0.0
    for p, r in zip(*outs):
        d = (p - r).abs()
        worst, mean = max(worst, d.max().item()), mean + d.mean().item() / len(outs[0])
    assert worst <= 8.5e-5 and mean <= 2e-6, (worst, mean)
