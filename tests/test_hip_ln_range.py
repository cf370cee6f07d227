"""Every hand-written LayerNorm of csrc/ on constant, offset and wide-range rows (tests/ln_cases.py): the seven forward
copies and the six backward copies against tests/kernel_math.py in float64 on the CPU, each row held to its own bar, every
planted row named in the failure message, no row and no element left out.  The GEMM part of a fused copy is nulled (zero
operand or zero weights), so that its pre-LayerNorm sum IS the planted matrix, bit for bit -- asserted first.

Every test prints the worst error / (u x bound) it measured per quantity (the bar is K = 16)."""
import pytest
import torch

import attn_range_cases as acr
import ln_cases as lc

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
R0 = 67
ALL = lc.FORWARD + lc.FIRST + lc.SECOND


def _dgf():
    from druggen_amd import functional as dgf
    return dgf


def _place(t, dtype, offset=False):
    """The float64 CPU tensor on the GPU in ``dtype``; ``offset``: as ``flat[4:]`` of a buffer four elements longer."""
    if not offset:
        return t.to(dtype).cuda().contiguous()
    buf = torch.empty(t.numel() + 4, dtype=dtype, device="cuda")
    out = buf[4:].view(t.shape)
    out.copy_(t.to(dtype))
    return out


def _hold(copy, label, got, want, bound, where, quantities):
    worst = {}
    bad = lc.failures(f"{copy} {label}", got, want, bound, where, quantities, worst=worst)
    lc.report(f"[{copy}] {label}", worst)
    assert not bad, "\n".join(bad)


def _gen(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


# ------------------------------------------------------------------------------------------------ a. stand-alone kernels
def _ln_residual_all_orders(z, gamma, beta, dy, tz, dtype, with_residual, seed, offset=False):
    """dgf.ln_residual forward, backward and second order (dg_ln_residual_fwd / _bwd_add / _bwd2) -> (got, want, bound)."""
    dgf = _dgf()
    summed = None
    if with_residual:
        a, r, z = lc.split_residual(z, seed, dtype)
        summed = (a, r)
    else:
        a, r = z, None
    want = lc.reference(z, gamma, beta, dy, tz)
    bound = lc.bounds(z, gamma, beta, dy, tz, summed=summed)
    ad = _place(a, dtype, offset).requires_grad_(True)
    rd = _place(r, dtype, offset).requires_grad_(True) if with_residual else None
    gd, bd = _place(gamma, F32).requires_grad_(True), _place(beta, F32).requires_grad_(True)
    dyd = _place(dy, dtype, offset).requires_grad_(True)
    tzd = _place(tz, dtype, offset)
    y = dgf.ln_residual(ad, rd, gd, bd, lc.EPS)
    sv = y.grad_fn.saved_tensors
    ins = [ad, gd, bd] + ([rd] if with_residual else [])
    grads = torch.autograd.grad(y, ins, dyd, create_graph=True)
    if with_residual:
        assert torch.equal(grads[3], grads[0])
    gz, gg, gdy = torch.autograd.grad((grads[0] * tzd).sum(), [ad, gd, dyd])
    got = dict(y=y.detach(), mean=sv[3], rstd=sv[4], dz=grads[0].detach(), dgamma=grads[1].detach(), dbeta=grads[2].detach(),
               gz=gz, ggamma=gg, gdy=gdy)
    return got, want, bound


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("C", lc.WIDTHS)
def test_ln_residual_all_orders_on_planted_rows(C, with_residual):
    """layernorm.hip in float32: one, two, three (dispatched as four, the last slot masked wholly or in part) and four quads
    per lane, C = 4 (seven of eight group lanes masked), a partly filled second slot (260)."""
    seed = C + int(with_residual)
    z, where = lc.plant(R0, C, seed)
    gamma, beta, dy, tz = lc.operands(R0, C, seed)
    got, want, bound = _ln_residual_all_orders(z, gamma, beta, dy, tz, F32, with_residual, seed)
    _hold("layernorm.hip f32", f"C={C} residual={with_residual}", got, want, bound, where, ALL)


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("C", [32, 128])
def test_ln_residual_all_orders_on_planted_rows_bf16(C, with_residual):
    """bf16 rows (the rows are rounded to bf16 first; the reference sees the rounded values).  C = 128: the backward and the
    second order take the PAIR instance (eight consecutive channels per lane)."""
    seed = C + int(with_residual)
    z, where = lc.plant(R0, C, seed, BF)
    gamma, beta, dy, tz = lc.operands(R0, C, seed, BF)
    got, want, bound = _ln_residual_all_orders(z, gamma, beta, dy, tz, BF, with_residual, seed)
    assert got["y"].dtype == BF and got["dz"].dtype == BF and got["gz"].dtype == BF
    _hold("layernorm.hip bf16" + (" PAIR" if C == 128 else ""), f"C={C} residual={with_residual}", got, want, bound, where, ALL)


@pytest.mark.parametrize("with_residual", [False, True])
def test_ln_bf16_rows_off_16_byte_alignment_take_the_generic_instance(with_residual):
    """C = 128 in bf16 with every activation at an 8-byte offset: the 16-byte accesses of the PAIR instance are not possible,
    the generic <bf16, 32, 1> instance runs.  The same bars, and agreement with the PAIR result to 2^-8 of each row
    (ln_cases.row_rel)."""
    C = 128
    seed = C + int(with_residual)
    z, where = lc.plant(R0, C, seed, BF)
    gamma, beta, dy, tz = lc.operands(R0, C, seed, BF)
    got, want, bound = _ln_residual_all_orders(z, gamma, beta, dy, tz, BF, with_residual, seed, offset=True)
    _hold("layernorm.hip bf16 generic", f"C={C} residual={with_residual} offset", got, want, bound, where, ALL)
    pair, _, _ = _ln_residual_all_orders(z, gamma, beta, dy, tz, BF, with_residual, seed)
    for q in ("dz", "gz", "gdy"):
        rel = lc.row_rel(got[q], pair[q])
        print(f"generic against PAIR {q}: worst row {float(rel.max()):.3g}")
        assert float(rel.max()) <= 2.0 ** -8, (q, int(rel.argmax()), where.get(int(rel.argmax()), "normal"))
    # (16 against 32 lanes per row: the float32 column sums of the two instances differ in their last bits)
    print("generic against PAIR dgamma: max |difference| = "
          f"{float((got['dgamma'].double() - pair['dgamma'].double()).abs().max()):.3g}")
    for q in ("y", "mean", "rstd"):      # the forward has one instance: the same arithmetic at either alignment
        assert torch.equal(got[q], pair[q]), q


# ------------------------------------------------------------------------------------------------ b. grid-stride
@pytest.mark.parametrize("R,C", [(4099, 256), (8197, 128)])
def test_ln_grid_stride_with_a_ragged_last_pass(R, C):
    """More than 1024 passes (R > 1024 * 256 / G): pass 1024 is the ragged last one (3 rows of 4 at C = 256, 5 of 8 at
    C = 128) and block 0's second trip.  The named rows fill that pass, a chunk at a time, and the same names sit in block 0's
    first trip; dgamma, dbeta and ggamma go through the finish over 1024 partials (its 8-wide unrolled loop)."""
    G = C // 4
    rpb = 256 // G
    assert (R + rpb - 1) // rpb == 1025 and R % rpb != 0
    tail = R - 1024 * rpb
    gamma, beta, dy, tz = lc.operands(R, C, R)
    for k in range(0, len(lc.NAMES), tail):
        names = lc.NAMES[k:k + tail]
        positions = [R - tail + i for i in range(len(names))] + list(range(len(names)))
        z, where = lc.plant(R, C, R + k, positions=positions, names=names)
        got, want, bound = _ln_residual_all_orders(z, gamma, beta, dy, tz, F32, False, R + k)
        _hold("layernorm.hip f32 grid-stride", f"R={R} C={C} {'+'.join(names)}", got, want, bound, where, ALL)


# ------------------------------------------------------------------------------------------------ d. dz_add
def _given(R, C, seed, dtype=F32):
    """Planted rows with the statistics a backward copy is given: float64 mean / rstd rounded to float32."""
    z, where = lc.plant(R, C, seed, dtype)
    gamma, beta, dy, tz = lc.operands(R, C, seed, dtype)
    stats = lc.round_stats(z)
    want = lc.reference(z, gamma, beta, dy, tz, stats=stats)
    bound = lc.bounds(z, gamma, beta, dy, tz, stats=stats)
    d = dict(pre=_place(z, dtype), gamma=_place(gamma, F32), mean=_place(stats[0].squeeze(-1), F32),
             rstd=_place(stats[1].squeeze(-1), F32), dy=_place(dy, dtype), tz=_place(tz, dtype))
    return d, where, want, bound


@pytest.mark.parametrize("C", [128, 384])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_ln_backward_dz_add_is_the_plain_backward_plus_one_add(C, dtype):
    """dg_ln_residual_bwd_add with a second gradient source: in float32 bit-equal to the launch without it followed by one
    elementwise add (the contract in the kernel's comment); in bf16, where the fused form rounds once and the two-step form
    twice, equal to 2^-8 of each row (ln_cases.row_rel)."""
    dgf = _dgf()
    d, where, _, _ = _given(R0, C, 7 * C, dtype)
    t = _place(_gen((R0, C), 5), dtype)
    plain = dgf._ln_bwd_rows(d["pre"], d["gamma"], d["mean"], d["rstd"], d["dy"])
    fused = dgf._ln_bwd_rows(d["pre"], d["gamma"], d["mean"], d["rstd"], d["dy"], dz_add=t)
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[2], plain[2])
    assert bool(torch.isfinite(fused[0].float()).all())
    if dtype == F32:
        diff = torch.nonzero((fused[0] != plain[0] + t).any(1)).flatten().tolist()
        assert not diff, [(r, where.get(r, "normal")) for r in diff]
    else:
        rel = lc.row_rel(fused[0], plain[0] + t)
        print(f"dz_add bf16 C={C}: worst row {float(rel.max()):.3g}")
        assert float(rel.max()) <= 2.0 ** -8, (int(rel.argmax()), where.get(int(rel.argmax()), "normal"))


# ------------------------------------------------------------------------------------------------ e. fused forward copies
def _forward_case(R, seed, dtype=F32):
    C = 128
    z, where = lc.plant(R, C, seed, dtype)
    gamma, beta, _, _ = lc.operands(R, C, seed, dtype)
    return z, where, gamma, beta, lc.reference(z, gamma, beta), lc.bounds(z, gamma, beta)


def _hold_forward(copy, label, z, where, want, bound, y, mean, rstd, pre):
    zd = z.to(pre.dtype)
    diff = torch.nonzero((pre.cpu() != zd).any(1)).flatten().tolist()
    assert torch.equal(pre.cpu(), zd), f"{copy} {label}: pre differs from the planted rows in " \
                                      f"{[(r, where.get(r, 'normal')) for r in diff]}"
    _hold(copy, label, dict(y=y, mean=mean.reshape(-1), rstd=rstd.reshape(-1)), want, bound, where, lc.FORWARD)


@pytest.mark.parametrize("K,R,dtype", [(128, R0, F32), (384, R0, F32), (384, 16 * 5 + 1, F32), (128, R0, BF)],
                         ids=["row_gemm", "row_gemm_k384", "row_gemm_k384-R81", "gemm_bf16"])
def test_row_gemm_layernorm_epilogue_on_planted_rows(K, R, dtype):
    """The LayerNorm epilogues of row_gemm.hip (128 -> 128), row_gemm_k384.hip (384 -> 128; R = 67 and 16 * 5 + 1) and
    gemm_bf16.hip: a zero A operand and a zero bias, the planted matrix as the residual."""
    dgf = _dgf()
    N = 128
    z, where, gamma, beta, want, bound = _forward_case(R, K + R, dtype)
    packed = dgf.packed_weight(_place(_gen((N, K), 3, 0.1), F32), 0, dtype)
    a2 = torch.zeros(R, K, dtype=dtype, device="cuda")
    run = lambda: dgf.row_gemm(a2, packed, K, N, bias=torch.zeros(N, device="cuda"), residual=_place(z, dtype),
                               ln=(_place(gamma, F32), _place(beta, F32), lc.EPS), want_pre=True)
    y, mean, rstd, pre = run()
    copy = {(128, F32): "row_gemm.hip", (384, F32): "row_gemm_k384.hip", (128, BF): "gemm_bf16.hip"}[(K, dtype)]
    _hold_forward(copy, f"R={R}", z, where, want, bound, y, mean, rstd, pre)
    assert all(torch.equal(a_, b_) for a_, b_ in zip((y, mean, rstd, pre), run()))


def _ffn_inputs(z, gamma, beta, dtype):
    """x = the planted rows, fc1 random, fc2 = 0 with a zero bias: the pre-LayerNorm sum is x."""
    C, H = 128, 384
    f = lambda t, dt=F32: _place(t, dt).requires_grad_(True)
    return [f(z, dtype), f(_gen((H, C), 11, 0.1)), f(_gen((H,), 12, 0.1)), f(torch.zeros(C, H, dtype=torch.float64)),
            f(torch.zeros(C, dtype=torch.float64)), f(gamma), f(beta)]


def _ffn_run(node, ins, dyd):
    """-> (y, pre, mean, rstd, dx, dgamma, dbeta) of one feed-forward node class on ``ins``."""
    out = node.apply(*ins, lc.EPS)
    if isinstance(out, tuple):
        y, pre, mean, rstd = out
    else:
        y, sv = out, out.grad_fn.saved_tensors
        pre, mean, rstd = sv[7], sv[8], sv[9]
    dx, dg, db = torch.autograd.grad(y, [ins[0], ins[5], ins[6]], dyd)
    return y.detach(), pre.detach(), mean, rstd, dx, dg, db


FFN_COPIES = ["ffn_fused_f32", "row_gemm_k384-two-launch", "gemm_bf16-two-launch", "ffn_bf16"]


@pytest.mark.parametrize("copy", FFN_COPIES)
def test_feed_forward_layernorm_forward_and_backward_on_planted_rows(copy):
    """LN(x + fc2(relu(fc1 x))) with fc2 = 0: _FFNLN in float32 on the fused forward (ffn_fused_f32.hip) and on the two
    row-GEMM launches, _FFNLN under the bf16 activation dtype (the two launches of gemm_bf16.hip) and the fused bf16 node
    (ffn_bf16.hip).  Forward: pre == x bit for bit, then y, mean, rstd to the bars.  Backward (the feed-forward backward
    kernels, float32 and bf16): dh = dz W2 = 0, so dx IS the LayerNorm input gradient -- dx, dgamma, dbeta to the dz, dgamma,
    dbeta bars, repeated launches bit-identical."""
    dgf = _dgf()
    from druggen_amd.options import options
    dtype = BF if copy in ("gemm_bf16-two-launch", "ffn_bf16") else F32
    node = dgf._FFNLNFusedBF16 if copy == "ffn_bf16" else dgf._FFNLN
    R, C = R0, 128
    seed = 40 + FFN_COPIES.index(copy)
    z, where = lc.plant(R, C, seed, dtype)
    gamma, beta, dy, _ = lc.operands(R, C, seed, dtype)
    want, bound = lc.reference(z, gamma, beta, dy), lc.bounds(z, gamma, beta, dy)
    ins = _ffn_inputs(z, gamma, beta, dtype)
    dyd = _place(dy, dtype)
    prev_fused = options.ffn_f32 == "fused"      # (the shipped choice comes back)
    try:
        dgf.set_fused_ffn_f32(copy == "ffn_fused_f32")
        y, pre, mean, rstd, dx, dg, db = _ffn_run(node, ins, dyd)
        again = _ffn_run(node, ins, dyd)
    finally:
        dgf.set_fused_ffn_f32(prev_fused)
    assert y.dtype == dtype and dx.dtype == dtype
    fwd_name = {"ffn_fused_f32": "ffn_fused_f32.hip", "row_gemm_k384-two-launch": "row_gemm_k384.hip via _FFNLN",
                "gemm_bf16-two-launch": "gemm_bf16.hip K=384 via _FFNLN", "ffn_bf16": "ffn_bf16.hip"}[copy]
    _hold_forward(fwd_name, "forward", z, where, want, bound, y.view(R, C), mean, rstd, pre.view(R, C))
    # the backward reads the forward's own statistics: the bars cover their error (kappa)
    _hold("feed-forward backward " + ("bf16" if copy == "ffn_bf16" else f"{'bf16 rows' if dtype == BF else 'f32'} after {copy}"),
          "dx dgamma dbeta", dict(dz=dx.view(R, C), dgamma=dg, dbeta=db), want, bound, where, lc.FIRST)
    assert all(torch.equal(a_, b_) for a_, b_ in zip((y, pre, mean, rstd, dx, dg, db), again))


def test_attention_half_layernorm_on_planted_rows():
    """dg_attn_half_f32_fwd (attn_half_f32.hip) with Woe = 0, boe = 0: B = 1, N = 9, the 81 edge rows y are the planted matrix,
    random q, k, v, We."""
    B, N, C = 1, 9, 128
    R = B * N * N
    z, where, gamma, beta, want, bound = _forward_case(R, 81)
    h = acr.half_case("normal", B, N)
    h.update(y=z.view(B, N, N, C), Woe=torch.zeros(C, C, dtype=torch.float64), boe=torch.zeros(C, dtype=torch.float64),
             g4=gamma, b4=beta)
    x = acr.half_to_gpu(h, F32)
    out = acr.run_half_f32_fwd(x, B, N, lc.EPS)
    f = lambda n: out[n][:B].reshape(R, -1)
    assert all(acr.all_written(out[n], B) and acr.guard_untouched(out[n], B) for n in ("y2", "pre", "mean", "rstd"))
    _hold_forward("attn_half_f32.hip", "B=1 N=9", z, where, want, bound, f("y2"), f("mean"), f("rstd"), f("pre"))
    again = acr.run_half_f32_fwd(x, B, N, lc.EPS)
    assert all(torch.equal(out[n], again[n]) for n in ("y2", "pre", "mean", "rstd"))


# ------------------------------------------------------------------------------------------------ f. backward copies
def test_ln_backward_kernels_on_given_statistics():
    """dg_ln_residual_bwd_add and dg_ln_residual_bwd2 through _ln_bwd_rows / _ln_bwd2_rows at C = 128, float32."""
    dgf = _dgf()
    d, where, want, bound = _given(R0, 128, 61)
    run1 = lambda: dgf._ln_bwd_rows(d["pre"], d["gamma"], d["mean"], d["rstd"], d["dy"])
    run2 = lambda: dgf._ln_bwd2_rows(d["pre"], d["gamma"], d["mean"], d["rstd"], d["dy"], d["tz"])
    dz, dg, db = (t.clone() for t in run1())
    gz, gdy, gg = (t.clone() for t in run2())
    _hold("dg_ln_residual_bwd_add", "given statistics", dict(dz=dz, dgamma=dg, dbeta=db), want, bound, where, lc.FIRST)
    _hold("dg_ln_residual_bwd2", "given statistics", dict(gz=gz, gdy=gdy, ggamma=gg), want, bound, where, lc.SECOND)
    assert all(torch.equal(a_, b_) for a_, b_ in zip((dz, dg, db), run1()))
    assert all(torch.equal(a_, b_) for a_, b_ in zip((gz, gdy, gg), run2()))


@pytest.mark.parametrize("R", [R0, 200])
def test_row_gemm_layernorm_backward_epilogue_on_given_statistics(R):
    """dg_row_gemm_ln_bwd with a zero A operand and dy as the residual: the output gradient that reaches the epilogue is
    exactly dy."""
    dgf = _dgf()
    d, where, want, bound = _given(R, 128, 62 + R)
    packed = dgf.packed_weight(_place(_gen((128, 128), 4, 0.1), F32), 1)
    a2 = torch.zeros(R, 128, device="cuda")
    run = lambda: dgf.row_gemm_ln_bwd(a2, packed, 128, d["dy"], d["pre"], d["gamma"], d["mean"], d["rstd"])
    dz, dg, db = (t.clone() for t in run())
    _hold("dg_row_gemm_ln_bwd", f"R={R}", dict(dz=dz, dgamma=dg, dbeta=db), want, bound, where, lc.FIRST)
    assert all(torch.equal(a_, b_) for a_, b_ in zip((dz, dg, db), run()))


@pytest.mark.parametrize("R", [R0, 200])
def test_row_gemm_layernorm_backward_prologue_on_given_statistics(R):
    """dg_row_gemm_ln_bwd_in: dz to the bar; y = dz W against the kernel's own dz in float64 at 1e-6 (|dz| |W|), the bar of
    test_row_gemm_split_edge_rows."""
    dgf = _dgf()
    d, where, want, bound = _given(R, 128, 63 + R)
    w = lc.rounded(_gen((128, 128), 5, 0.1))
    packed = dgf.packed_weight(_place(w, F32), 1)
    run = lambda: dgf.ln_bwd_row_gemm(d["pre"], d["gamma"], d["mean"], d["rstd"], d["dy"], packed)
    dz, y, dg, db = (t.clone() for t in run())
    _hold("dg_row_gemm_ln_bwd_in", f"R={R}", dict(dz=dz, dgamma=dg, dbeta=db), want, bound, where, lc.FIRST)
    dzd = dz.double().cpu()
    assert bool(torch.isfinite(y).all())
    err = (y.double().cpu() - dzd @ w).abs() / (dzd.abs() @ w.abs()).clamp_min(1e-300)
    print(f"dg_row_gemm_ln_bwd_in R={R}: y against dz W, worst error / (|dz| |W|) = {float(err.max()):.3g}")
    bad = torch.nonzero((err > 1e-6).any(1)).flatten().tolist()
    assert not bad, [(r, where.get(r, "normal"), float(err[r].max())) for r in bad]
    assert all(torch.equal(a_, b_) for a_, b_ in zip((dz, y, dg, db), run()))
