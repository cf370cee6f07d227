"""CPU checks of tests/bf16_cases.py, the cases and bars of tests/test_hip_bf16_elements.py: (1) the exact cases are exact by
construction -- every storage point of the float64 evaluation equals its own bf16 round trip, for several seeds, and the cases
are not degenerate; (2) a plain float32 restatement of every operation sits inside its bar, with a factor 2 to spare on every term but the
output rounding itself; (3) wrong
restatements with ONE planted error land outside the element-wise bar while passing the norm-wise 4e-3 of
tests/test_hip_bf16.py on the same data; (4) dropping or doubling one planted row of a weight gradient breaks its bar by more
than a factor 10.  Run with -s for the figures."""
import pytest
import torch

import bf16_cases as bc

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("R,K,N", [(257, 128, 128), (257, 128, 384), (65, 384, 128), (4133, 384, 128)])
def test_row_gemm_exact_case_is_exact_at_every_storage_point(R, K, N, seed):
    c = bc.gemm_exact_case(R, K, N, seed)
    assert int(c["w"].abs().sum(1).max()) == bc.NNZ_GEMM == int(c["w"].abs().sum(1).min())
    points = {"a": c["a"], "w": c["w"], "residual": c["residual"], "a2": c["a2"], "w2": c["w2"]}
    plain, _ = bc.gemm_chain(c["a"], c["w"], store=False)
    biased, z = bc.gemm_chain(c["a"], c["w"], c["bias"], store=False)
    act, _ = bc.gemm_chain(c["a"], c["w"], c["bias"], relu=True, store=False)
    masked, _ = bc.gemm_chain(c["a2"], c["w2"], mask=(z > 0), store=False)
    summed, _ = bc.gemm_chain(c["a"], c["w"], c["bias"], residual=c["residual"], store=False)
    points.update(plain=plain, biased=biased, relu=act, masked=masked, residual_sum=summed)
    for name, t in points.items():
        assert bc.holds(t), name
        assert float(t.abs().max()) <= 2 * bc.NNZ_GEMM + 7, name
    assert torch.equal(c["bias"].float().double(), c["bias"])
    if N == 128:      # the LayerNorm epilogue's width: the mean is a multiple of 1/128 below 2^8
        mean = summed.mean(-1)
        assert torch.equal(mean.float().double(), mean)
    positive = float((z > 0).double().mean())
    assert 0.2 <= positive <= 0.8, positive
    for t in (plain, act, masked, summed):
        assert bool((t != 0).any(0).all()), "an output column is all zero"


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("R", [65, 257])
def test_ffn_exact_case_is_exact_at_every_storage_point(R, seed):
    c = bc.ffn_exact_case(R, seed)
    ref = bc.ffn_chain(c, F64)
    assert int(c["w1"].abs().sum(1).max()) == bc.NNZ_W1 and int(c["w2"].abs().sum(1).max()) == bc.NNZ_W2
    unrounded_h = torch.relu(ref["hpre"])
    for name, t in dict(x=c["x"], w1=c["w1"], w2=c["w2"], h=unrounded_h, z=ref["z"], dy=c["dy"]).items():
        assert bc.holds(t), name
    assert float(unrounded_h.max()) <= bc.NNZ_W1 + 1 and float(ref["z"].abs().max()) <= bc.NNZ_W2 * (bc.NNZ_W1 + 1) + 4
    assert torch.equal(ref["pre"], ref["z"]) and torch.equal(ref["mean"].float().double(), ref["mean"])
    positive = float(ref["m"].mean())
    assert 0.2 <= positive <= 0.8, positive
    assert bool((ref["h"] != 0).any(0).all()) and bool((ref["z"] != 0).any(0).all())


@pytest.mark.parametrize("R,N,K", [(257, 128, 128), (129, 384, 128), (65, 128, 384), (4133, 13, 128)])
def test_weight_gradient_exact_case_is_exact(R, N, K):
    c = bc.wgrad_exact_case(R, N, K)
    assert bc.holds(c["dy"]) and bc.holds(c["x"])
    dw = (c["dy"] * (c["mask"] > 0)).t() @ c["x"]
    assert float((c["dy"].abs().t() @ c["x"].abs()).max()) < 2 ** 24 and torch.equal(dw.float().double(), dw)
    assert bool((dw != 0).any(0).all())


@pytest.mark.parametrize("variant", ["normal", "scaled"])
@pytest.mark.parametrize("K,N", bc.GEMM_SHAPES)
def test_float32_restatement_sits_inside_the_single_product_bar(K, N, variant):
    worst = worst_acc = 0.0
    for R in (1, 65, 257):
        c = bc.gemm_random_case(R, K, N, variant)
        for kw in (dict(), dict(bias=c["bias"]), dict(bias=c["bias"], relu=True), dict(bias=c["bias"], residual=c["residual"])):
            want, _ = bc.gemm_chain(c["a"], c["w"], dtype=F64, store=False, **kw)
            got, _ = bc.gemm_chain(c["a"], c["w"], dtype=F32, **kw)
            raw, _ = bc.gemm_chain(c["a"], c["w"], dtype=F32, store=False, **kw)
            S = bc.gemm_scale(c["a"], c["w"], kw.get("bias"), kw.get("residual"))
            worst = max(worst, bc.worst_ratio(got, want, bc.product_bar(want, S, K)))
            worst_acc = max(worst_acc, bc.worst_ratio(raw, want, bc.product_bar(want, S, K, stored=False)))
    print(f"single-product bar, float32 restatement K={K} N={N} {variant}: worst error / bar {worst:.3f} stored, "
          f"{worst_acc:.3f} of the accumulation term before the store")
    # a correctly rounded bf16 value is itself up to 2^-8 |want| away: the stored result can only be inside the bar; the
    # factor 2 to spare is held on the term that is the restatement's own, the accumulation
    assert worst <= 1.0 and worst_acc <= 0.5


@pytest.mark.parametrize("R,K,N,relu", [(100000, 384, 128, False), (100000, 128, 128, False), (100000, 128, 384, True)])
def test_planted_errors_pass_the_norm_wise_bar_and_fail_the_element_wise_bar(R, K, N, relu):
    c = bc.gemm_random_case(R, K, N)
    want, _ = bc.gemm_chain(c["a"], c["w"], c["bias"], relu, None, c["residual"], F64, store=False)
    bar = bc.product_bar(want, bc.gemm_scale(c["a"], c["w"], c["bias"], c["residual"]), K)
    good, wrong = bc.planted_errors(c, relu)
    assert bc.worst_ratio(good, want, bar) <= 1.0
    assert len(wrong) == (5 if relu else 4)
    for name, y in wrong.items():
        nw, ew = bc.normwise(y, want), bc.worst_ratio(y, want, bar)
        print(f"R={R} K={K} N={N} {name}: norm-wise {nw:.2e} (bar {bc.NORMWISE_IO:.0e}), worst element error / bar {ew:.1f}")
        assert nw < bc.NORMWISE_IO, name          # today's check does not see it
        assert ew > 1.0, name                     # the element-wise check does


def test_layernorm_epilogue_bars_hold_for_a_float32_restatement():
    c = bc.gemm_exact_case(257, 128, 128)
    z, _ = bc.gemm_chain(c["a"], c["w"], c["bias"], residual=c["residual"], store=False)
    y, mean, rstd = bc.ln_rows(z, c["gamma"], c["beta"])
    zf = z.float()
    mf = zf.mean(-1)
    rf = (zf.var(-1, unbiased=False) + bc.EPS).rsqrt()
    yf = ((zf - mf[:, None]) * rf[:, None] * c["gamma"].float() + c["beta"].float()).to(bc.BF)
    assert torch.equal(mf.double(), mean)
    assert float(((rf.double() - rstd).abs() / rstd).max()) <= bc.RSTD_REL / 2
    assert bc.worst_ratio(yf, y, bc.ln_out_bar(z, c["gamma"], c["beta"])) <= 1.0


@pytest.mark.parametrize("R", [65, 257, 4133])
def test_chained_restatement_figures(R):
    """The float32 restatement against the float64 reference with the same storage points: the figures the GPU test multiplies
    by MARGIN_MAX / MARGIN_RMS.  Both sides round to bf16 at the same points, so the figures are those of rare one-ulp
    disagreements (none at all in a few thousand elements): the GPU test pools its cases before it compares."""
    c = bc.ffn_random_case(R)
    ref, low = bc.ffn_chain(c, F64), bc.ffn_chain(c, F32)
    for name in ("y", "dz", "dx"):
        mx, rms = bc.row_scaled_error(low[name], ref[name])
        print(f"feed-forward restatement R={R} {name}: max {mx:.3e} rms {rms:.3e} of the row rms")
        assert rms < 2.0 ** -7 and mx < 16 * 2.0 ** -7, (name, mx, rms)


@pytest.mark.parametrize("R,grid", [(65, None), (257, None), (2 * 64 + 65, 2)])
def test_planted_rows_bars_hold_and_see_a_dropped_or_doubled_row(R, grid):
    c = bc.ffn_exact_case(R)
    rows = bc.planted_rows(R, grid)
    assert len(rows) <= 8 and rows[0] == 0 and rows[-1] == R - 1
    dy = bc.plant(c["dy"], rows)
    ref, low = bc.ffn_chain(c, F64, dy=dy), bc.ffn_chain(c, F32, dy=dy)
    bars = bc.ffn_planted_bars(c, ref, rows)
    outside = [r for r in range(R) if r not in rows]
    assert not ref["dz"][outside].any() and not low["dz"][outside].any()      # a zero dy row is a zero dz row
    for name, bar in bars.items():
        spare = bc.worst_ratio(low[name], ref[name], bar)
        print(f"planted rows R={R} {name}: float32 restatement error / bar {spare:.3f}")
        assert spare <= 0.5, (name, spare)
        assert bool((ref[name] != 0).any()), name
    for r in rows:
        one = bc.ffn_chain(c, F64, dy=bc.plant(c["dy"], [r]))
        for name, bar in bars.items():
            for what, wrong in (("dropped", ref[name] - one[name]), ("doubled", ref[name] + one[name])):
                ratio = bc.worst_ratio(wrong, ref[name], bar)
                assert ratio >= 10, (name, what, r, ratio)


def test_planted_rows_name_the_tile_edges():
    assert bc.planted_rows(1) == [0]
    assert bc.planted_rows(65) == [0, 63, 64]
    assert bc.planted_rows(257) == [0, 63, 64, 192, 255, 256]
    assert bc.planted_rows(256 * 64 + 65, 256) == [0, 63, 64, 16384, 16447, 16448]
    assert bc.planted_rows(3 * 64 + 65, 2) == [0, 63, 64, 128, 191, 192, 255, 256]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("B,N", [(2, 9), (3, 20)])
def test_attention_half_exact_case_is_exact_and_its_written_out_backward_is_autograd(B, N, seed):
    c = bc.attn_exact_case(B, N, seed)
    tiles = bc.attn_planted_tiles(B, N)
    dz, dO = bc.plant_tiles(c, tiles)
    ref = bc.attn_half_chain(c, dz, dO)
    for name, t in dict(y=c["y"], q=c["q"], k=c["k"], we=c["we"], woe=c["woe"], e=ref["e"], s=ref["s"], pre=ref["pre"]).items():
        assert bc.holds(t), name
    assert float(ref["e"].abs().max()) <= 8 and float(ref["s"].abs().max()) <= 18 and float(ref["pre"].abs().max()) <= 112
    mean = ref["pre"].mean(-1)
    assert torch.equal(mean.float().double(), mean)
    assert bool((ref["s"].reshape(-1, 128) != 0).any(0).all()) and bool((ref["pre"].reshape(-1, 128) != 0).any(0).all())
    assert 0.1 <= float((ref["s"] != 0).double().mean()) <= 0.9
    # the written-out backward against float64 autograd of the same forward
    leaves = {n: c[n].clone().requires_grad_(True) for n in ("we", "be", "woe", "boe")}
    e = c["y"] @ leaves["we"].t() + leaves["be"]
    s = bc.ALPHA * c["q"][:, :, None, :] * c["k"][:, None, :, :] * (e * e + e)
    o = (torch.softmax(s, dim=2) * c["v"][:, None, :, :]).sum(2)
    pre = c["y"] + s @ leaves["woe"].t() + leaves["boe"]
    ((o * dO).sum() + (pre * dz).sum()).backward()
    for n in ("we", "be", "woe", "boe"):
        got, want = ref["d" + n], leaves[n].grad
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), n
    # a float32 evaluation sits inside the bars; a dropped or doubled planted row does not
    c32 = {n: (t.float() if torch.is_tensor(t) else t) for n, t in c.items()}
    low = bc.attn_half_chain(c32, dz.float(), dO.float())
    rows = [(t, j) for t in tiles for j in (0, N - 1)]
    for n, bar in ref["bars"].items():
        spare = bc.worst_ratio(low[n], ref[n], bar)
        print(f"attention half planted tiles B={B} N={N} {n}: float32 restatement error / bar {spare:.3f}")
        assert spare <= 0.5, (n, spare)
    for t, j in rows:
        one = torch.zeros_like(dz).view(B * N, N, 128)
        one[t, j] = dz.view(B * N, N, 128)[t, j]
        r1 = bc.attn_half_chain(c, one.view(B, N, N, 128), torch.zeros_like(dO))
        for n, bar in ref["bars"].items():
            for wrong in (ref[n] - r1[n], ref[n] + r1[n]):
                assert bc.worst_ratio(wrong, ref[n], bar) >= 10, (n, t, j)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("B,N,E", [(2, 6, 5), (3, 17, 8), (2, 45, 1)])
def test_embedding_exact_case_is_exact_and_its_written_out_backward_is_autograd(B, N, E, seed):
    c = bc.embed_exact_case(B, N, E, seed)
    ref = bc.embed_chain(c)
    assert int(c["w2"].abs().sum(1).max()) == 8 == int(c["w2"].abs().sum(1).min())
    assert int(c["w2"].abs().sum(0).max()) == 16 == int(c["w2"].abs().sum(0).min())
    for name in ("h", "gs", "dpre2", "dh", "dpre1"):
        assert bc.holds(ref[name]), name
    assert bc.holds(c["w1"]) and bc.holds(c["w2"]) and bc.holds(c["g"])
    assert float(ref["h"].max()) <= 2 * E + 1 and float(ref["dpre2"].abs().max()) <= 4 and float(ref["dh"].abs().max()) <= 64
    assert float(ref["pre2"].abs().min()) >= 0 and torch.equal(ref["pre2"], ref["pre2"].round())      # the sign of pre2 is that of an integer
    for name in ("da", "dw1", "db1", "dw2", "db2"):
        assert torch.equal(ref[name].float().double(), ref[name]) and float(ref[name].abs().max()) < 2 ** 24, name
    positive = float((ref["pre2"] > 0).double().mean())
    assert 0.2 <= positive <= 0.8, positive
    # (a takes 2^E values, so some output channels never fire on any row: three quarters must, half of them at E = 1)
    live = float((ref["dw2"] != 0).any(1).double().mean())
    assert live >= (0.75 if E >= 5 else 0.5) and bool((ref["da"].reshape(-1, E) != 0).any(0).all())
    leaves = {n: c[n].clone().requires_grad_(True) for n in ("a", "w1", "b1", "w2", "b2")}
    f = torch.relu(torch.relu(leaves["a"] @ leaves["w1"].t() + leaves["b1"]) @ leaves["w2"].t() + leaves["b2"])
    (((f + f.transpose(1, 2)) / 2) * c["g"]).sum().backward()
    for n in ("a", "w1", "b1", "w2", "b2"):
        assert torch.equal(ref["d" + n], leaves[n].grad), n


@pytest.mark.parametrize("slope", [0.0, 0.01])
@pytest.mark.parametrize("B,N,E", [(2, 6, 5), (3, 17, 8), (2, 45, 1)])
def test_embedding_restatement_sits_inside_the_stored_chain_bars(B, N, E, slope):
    """relu and leaky on N(0,1) data: the float32 restatement of the kernel's chain inside the derived bars (an adjacent-bf16
    disagreement of one h or dpre1 may use a whole 2^-7 term: the bar is the bound, there is nothing to spare on it), and the
    chain without storage points is float64 autograd."""
    c = bc.embed_random_case(B, N, E)
    ref, low = bc.embed_stored_chain(c, slope), bc.embed_stored_chain(c, slope, F32)
    for name, bar in ref["bars"].items():
        ratio = bc.worst_ratio(low[name], ref[name], bar)
        print(f"embedding restatement B={B} N={N} E={E} slope {slope} {name}: error / bar {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)
    leaves = {n: c[n].clone().requires_grad_(True) for n in ("a", "w1", "b1", "w2", "b2")}
    act = lambda v: torch.nn.functional.leaky_relu(v, slope) if slope else torch.relu(v)
    f = act(act(leaves["a"] @ leaves["w1"].t() + leaves["b1"]) @ leaves["w2"].t() + leaves["b2"])
    (((f + f.transpose(1, 2)) / 2) * c["g"]).sum().backward()
    for n in ("a", "w1", "b1", "w2", "b2"):      # the storage points move every gradient by a few bf16 roundings, no more
        got, want = ref["d" + n], leaves[n].grad
        assert float((got - want).norm() / want.norm()) < 3 * bc.ULP_BF16, n
