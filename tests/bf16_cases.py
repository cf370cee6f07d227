"""Cases, float64 references and per-element bars of tests/test_bf16_cases_host.py and tests/test_hip_bf16_elements.py: the
dense kernels of the bf16 configuration (csrc/gemm_bf16.hip, csrc/ffn_bf16.hip, the bf16 instance of csrc/linear_wgrad.hip)
held element by element, at row counts around the 64-row tile and past the persistent grid.  Nothing here needs a GPU and no
bar comes from a kernel's output.

Exact cases.  bf16 holds every integer up to 256; float32 sums of integers below 2^24 are exact in any order.  The builders
below bound every stored value BY CONSTRUCTION (a fixed number of +-1 entries per weight row), so a correct kernel has to give
the float64 result bit for bit:

    row GEMM      a in {-2..2}, W' rows with exactly 96 entries of +-1, bias in {-3..3}, residual in {-4..4}:
                  |z| <= 2 * 96 + 3 + 4 = 199
    feed-forward  x in {-1, 0, 1}, W1 rows with exactly 8 entries of +-1 (density 1/16), b1 in {-1, 0, 1}: 0 <= h <= 9;
                  W2 rows with exactly 24 entries of +-1 (density 1/16), b2 in {-3..3}: |pre| <= 24 * 9 + 3 + 1 = 220
    weight grad   dy, x in {-2..2}: |dW| <= 4 R < 2^24 for R < 2^22

The mean of an integer row of 128 channels is a multiple of 1/128 below 2^8: exact.  The variance is not a float32 number in
general; rstd is a float32 function of it: the sum of 128 non-negative squares carries at most (128 + 2) u32 relative error in
any order, rsqrt halves that and adds its own 2 ulp: RSTD_REL = 2^-17 covers (65 + 4) 2^-24 = 2^-17.9.

Single-product bar (a bf16 output of ONE fp32-accumulated product, epilogue terms added in fp32):

    |got - want| <= 2^-8 |want| + (K + 4) 2^-23 (1 + 2^-8) S,     S = sum_k |a_k| |w_k| + |bias| + |residual|

2^-8 is the unit roundoff of bf16 (one rounding of the output).  The second term is the worst-order bound of a K-term fp32
sum, (K - 1) 2^-24 S, plus the epilogue additions, with one spare bit because the MFMA's internal rounding is not specified,
carried through the output rounding.  fp32 outputs (weight gradients of given operands) drop the first term.

Chained outputs (y, dz, dx of the fused feed-forward) pass through several bf16 storage points; the float64 reference
(``ffn_chain`` in float64) has the same storage points: bf16 weights, bf16 hidden tile, bf16 pre-LayerNorm sum as the backward
reads it, bf16 dz, bf16 dh.  The error of an element is divided by the rms of its row of the reference, and the bar is the
same figure of the float32 restatement (``ffn_chain`` in float32) times MARGIN_MAX / MARGIN_RMS.

Planted rows (weight gradients).  dy is zero outside at most 8 named rows, so dz = LN'(dy) is zero there too and every
parameter gradient is a sum over the planted rows only.  On the exact feed-forward case h, the ReLU bits, pre and mean are
exact; dz and dh are rounded to bf16 by the kernel and by the reference from values that differ by float32 rounding, so they
may land on ADJACENT bf16 numbers (one ulp = 2^-7 relative) -- never further, given the absolute term for cancellation inside
the LayerNorm backward:

    E(dz_rc) = 2^-7 |dz_rc| + 2^-15 rstd_r (|u_rc| + mean_c |u_rc| + |xhat_rc| mean_c |u_rc xhat_rc|)        u = gamma dy
    E(dh_rj) = 2^-7 |dh_rj| + m_rj sum_c E(dz_rc) |W2_cj| + (128 + 4) 2^-23 m_rj sum_c |dz_rc| |W2_cj|

and the bars of the gradients are, with A = (P + 4) 2^-23 for P planted rows,

    dW2_cj   sum_r E(dz_rc) h_rj + A sum_r |dz_rc| h_rj          db2_c  sum_r E(dz_rc) + A sum_r |dz_rc|
    dW1_jc   sum_r E(dh_rj) |x_rc| + A sum_r |dh_rj| |x_rc|      db1_j  sum_r E(dh_rj) + A sum_r |dh_rj|
    dbeta_c  A sum_r |dy_rc|                                     dgamma_c  (A + 2^-16) sum_r |dy_rc xhat_rc|

(xhat = rstd (pre - mean) is recomputed in float32 from exact pre and mean -- their difference is exact -- and an rstd within
RSTD_REL = 2^-17: 2^-16 with its own rounding; the same relative error of xhat, twice, and the two float32 row means are the
2^-15 term of E(dz).)  A dropped or doubled planted row moves
an element by |l_ri r_rj|, about 1/P of S_ij = sum_r |l_ri| |r_rj|, against a bar of about 2^-7 S_ij: with P <= 8 that is
more than a factor 10 on the worst element, which tests/test_bf16_cases_host.py asserts."""
import torch

BF = torch.bfloat16
U_BF16 = 2.0 ** -8          # unit roundoff of bf16
ULP_BF16 = 2.0 ** -7        # distance of adjacent bf16 numbers, relative
RSTD_REL = 2.0 ** -17
EPS = 1e-5
MARGIN_MAX, MARGIN_RMS = 2.0, 1.5       # kernel against float32 restatement, chained outputs (tests/test_hip_kernels.py:920)
NORMWISE_IO = 4e-3                      # the norm-wise bar of tests/test_hip_bf16.py, for the planted-error comparison
ROW_COUNTS = (1, 15, 17, 63, 64, 65, 129)
GEMM_SHAPES = ((128, 128), (128, 384), (384, 128))      # (K, N) of dg_row_gemm
NNZ_GEMM, NNZ_W1, NNZ_W2 = 96, 8, 24


def bf(t):
    """float64 values after one bf16 round trip."""
    return t.to(BF).double()


def holds(t):
    """every value survives a bf16 round trip"""
    return bool(torch.equal(bf(t), t.double()))


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def sparse_signs(rows, cols, nnz, g):
    """[rows, cols] float64 with exactly ``nnz`` entries of +-1 in every row."""
    idx = torch.rand(rows, cols, generator=g).argsort(1)[:, :nnz]
    sign = torch.randint(0, 2, (rows, nnz), generator=g).double() * 2 - 1
    return torch.zeros(rows, cols, dtype=torch.float64).scatter_(1, idx, sign)


# ------------------------------------------------------------------------------------------------ row GEMM
def gemm_exact_case(R, K, N, seed=0):
    """Integer operands of y = epi(a W'^T): W' [N, K] is the forward weight (mode 0) or the transpose of an input-gradient
    weight (mode 1); ``a2`` / ``w2`` feed the masked second launch of the same geometry."""
    g = torch.Generator().manual_seed(7000 + 131 * seed + R + K + 3 * N)
    return dict(R=R, K=K, N=N, a=_ints((R, K), -2, 2, g), w=sparse_signs(N, K, NNZ_GEMM, g), bias=_ints((N,), -3, 3, g),
                residual=_ints((R, N), -4, 4, g), a2=_ints((R, K), -2, 2, g), w2=sparse_signs(N, K, NNZ_GEMM, g),
                gamma=torch.rand(N, generator=g, dtype=torch.float64).float().double() + 0.5,
                beta=(torch.randn(N, generator=g, dtype=torch.float64) * 0.1).float().double())


def gemm_random_case(R, K, N, variant="normal", seed=0):
    """N(0,1) rows already rounded to bf16, weights x 0.1 as bf16 values; ``scaled``: rows x 2^(-30..30), weight columns x
    10^(-3..3) (tests/test_hip_kernels.py test_row_gemm_split_bf16_is_fp32_class_accurate)."""
    g = torch.Generator().manual_seed(9000 + 17 * seed + R + K + 3 * N)
    a = torch.randn(R, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64) * 0.1
    bias = torch.randn(N, generator=g, dtype=torch.float64) * 0.1
    residual = torch.randn(R, N, generator=g, dtype=torch.float64)
    if variant == "scaled":
        s = torch.exp2(torch.randint(-30, 31, (R, 1), generator=g).double())
        a, residual = a * s, residual * s
        w = w * (10.0 ** (torch.rand(N, 1, generator=g, dtype=torch.float64) * 6 - 3))
    # the weight is an fp32 parameter; its bf16 rounding is what the pack kernel stores: keep bf16 values so that the
    # reference and the kernel see the same numbers
    return dict(R=R, K=K, N=N, a=bf(a), w=bf(w), bias=bias.float().double(), residual=bf(residual))


def gemm_chain(a, w, bias=None, relu=False, mask=None, residual=None, dtype=torch.float64, store=True):
    """epi(a W'^T) in ``dtype`` arithmetic in the kernel's order: + bias, ReLU, mask, + residual; ``store``: rounded to bf16
    (returned in ``dtype``).  -> (y, z before ReLU / mask / residual)."""
    z = a.to(dtype) @ w.to(dtype).t()
    if bias is not None:
        z = z + bias.to(dtype)
    y = torch.relu(z) if relu else z
    if mask is not None:
        y = y * mask.to(dtype)
    if residual is not None:
        y = y + residual.to(dtype)
    return (y.to(BF).to(dtype) if store else y), z


def gemm_scale(a, w, bias=None, residual=None):
    """S of the single-product bar, float64."""
    s = a.abs() @ w.abs().t()
    if bias is not None:
        s = s + bias.abs()
    if residual is not None:
        s = s + residual.abs()
    return s


def product_bar(want, S, K, stored=True):
    """The single-product bar per element (module docstring)."""
    acc = (K + 4) * 2.0 ** -23 * (1 + U_BF16) * S
    return U_BF16 * want.abs() + acc if stored else acc


def worst_ratio(got, want, bar):
    """max over elements of |got - want| / bar, with 0 / 0 = 0 and x / 0 = inf."""
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    return float(ratio.max())


def ln_rows(z, gamma, beta, eps=EPS):
    """float64 LayerNorm over the last dimension -> (y, mean, rstd)."""
    mean = z.mean(-1)
    rstd = (z.var(-1, unbiased=False) + eps).rsqrt()
    return (z - mean[:, None]) * rstd[:, None] * gamma + beta, mean, rstd


def ln_out_bar(z, gamma, beta, eps=EPS):
    """Bar of the bf16 output of a LayerNorm epilogue on EXACT z: the output rounding plus float32 evaluation of
    (z - mean) rstd gamma + beta with rstd within RSTD_REL (8 float32 roundings with room: 2^-16 of the two terms)."""
    y, mean, rstd = ln_rows(z, gamma, beta, eps)
    return U_BF16 * y.abs() + 2.0 ** -16 * (((z - mean[:, None]) * rstd[:, None] * gamma).abs() + beta.abs())


# the wrong restatements of section 2: each takes the operands and returns a bf16-stored result with ONE planted error
def planted_errors(c, relu):
    """name -> wrong float32 restatement of y = relu?(a W'^T + bias) + residual, for the host test."""
    a, w, bias, res = c["a"], c["w"], c["bias"], c["residual"]
    R, K, N = c["R"], c["K"], c["N"]
    f32 = torch.float32
    good, z = gemm_chain(a, w, bias, relu, None, res, f32)
    out = {}
    y = good.clone()
    y[R - 1] = gemm_chain(a[R - 1:], w, None, relu, None, res[R - 1:], f32)[0][0]
    out["bias missing in the last row"] = y
    y = good.clone()
    y[R // 2, 4 * 5:4 * 6] = 0
    out["one 4-channel slot of one row zero"] = y
    y = good.clone()
    cut = a[R - 2:R - 1].clone()
    cut[:, K - 32:] = 0
    y[R - 2] = gemm_chain(cut, w, bias, relu, None, res[R - 2:R - 1], f32)[0][0]
    out["the last 32 k-steps missing in one row"] = y
    if relu:
        y = good.clone()
        y[R - 1] = (z[R - 1] + res[R - 1].float()).to(BF).float()
        out["the ReLU mask of one tail row all ones"] = y
    y = good.clone()
    y[R - 1] = gemm_chain(a[R - 1:], w, bias, relu, None, res[R - 2:R - 1], f32)[0][0]
    out["the residual taken from the row above"] = y
    return good, out


def normwise(got, want):
    return float((got.double() - want).norm() / want.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ weight gradient of given operands
def wgrad_exact_case(R, N, K, seed=0):
    g = torch.Generator().manual_seed(11000 + 7 * seed + R + 3 * N + 5 * K)
    return dict(R=R, N=N, K=K, dy=_ints((R, N), -2, 2, g), x=_ints((R, K), -2, 2, g), mask=_ints((R, N), -1, 1, g))


def planted_rows(R, grid=None):
    """At most 8 rows: 0, 63, 64, R - 1, the first and last row of the last full tile and, when ``grid`` workgroups do not
    cover the tiles, the first and last row of the first tile a workgroup takes in its second round."""
    rows = {0, 63, 64, R - 1}
    full = R // 64
    if full >= 1:
        rows |= {64 * (full - 1), 64 * full - 1}
    if grid is not None and (R + 63) // 64 > grid:
        rows |= {64 * grid, min(64 * grid + 63, R - 1)}
    rows = sorted(r for r in rows if 0 <= r < R)
    assert len(rows) <= 8
    return rows


def plant(t, rows):
    """``t`` with every row outside ``rows`` zero."""
    out = torch.zeros_like(t)
    out[rows] = t[rows]
    return out


# ------------------------------------------------------------------------------------------------ fused feed-forward
def ffn_exact_case(R, seed=0):
    g = torch.Generator().manual_seed(13000 + 11 * seed + R)
    return dict(R=R, x=_ints((R, 128), -1, 1, g), w1=sparse_signs(384, 128, NNZ_W1, g), b1=_ints((384,), -1, 1, g),
                w2=sparse_signs(128, 384, NNZ_W2, g), b2=_ints((128,), -3, 3, g),
                gamma=torch.rand(128, generator=g, dtype=torch.float64).float().double() + 0.5,
                beta=(torch.randn(128, generator=g, dtype=torch.float64) * 0.1).float().double(),
                dy=bf(torch.randn(R, 128, generator=g, dtype=torch.float64)))


def ffn_random_case(R, seed=0):
    """The data of tests/test_hip_bf16.py test_fused_ffn_bf16_forward_backward; weights as bf16 values."""
    g = torch.Generator().manual_seed(15000 + 11 * seed + R)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(R=R, x=bf(rn(R, 128)), w1=bf(rn(384, 128) * 0.1), b1=(rn(384) * 0.1).float().double(),
                w2=bf(rn(128, 384) * 0.06), b2=(rn(128) * 0.1).float().double(),
                gamma=(torch.rand(128, generator=g, dtype=torch.float64) + 0.5).float().double(),
                beta=(rn(128) * 0.1).float().double(), dy=bf(rn(R, 128)))


def ffn_chain(c, dtype=torch.float64, dy=None, eps=EPS):
    """The fused feed-forward, forward and backward, in ``dtype`` arithmetic with the kernel's storage points (module
    docstring).  float64: the reference; float32: the restatement the chained bars are measured on."""
    t = lambda v: v.to(dtype)
    st = lambda v: v.to(BF).to(dtype)
    x, w1, b1, w2, b2, gamma, beta = (t(c[k]) for k in ("x", "w1", "b1", "w2", "b2", "gamma", "beta"))
    dy = t(c["dy"] if dy is None else dy)
    hpre = x @ w1.t() + b1
    m = (hpre > 0).to(dtype)
    h = st(torch.relu(hpre))
    z = x + h @ w2.t() + b2
    mean = z.mean(-1)
    rstd = (z.var(-1, unbiased=False) + eps).rsqrt()
    y = st((z - mean[:, None]) * rstd[:, None] * gamma + beta)
    pre = st(z)
    xhat = (pre - mean[:, None]) * rstd[:, None]
    u = dy * gamma
    c1, c2 = u.mean(-1, keepdim=True), (u * xhat).mean(-1, keepdim=True)
    dz = st(rstd[:, None] * (u - c1 - c2 * xhat))
    dh = st(torch.where(m > 0, dz @ w2, torch.zeros((), dtype=dtype)))      # (a select, as autograd's ReLU backward: no 0 * inf)
    dx = st(dz + dh @ w1)
    return dict(hpre=hpre, h=h, m=m, z=z, pre=pre, mean=mean, rstd=rstd, y=y, xhat=xhat, u=u, c1=c1, c2=c2, dz=dz, dh=dh, dx=dx,
                dw2=dz.t() @ h, db2=dz.sum(0), dw1=dh.t() @ x, db1=dh.sum(0), dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0))


def row_scaled_errors(got, want):
    """|got - want| / rms of the element's row of ``want``, flat (rows with a zero rms, and rows in which ``want`` is not
    finite, are skipped)."""
    want = want.double()
    rms = want.pow(2).mean(-1, keepdim=True).sqrt()
    keep = (torch.isfinite(rms) & (rms > 0)).squeeze(-1)
    return ((got.double() - want).abs() / rms)[keep].reshape(-1)


def max_rms(e):
    return (float(e.max()), float(e.pow(2).mean().sqrt())) if e.numel() else (0.0, 0.0)


def row_scaled_error(got, want):
    """(max, rms) of ``row_scaled_errors``."""
    return max_rms(row_scaled_errors(got, want))


def ffn_planted_bars(c, ref, rows):
    """name -> per-element bar of the parameter gradients of the EXACT feed-forward case with ``dy`` planted in ``rows``
    (module docstring); ``ref`` = ffn_chain(c, float64, dy=planted dy)."""
    P = len(rows)
    A = (P + 4) * 2.0 ** -23
    dy = plant(c["dy"], rows)[rows]
    rstd, xhat, u = ref["rstd"][rows, None], ref["xhat"][rows], ref["u"][rows]
    dz, dh, h, m, x = ref["dz"][rows].abs(), ref["dh"][rows].abs(), ref["h"][rows], ref["m"][rows], c["x"][rows].abs()
    w2 = c["w2"].abs()
    c1a, c2a = u.abs().mean(-1, keepdim=True), (u * xhat).abs().mean(-1, keepdim=True)
    e_dz = ULP_BF16 * dz + 2.0 ** -15 * rstd * (u.abs() + c1a + c2a * xhat.abs())
    e_dh = ULP_BF16 * dh + m * (e_dz @ w2) + (128 + 4) * 2.0 ** -23 * m * (dz @ w2)
    return dict(dw2=e_dz.t() @ h + A * (dz.t() @ h), db2=e_dz.sum(0) + A * dz.sum(0),
                dw1=e_dh.t() @ x + A * (dh.t() @ x), db1=e_dh.sum(0) + A * dh.sum(0),
                dbeta=A * dy.abs().sum(0),
                dgamma=(A + 2.0 ** -16) * (dy * xhat).abs().sum(0))


# ------------------------------------------------------------------------------------------------ fused attention half
ALPHA = 0.25
NNZ_WE, NNZ_WOE = 7, 6


def attn_exact_case(B, N, seed=0):
    """Integer operands of dg_attn_half_fwd, exact by construction: y, q, k in {-1, 0, 1}, We rows with exactly 7 entries of
    +-1, be in {-1, 0, 1}: |e| <= 8 and e^2 + e is even and at most 72; alpha = 1/4: s a multiple of 1/2 with |s| <= 18; Woe
    rows with exactly 6 entries of +-1, boe in {-3..3}: pre a multiple of 1/2 with |pre| <= 6 * 18 + 3 + 1 = 112 < 128, where
    bf16 still resolves 1/2; the mean of 128 such values is a multiple of 1/256 below 2^7: a float32 number.  v, dz4 and d_o
    are N(0,1) bf16 values."""
    g = torch.Generator().manual_seed(17000 + 13 * seed + 101 * B + N)
    rn = lambda *s: bf(torch.randn(*s, generator=g, dtype=torch.float64))
    return dict(B=B, N=N, y=_ints((B, N, N, 128), -1, 1, g), q=_ints((B, N, 128), -1, 1, g), k=_ints((B, N, 128), -1, 1, g),
                v=rn(B, N, 128), we=sparse_signs(128, 128, NNZ_WE, g), be=_ints((128,), -1, 1, g),
                woe=sparse_signs(128, 128, NNZ_WOE, g), boe=_ints((128,), -3, 3, g),
                gamma=torch.rand(128, generator=g, dtype=torch.float64).float().double() + 0.5,
                beta=(torch.randn(128, generator=g, dtype=torch.float64) * 0.1).float().double(),
                dz=rn(B, N, N, 128), dO=rn(B, N, 128))


def attn_planted_tiles(B, N):
    """(b, i) of the first tile, one in the middle and the last."""
    T = B * N
    return sorted({0, T // 2, T - 1})


def plant_tiles(c, tiles):
    """(dz4, d_o) of case ``c`` with every (b, i) tile outside ``tiles`` zero."""
    B, N = c["B"], c["N"]
    dz, dO = torch.zeros_like(c["dz"]).view(B * N, N, 128), torch.zeros_like(c["dO"]).view(B * N, 128)
    dz[tiles], dO[tiles] = c["dz"].view(B * N, N, 128)[tiles], c["dO"].view(B * N, 128)[tiles]
    return dz.view(B, N, N, 128), dO.view(B, N, 128)


def attn_half_chain(c, dz, dO, alpha=ALPHA):
    """float64 forward of the attention half and the parameter gradients of its backward, written out (the host test holds
    them against autograd), with the per-element bars of the planted-tile test: dwoe / dboe are float32 sums of products of
    given bf16 numbers (bar A S, A = (P + 4) 2^-23 for P planted rows); de is rounded to bf16 on its way into the dwe
    product, from a float32 value whose softmax backward cancels:

        E(de) = 2^-7 |de| + 2^-15 |alpha q k (2 e + 1)| (|dz4| |Woe| + p (|g| + sum_j p |g|)),      g_ij = d_o_i v_j

    (2^-15: exp of |s| <= 18 in float32 and the two sums over j), and the bars of dwe / dbe are sum_r E(de_r) |y_r| + A S."""
    y, q, k, v, we, be, woe, boe = (c[n] for n in ("y", "q", "k", "v", "we", "be", "woe", "boe"))
    e = y @ we.t() + be
    qk = alpha * q[:, :, None, :] * k[:, None, :, :]
    s = qk * (e * e + e)
    p = torch.softmax(s, dim=2)
    o = (p * v[:, None, :, :]).sum(2)
    pre = y + s @ woe.t() + boe
    g = dO[:, :, None, :] * v[:, None, :, :]
    ds = dz @ woe + p * (g - (p * g).sum(2, keepdim=True))
    fac = qk * (2 * e + 1)
    de = ds * fac
    P = int((dz.abs().sum(-1) + dO.abs().sum(-1)[:, :, None] > 0).sum())
    A = (P + 4) * 2.0 ** -23
    e_de = ULP_BF16 * de.abs() + 2.0 ** -15 * fac.abs() * (dz.abs() @ woe.abs() + p * (g.abs() + (p * g.abs()).sum(2, keepdim=True)))
    f2 = lambda t: t.reshape(-1, 128)
    out = dict(e=e, s=s, o=o, pre=pre, de=de, dwe=f2(de).t() @ f2(y), dbe=f2(de).sum(0), dwoe=f2(dz).t() @ f2(s), dboe=f2(dz).sum(0))
    out["bars"] = dict(dwe=f2(e_de).t() @ f2(y).abs() + A * (f2(de).abs().t() @ f2(y).abs()), dbe=f2(e_de).sum(0) + A * f2(de).abs().sum(0),
                       dwoe=A * (f2(dz).abs().t() @ f2(s).abs()), dboe=A * f2(dz).abs().sum(0))
    return out


# ------------------------------------------------------------------------------------------------ edge embedding backward
def embed_exact_case(B, N, E, seed=0):
    """Integer operands of dg_embed_sym_bwd_bf16 (relu), exact by construction: a in {0, 1}^E, W1 in {-2..2}, b1 in
    {-1, 0, 1}: 0 <= h <= 2 E + 1 <= 17; W2 [128, 64] with +-1 at columns (c + 8 t) mod 64, t < 8 -- 8 per row, 16 per column -- and b2
    in {-1, 0, 1}; g even in {-4..4}, so gs = (g_ij + g_ji) / 2 and dpre2 are integers up to 4, |dh| <= 4 * 16 = 64 survives
    its bf16 store, |da| <= 64 * 64 * 2 and the parameter gradients are integer sums far below 2^24."""
    g = torch.Generator().manual_seed(19000 + 7 * seed + 1009 * B + 31 * N + E)
    a = _ints((B, N, N, E), 0, 1, g)
    w2 = torch.zeros(128, 64, dtype=torch.float64)
    c = torch.arange(128)
    for t in range(8):
        w2[c, (c + 8 * t) % 64] = torch.randint(0, 2, (128,), generator=g).double() * 2 - 1
    return dict(B=B, N=N, E=E, a=a, w1=_ints((64, E), -2, 2, g), b1=_ints((64,), -1, 1, g), w2=w2, b2=_ints((128,), -1, 1, g),
                g=2 * _ints((B, N, N, 128), -2, 2, g))


def embed_chain(c, g=None):
    """float64 backward of out = (f + f^T) / 2, f = relu(W2 relu(W1 a + b1) + b2), written out as the kernel's header does."""
    a, w1, b1, w2, b2 = (c[n] for n in ("a", "w1", "b1", "w2", "b2"))
    g = c["g"] if g is None else g
    pre1 = a @ w1.t() + b1
    h = torch.relu(pre1)
    pre2 = h @ w2.t() + b2
    gs = (g + g.transpose(1, 2)) / 2
    zero = torch.zeros((), dtype=gs.dtype)      # selects, as autograd's ReLU backward: a masked element is 0, never 0 * inf
    dpre2 = torch.where(pre2 > 0, gs, zero)
    dh = dpre2 @ w2
    dpre1 = torch.where(pre1 > 0, dh, zero)
    f2 = lambda t: t.reshape(-1, t.shape[-1])
    return dict(h=h, pre2=pre2, gs=gs, dpre2=dpre2, dh=dh, dpre1=dpre1, da=dpre1 @ w1, dw1=f2(dpre1).t() @ f2(a), db1=f2(dpre1).sum(0),
                dw2=f2(dpre2).t() @ f2(h), db2=f2(dpre2).sum(0))


def embed_random_case(B, N, E, seed=0):
    """The data of tests/test_hip_bf16.py test_embed_sym_bwd_bf16_streaming_kernel: a = softmax rows, float32 parameters, g an
    N(0,1) bf16 gradient."""
    g = torch.Generator().manual_seed(21000 + 7 * seed + 1009 * B + 31 * N + E)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    f = lambda t: t.float().double()
    return dict(B=B, N=N, E=E, a=f(torch.softmax(2 * rn(B, N, N, E), -1)), w1=f(rn(64, E) * 0.5), b1=f(rn(64) * 0.1),
                w2=f(rn(128, 64) * 0.15), b2=f(rn(128) * 0.1), g=bf(rn(B, N, N, 128)))


def embed_stored_chain(c, slope=0.0, dtype=torch.float64, g=None):
    """The embedding backward in ``dtype`` arithmetic with the storage points of csrc/embed_bf16.hip: h as bf16 in the dW2
    product (its sign, and the sign of pre2 from unrounded h and W2, decide act'), dpre2 as bf16 everywhere, W2 and W1 as bf16
    in dh = dpre2 W2 and da = dpre1 W1, dpre1 as bf16 in da only (dW1 / db1 take it in float32).  float64: the reference, with
    the per-element bars of the five outputs under "bars"; float32: the restatement the host test holds inside them.

    gs = (g_ij + g_ji) / 2 of two bf16 numbers and its bf16 rounding are the same numbers on both sides, so dpre2 carries no
    rounding error -- but its factor act'(pre2) is a sign, and the kernel recomputes pre2 from bf16 hi + lo splits of h and W2
    (three products): each split leaves 2^-16 of its value, the dropped lo x lo product is another 2^-16, so the sign of an
    element with |pre2| <= 2^-14 S2, S2 = sum_u |h_u| |W2_cu| + |b2_c|, is not determined (about one element in 10^4 on N(0,1)
    data; its forward value is zero to the same precision): E(dpre2) = (1 - slope) |gs| there, 0 elsewhere (leaky: plus
    2^-7 |dpre2| where pre2 <= 0 -- slope gs is rounded to float32 and then to bf16, the adjacent bf16 number at worst),
    and it enters dW2, db2 and, through E(dh) += sum_c E(dpre2_c) |W2_cu|, everything downstream.  h is rounded to bf16 from a float32 fma chain: E(h) = 2^-7 |h| (the adjacent bf16 number at worst).  dh is a
    128-term float32 sum of exact products: E(dh) = 132 * 2^-23 sum_c |dpre2_c| |W2_cu|, and so is E(dpre1) up to |act'|; its
    bf16 rounding in da adds 2^-7 |dpre1|.  With R = B N^2 rows and A = (R + 4) 2^-23:
        dW2  sum_r (|dpre2| E(h) + E(dpre2) |h|) + A sum_r |dpre2| |h|        db2  sum_r E(dpre2) + A sum_r |dpre2|
        dW1  sum_r E(dpre1) a + A sum_r |dpre1| a            db1  sum_r E(dpre1) + A sum_r |dpre1|
        da   sum_u (E(dpre1_u) + 2^-7 |dpre1_u|) |W1_ue| + 68 * 2^-23 sum_u |dpre1_u| |W1_ue|"""
    t = lambda v: v.to(dtype)
    st = lambda v: v.to(BF).to(dtype)
    a, w1, b1, w2, b2 = (t(c[n]) for n in ("a", "w1", "b1", "w2", "b2"))
    g = t(c["g"] if g is None else g)
    zero = torch.zeros((), dtype=dtype)
    dact = lambda x, d: torch.where(x > 0, d, slope * d if slope else zero)
    pre1 = a @ w1.t() + b1
    h = torch.where(pre1 > 0, pre1, slope * pre1)
    pre2 = h @ w2.t() + b2
    hb, w2b, w1b = st(h), st(w2), st(w1)
    gs = (g + g.transpose(1, 2)) / 2      # exact in float32: two bf16 numbers
    dpre2 = st(dact(pre2, gs))
    dh = dpre2 @ w2b
    dpre1 = dact(hb, dh)
    f2 = lambda v: v.reshape(-1, v.shape[-1])
    out = dict(da=st(dpre1) @ w1b, dw1=f2(dpre1).t() @ f2(a), db1=f2(dpre1).sum(0), dw2=f2(dpre2).t() @ f2(hb), db2=f2(dpre2).sum(0))
    if dtype == torch.float64:
        R = f2(a).shape[0]
        A = (R + 4) * 2.0 ** -23
        e_h = ULP_BF16 * f2(hb).abs()
        undecided = pre2.abs() <= 2.0 ** -14 * (h.abs() @ w2.abs().t() + b2.abs())
        e_d2 = f2(undecided * (1 - slope) * gs.abs())
        if slope:      # slope * gs is rounded to float32, then to bf16: the adjacent bf16 number at worst
            e_d2 = e_d2 + ULP_BF16 * f2((pre2 <= 0) * dpre2.abs())
        e_d1 = 132 * 2.0 ** -23 * (f2(dpre2).abs() @ w2b.abs()) + e_d2 @ w2b.abs()
        d1, d2 = f2(dpre1).abs(), f2(dpre2).abs()
        out["bars"] = dict(dw2=d2.t() @ e_h + e_d2.t() @ f2(hb).abs() + A * (d2.t() @ f2(hb).abs()), db2=e_d2.sum(0) + A * d2.sum(0),
                           dw1=e_d1.t() @ f2(a).abs() + A * (d1.t() @ f2(a).abs()), db1=e_d1.sum(0) + A * d1.sum(0),
                           da=((e_d1 + ULP_BF16 * d1) @ w1b.abs() + 68 * 2.0 ** -23 * (d1 @ w1b.abs())).reshape(out["da"].shape))
    return out
