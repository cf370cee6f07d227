"""Rows, references and per-row bars of tests/test_ln_cases_host.py and tests/test_hip_ln_range.py: every hand-written
LayerNorm of csrc/ (seven forward copies, six backward copies) on rows away from N(0,1) -- constant rows, rows with a large
offset, rows of very large or very small magnitude, single spikes and outliers -- each row held to a bar of its own.

Rows are built in float64 on the CPU from fixed seeds and rounded through the storage type (float32 or bf16); the rounded
values are what the float64 references (tests/kernel_math.py) see.  Nothing here needs a GPU.

Bars.  With u = 2^-24 and, per row, kappa = 1 + rstd max|z|, X = 1 + max|xhat|, Gamma = max|gamma|, U = max|gamma dy|,
T = max|tz|, the max-abs error within a row is bounded by K u times

    mean   max|z|                                   (a zero row's mean is exactly 0)
    rstd   kappa rstd
    y      kappa Gamma X + max|beta|
    dz     kappa rstd U X^2
    gdy    kappa rstd Gamma T X^2
    gz     kappa rstd^2 U T X^3

and the error of a column sum (over all rows r) in channel c by K u times

    dbeta   sum_r |dy_rc|
    dgamma  sum_r (kappa_r X_r |dy_rc| + |dy_rc xhat_rc|)
    ggamma  sum_r kappa_r rstd_r T_r X_r^2 |dy_rc|

-- the first-order effect of one float32 rounding of z and of the mean on each formula of tests/kernel_math.py.  Every bar
comes from the float64 reference alone.  Where z = a + r is summed inside the kernel, max|z| grows by u max(|a| + |r|).
bf16 kernels: the same bars plus, for every output that is stored as bf16, 2^-8 |want| per element (2^-8 is the unit
roundoff of bf16: one rounding of the output); their float32 statistics and column sums get the float32 bars.

K.  tests/test_ln_cases_host.py evaluates kernel_math.ln_fwd / ln_bwd / ln_bwd2 in plain float32 (and float32
torch.nn.functional.layer_norm, forward only) against float64 on these rows, C in WIDTHS, five seeds, and prints the worst
error / (u x bound) per quantity.  Measured (K = 1 units):

    mean 2.73   rstd 0.91   y 2.68   dz 3.05   gdy 3.46   gz 0.71   dbeta 1.75   dgamma 0.46   ggamma 0.05
    torch layer_norm, forward:   mean 2.65   rstd 1.00   y 1.99
    on statistics rounded from float64 (C = 128):   dz 2.03   gdy 1.40   gz 0.01   dbeta 0.90

The worst is 3.46 (gdy); K = 16 is four times that, rounded up to a power of two: the margin is there because the kernels
sum in butterfly order, not sequentially.  The float32 restatements must stay within K / 4, and the host test fails if the
measured worst ratio stops supporting this K."""
import torch

import kernel_math as km

U32 = 2.0 ** -24
K = 16
EPS = 1e-5
BF16_OUT = 2.0 ** -8
NAMES = ("normal", "const", "zero", "off1e4", "off1e6", "huge", "tiny", "spike", "const_ulps", "alt", "outlier")
WIDTHS = (4, 8, 12, 128, 260, 384, 516, 640, 768, 1024)
FORWARD = ("mean", "rstd", "y")
FIRST = ("dz", "dgamma", "dbeta")
SECOND = ("gz", "gdy", "ggamma")
COLUMN = ("dgamma", "dbeta", "ggamma")


def _randn(shape, g):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def rounded(t, dtype=torch.float32):
    """float64 values that the storage type holds exactly."""
    return t.to(dtype).double()


def rows(C, seed, dtype=torch.float32):
    """name -> float64 row [C], every value representable in ``dtype``.  The positions of the special channels are clamped
    into the row: the spike sits in the LAST channel (the last lane's share of every lane reduction), the 2^-20 step of
    const_ulps in the middle, the outlier at two thirds."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = {}
    out["normal"] = _randn((C,), g)
    out["const"] = torch.full((C,), 3.7, dtype=torch.float64)
    out["zero"] = torch.zeros(C, dtype=torch.float64)
    out["off1e4"] = 1e4 + _randn((C,), g)
    out["off1e6"] = 1e6 + 0.5 * _randn((C,), g)
    out["huge"] = 1e15 * _randn((C,), g)
    out["tiny"] = 1e-18 * _randn((C,), g)
    out["spike"] = torch.zeros(C, dtype=torch.float64)
    out["spike"][C - 1] = 1.0
    out["const_ulps"] = torch.ones(C, dtype=torch.float64)
    out["const_ulps"][min(C - 1, C // 2)] = 1.0 + 2.0 ** -20
    out["alt"] = 1e3 * (1 - 2 * (torch.arange(C) % 2)).double()
    out["outlier"] = _randn((C,), g)
    out["outlier"][min(C - 1, (2 * C) // 3)] = 1e8
    out = {n: rounded(out[n], dtype) for n in NAMES}
    for n, z in out.items():
        # the float32 sum of squares of the row stays finite (1e18 rows overflow float32 torch itself at C >= 384)
        assert C * float((z * z).max()) < 2.0 ** 126, (n, C)
    return out


def boundary_positions(R):
    """Rows at tile and group boundaries: 0, 15, 16, 63, 64 where R allows, R - 2 and R - 1."""
    return sorted({p for p in (0, 15, 16, 63, 64, R - 2, R - 1) if 0 <= p < R})


def plant(R, C, seed, dtype=torch.float32, positions=None, names=NAMES, reps=3):
    """-> (z [R, C] float64 of `normal` rows with named rows planted, {row: name}).  Without ``positions`` each name is
    planted ``reps`` times: the boundary positions come first, the others are spread over the rest of the matrix, and the
    name that meets a given position rotates with the seed.  With ``positions`` the names go there in order (cycling)."""
    g = torch.Generator().manual_seed(2000 + seed)
    z = rounded(_randn((R, C), g), dtype)
    if positions is None:
        first = boundary_positions(R)
        rest = [p for p in range(R) if p not in first]
        want = min(R, reps * len(names))
        extra = max(0, want - len(first))
        step = max(1, len(rest) // max(1, extra))
        positions = (first + rest[::step][:extra])[:want]
        shift = seed
    else:
        shift = 0
    where = {}
    for k, p in enumerate(positions):
        name = names[(k + shift) % len(names)]
        z[p] = rows(C, seed + 17 * k, dtype)[name]
        where[int(p)] = name
    return z, where


def operands(R, C, seed, dtype=torch.float32):
    """gamma, beta (float32 parameters), dy, tz (``dtype`` activations) as float64."""
    g = torch.Generator().manual_seed(3000 + seed)
    gamma = rounded(1 + 0.2 * _randn((C,), g))
    beta = rounded(_randn((C,), g))
    dy = rounded(_randn((R, C), g), dtype)
    tz = rounded(_randn((R, C), g), dtype)
    return gamma, beta, dy, tz


def split_residual(z, seed, dtype=torch.float32):
    """z = a + r for a random r: a = round(z - r).  -> (a, r, a + r in float64): the kernel's input IS a + r."""
    g = torch.Generator().manual_seed(4000 + seed)
    r = rounded(_randn(tuple(z.shape), g), dtype)
    a = rounded(z - r, dtype)
    return a, r, a + r


def round_stats(z, eps=EPS):
    """The float64 statistics of z rounded to float32: what a backward copy is GIVEN, so that no forward's error is in play."""
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    return rounded(mu), rounded(torch.rsqrt(var + eps))


def reference(z, gamma, beta, dy=None, tz=None, eps=EPS, stats=None, dtype=torch.float64):
    """tests/kernel_math.py on float64 operands evaluated in ``dtype`` -> dict of FORWARD (+ FIRST (+ SECOND)).
    ``stats``: (mean, rstd) [R,1] that the backward formulas take instead of the forward's."""
    c = lambda t: None if t is None else t.to(dtype)
    z, gamma, beta, dy, tz = map(c, (z, gamma, beta, dy, tz))
    y, mu, rstd = km.ln_fwd(z, gamma, beta, eps)
    out = dict(y=y, mean=mu.squeeze(-1), rstd=rstd.squeeze(-1))
    if stats is not None:
        mu, rstd = c(stats[0]), c(stats[1])
    if dy is not None:
        out["dz"], out["dgamma"], out["dbeta"] = km.ln_bwd(z, gamma, mu, rstd, dy)
    if tz is not None:
        out["gz"], out["ggamma"], out["gdy"] = km.ln_bwd2(z, gamma, mu, rstd, dy, tz)
    return out


def bounds(z, gamma, beta, dy=None, tz=None, eps=EPS, stats=None, summed=None):
    """The bounds of the module docstring WITHOUT the factor K u, from float64 alone: [R] for the row quantities, [C] for the
    column sums.  ``summed`` = (a, r): z = a + r is summed by the kernel (max|z| grows by u max(|a| + |r|))."""
    mu = z.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((z - mu) ** 2).mean(-1, keepdim=True) + eps)
    if stats is not None:
        mu, rstd = stats
    xhat = (z - mu) * rstd
    zmax = z.abs().amax(-1)
    if summed is not None:
        zmax = (z.abs() + U32 * (summed[0].abs() + summed[1].abs())).amax(-1)
    rs = rstd.squeeze(-1)
    kappa = 1 + rs * zmax
    X = 1 + xhat.abs().amax(-1)
    Gm = float(gamma.abs().max())
    out = dict(mean=zmax, rstd=kappa * rs, y=kappa * Gm * X + float(beta.abs().max()), kappa=kappa)
    if dy is not None:
        Ud = (gamma * dy).abs().amax(-1)
        out["dz"] = kappa * rs * Ud * X ** 2
        out["dbeta"] = dy.abs().sum(0)
        out["dgamma"] = ((kappa * X).unsqueeze(-1) * dy.abs() + (dy * xhat).abs()).sum(0)
    if tz is not None:
        T = tz.abs().amax(-1)
        out["gdy"] = kappa * rs * Gm * T * X ** 2
        out["gz"] = kappa * rs ** 2 * Ud * T * X ** 3
        out["ggamma"] = ((kappa * rs * T * X ** 2).unsqueeze(-1) * dy.abs()).sum(0)
    return out


def ratios(got, want, bound, bf16=None):
    """error / (u x bound) per row ([R]) or per channel ([C]) in K = 1 units: a result passes where this is <= K.  No element
    is left out; a non-finite element is an infinite error; where the bound is 0 only an exact result passes.  bf16 (by
    default: ``got`` is stored as bf16 -- the float32 statistics and column sums of a bf16 kernel get no allowance): the bar
    K u bound + 2^-8 |want| per element, expressed on the same scale."""
    want = want.double()
    if bf16 is None:
        bf16 = got.dtype == torch.bfloat16
    g = got.detach().double().cpu().reshape(want.shape)
    err = (g - want).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    b = bound.double().reshape(-1, *([1] * (want.dim() - bound.dim()))) if want.dim() > bound.dim() else bound.double()
    den = U32 * b.expand_as(err) + (BF16_OUT / K * want.abs() if bf16 else 0.0)
    q = torch.where(err == 0, torch.zeros_like(err), err / den)      # (x / 0 = inf for x > 0)
    return q.reshape(q.shape[0], -1).amax(1) if q.dim() > 1 else q


def failures(label, got, want, bound, where, quantities, k=K, bf16=None, worst=None):
    """One line per row (or channel) of the quantities that exceeds ``k``, every planted row by its name.  ``got``: name ->
    tensor of the kernel; ``worst``: dict that collects the largest ratio per quantity."""
    out = []
    for q in quantities:
        ratio = ratios(got[q], want[q], bound[q], bf16)
        if worst is not None:
            worst[q] = max(worst.get(q, 0.0), float(ratio.max()))
        for i in torch.nonzero(ratio > k).flatten().tolist():
            who = f"channel {i}" if q in COLUMN else f"row {i} ({where.get(i, 'normal')})"
            out.append(f"{label} {q} {who}: error / (u x bound) = {float(ratio[i]):.3g} > K = {k}")
    return out


def row_rel(got, want):
    """Per row ||got - want||_2 / ||want||_2 (0 where both rows are zero, inf where only ``want`` is or ``got`` is not finite):
    how two bf16 results of the same float32 values are compared.  Two float32 values a rounding apart may land on adjacent
    bf16 values, 2^-7 apart in relative terms at the low end of a binade, so an element-wise 2^-8 cannot hold; over a row
    such flips are rare and half-ulp differences average out, and 2^-8 of the row norm holds with a factor 2 to spare."""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    g, w = g.reshape(-1, g.shape[-1]), w.reshape(-1, w.shape[-1])
    num, den = (g - w).norm(dim=1), w.norm(dim=1)
    num = torch.where(torch.isfinite(g).all(1), num, torch.full_like(num, float("inf")))
    return torch.where(num == 0, torch.zeros_like(num), num / den)


def report(label, worst):
    print(f"{label}: worst error / (u x bound), K = {K}: " + "  ".join(f"{q} {v:.3g}" for q, v in worst.items()))
