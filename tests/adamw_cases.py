"""Cases, float64 reference and bars of tests/test_adamw_cases_host.py and tests/test_hip_adamw.py: the two AdamW entries
(dg_adamw_flat, dg_adamw_flat_devstep) and optim.FlatAdamW over T = 12 steps, where the bias corrections stop being exact.
Nothing here needs a GPU.

Hyper-parameters.  The ABI takes lr, beta1, beta2, eps, weight_decay as `float`; a case's hyper-parameters ARE those float32
values, widened to double for every float64 evaluation (``Case.h``).  With the float beta2 the kernel's `1.0f - beta2` is
exact, so the float64 reference, float64 torch and float32 torch -- all given the widened values -- evaluate the same
function as the kernels.

Gradients.  Element i has a scale 10^k_i, k_i uniform in [-12, 12] and fixed over the steps, times a standard normal per
step, rounded to float32.  g^2 and (1 - beta2) g^2 stay normal float32 numbers (asserted by the host test), so float32 and
float64 evaluate the same function.  A wider range would put 24 decades inside one element's history, where float32 torch
itself is off by order 1.

Initialisations.  ``zero``: the parameter is the sum of its updates (biases, LayerNorm betas) -- the update-precision case.
``spread``: a standard normal times 10^k, k uniform in [-3, 2] -- the weight-decay and rounding case.

Reference.  oracle/aux_oracle.adamw_step in float64 (the host test holds it to float64 torch.optim.AdamW step by step).

Floor.  floor(case) = max_t max_i |p32 - p64| / (lr t) of float32 CPU torch.optim.AdamW against float64 on the case's own
gradients from a zero initialisation: what a float32 evaluation of AdamW costs on these gradients, from the reference alone
(2.1e-7 to 3.2e-7; the host test asserts < 5e-7, so that a broken reference cannot widen a bar).  A shorter length takes
the first n elements and the first steps of the 4099-long case and keeps that case's floor: the floor is a maximum over
elements drawn from one distribution, and a prefix's own maximum over 1 to 1027 of them would only be a smaller sample of it.

Bars, at every step t (u = 2^-24):

    zero     max_i |p - p64|  <=  4 floor lr t          (4: the spare ln_cases.py gives a float32 evaluation)
    spread   |p - p64|_i      <=  t (4 u |p64|_i + 4 floor lr)
             (4 u |p64|: the rounded decay constant, the decay product and the subtraction, per step; with 2 in place of
             that 4 float32 torch reached 1.05 of the allowance)
    exp_avg_sq   |v - v64|_i  <=  8 u t v64_i
    exp_avg      |m - m64|_i  <=  8 u t A_i,   A = the same recursion on |g| (A >= |m64|)

exp_avg is a sum of terms of either sign: an element whose terms cancel has |m64| far below its terms, and no float32
evaluation keeps an error relative to |m64| there; A is the sum of the terms' magnitudes, which for exp_avg_sq (all terms
positive) is v64 itself.  The host test asserts float32 torch below 0.5 of the zero bar, 0.75 of the spread bar and 0.5 of
the moment bars, and that five short wrong restatements each exceed a bar on a named case."""
import functools

import numpy as np
import torch

from oracle import aux_oracle as aux

U32 = 2.0 ** -24
T = 12
N_BARS = 4099
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 1027, 4099)
SHORT_STEPS = 4
INITS = ("zero", "spread")
FLOOR_MAX = 5e-7
# (lr, beta1, beta2, eps, weight_decay) in the order of the ABI; [1] is the trainer's default
HYPERS = (
    (1e-3, .9, .999, 1e-8, 1e-2),
    (1e-5, .9, .999, 1e-8, 1e-2),
    (1e-4, .5, .999, 1e-8, 1e-2),
    (2e-4, .9, .9999, 1e-8, 0.0),
    (1e-3, 0.0, .99, 1e-6, .1),
    (1e-5, .5, .9, 1e-8, 1e-2),
)


def widened(h):
    """The float32 values the ABI receives, as Python floats."""
    return tuple(float(np.float32(x)) for x in h)


def gradients(n, seed, steps=T, decades=(-12.0, 12.0)):
    """[steps, n] float32: a fixed scale per element times a standard normal per step."""
    rng = np.random.default_rng(7000 + seed)
    scale = 10.0 ** rng.uniform(decades[0], decades[1], size=n)
    return (scale[None, :] * rng.standard_normal((steps, n))).astype(np.float32)


def initial(n, init, seed):
    """[n] float32."""
    if init == "zero":
        return np.zeros(n, dtype=np.float32)
    rng = np.random.default_rng(8000 + seed)
    return (10.0 ** rng.uniform(-3.0, 2.0, size=n) * rng.standard_normal(n)).astype(np.float32)


def reference(p0, grads, h, first_step=1):
    """aux_oracle.adamw_step in float64 from zero moments -> dict of [steps, n] float64: p, m, v and A (module docstring)."""
    lr, b1, b2, eps, wd = h
    p = np.asarray(p0, dtype=np.float64)
    m, v, a = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    out = dict(p=[], m=[], v=[], a=[])
    for k, g in enumerate(np.asarray(grads, dtype=np.float64)):
        p, m, v = aux.adamw_step(p, g, m, v, first_step + k, lr, b1, b2, eps, wd)
        a = b1 * a + (1 - b1) * np.abs(g)
        for key, val in zip("pmva", (p, m, v, a)):
            out[key].append(val)
    return {key: np.stack(val) for key, val in out.items()}


def torch_adamw(p0, grads, h, dtype):
    """torch.optim.AdamW on CPU tensors of ``dtype`` -> dict of [steps, n] float64: p, m, v."""
    lr, b1, b2, eps, wd = h
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0)).to(dtype).clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    out = dict(p=[], m=[], v=[])
    for g in grads:
        p.grad = torch.from_numpy(np.asarray(g)).to(dtype)
        opt.step()
        st = opt.state[p]
        for key, val in zip("pmv", (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
            out[key].append(val.double().numpy().copy())
    return {key: np.stack(val) for key, val in out.items()}


def floor_of(grads, h):
    """max_t max_i |p32 - p64| / (lr t): float32 torch against float64 torch on ``grads`` from a zero initialisation."""
    zero = np.zeros(grads.shape[1], dtype=np.float32)
    p32, p64 = torch_adamw(zero, grads, h, torch.float32)["p"], torch_adamw(zero, grads, h, torch.float64)["p"]
    t = np.arange(1, len(grads) + 1, dtype=np.float64)[:, None]
    return float((np.abs(p32 - p64) / (h[0] * t)).max())


class Case:
    """h (widened), p0 [n] and grads [steps, n] in float32, ref (``reference``), floor; ``init``, ``name``."""

    def __init__(self, name, h, init, p0, grads, ref, floor):
        self.name, self.h, self.init, self.p0, self.grads, self.ref, self.floor = name, h, init, p0, grads, ref, floor
        self.n, self.steps = grads.shape[1], grads.shape[0]

    def prefix(self, n, steps):
        """The first n elements and steps, with this case's floor (module docstring)."""
        ref = {k: v[:steps, :n] for k, v in self.ref.items()}
        return Case(f"{self.name} n={n}", self.h, self.init, self.p0[:n].copy(), self.grads[:steps, :n].copy(), ref,
                    self.floor)


@functools.lru_cache(maxsize=None)
def case(hyper, init, decades=(-12.0, 12.0)):
    """The N_BARS-long, T-step case of HYPERS[hyper]; computed once and shared (treat its arrays as read-only)."""
    h = widened(HYPERS[hyper])
    grads = gradients(N_BARS, hyper, T, decades)
    p0 = initial(N_BARS, init, hyper)
    return Case(f"set {hyper + 1} {HYPERS[hyper]} {init}", h, init, p0, grads, reference(p0, grads, h), floor_of(grads, h))


def _ratio(err, allowed, got):
    err = np.where(np.isfinite(got), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / allowed)


def p_ratio(c, t, p, rows=None):
    """error / bar of the parameters after step t (1-based) of case c, per element; passes where <= 1.  ``rows``: the
    initialisation kind per element where it is not the case's (FlatAdamW: True = zero-initialised)."""
    want = c.ref["p"][t - 1]
    got = np.asarray(p, dtype=np.float64).reshape(want.shape)
    lr = c.h[0]
    zero = (c.init == "zero") if rows is None else rows
    allowed = t * (np.where(zero, 0.0, 4 * U32 * np.abs(want)) + 4 * c.floor * lr)
    return _ratio(np.abs(got - want), allowed, got)


def moment_ratios(c, t, m, v):
    """-> (error / bar of exp_avg, of exp_avg_sq) after step t, per element."""
    m64, v64, a64 = (c.ref[k][t - 1] for k in "mva")
    m, v = (np.asarray(x, dtype=np.float64).reshape(m64.shape) for x in (m, v))
    return (_ratio(np.abs(m - m64), 8 * U32 * t * a64, m), _ratio(np.abs(v - v64), 8 * U32 * t * v64, v))


def worst(c, run, rows=None):
    """run: dict of [steps, n] p, m, v (a whole trajectory) -> dict of the largest error / bar over steps and elements."""
    out = dict(p=0.0, m=0.0, v=0.0)
    for t in range(1, len(run["p"]) + 1):
        rm, rv = moment_ratios(c, t, run["m"][t - 1], run["v"][t - 1])
        for k, r in zip("pmv", (p_ratio(c, t, run["p"][t - 1], rows), rm, rv)):
            out[k] = max(out[k], float(r.max()))
    return out


def failures(c, t, p, m, v, label="", rows=None, worst_so_far=None):
    """One line per quantity that exceeds its bar after step t, with the worst element."""
    rm, rv = moment_ratios(c, t, m, v)
    out = []
    for k, r in (("p", p_ratio(c, t, p, rows)), ("exp_avg", rm), ("exp_avg_sq", rv)):
        top = float(r.max()) if r.size else 0.0
        if worst_so_far is not None:
            worst_so_far[k] = max(worst_so_far.get(k, 0.0), top)
        if top > 1:
            out.append(f"{label} {c.name} step {t} {k}: error / bar = {top:.3g} at element {int(r.argmax())}")
    return out


# ---- float32 restatements of the kernels (host test: the correct one passes, the wrong ones exceed a bar) -------------
def emulate(c, variant="host"):
    """The kernels' formulas in float32 numpy on case c -> dict of [steps, n] p, m, v.  variant:
         host      bias corrections in double from the float betas, rounded once (dg_adamw_flat, and devstep now)
         powf      1.0f - powf(beta, t) in float32 (devstep before this change)
         no_bc2    no bias correction on the second moment
         eps_in    eps inside the square root
         l2        weight decay added to the gradient instead of decoupled decay
         step_off  a step count that is one ahead"""
    f = np.float32
    lr, b1, b2, eps, wd = (f(x) for x in c.h)
    p, m, v = c.p0.copy(), np.zeros_like(c.p0), np.zeros_like(c.p0)
    out = dict(p=[], m=[], v=[])
    for k, g in enumerate(c.grads):
        t = k + 1 + (variant == "step_off")
        if variant == "powf":
            bc1, bc2s = f(1) - np.power(b1, f(t)), np.sqrt(f(1) - np.power(b2, f(t)))
        else:
            bc1, bc2s = f(1.0 - float(b1) ** t), f(np.sqrt(1.0 - float(b2) ** t))
        if variant == "no_bc2":
            bc2s = f(1)
        if variant == "l2":
            g = g + wd * p
        else:
            p = p * (f(1) - lr * wd)
        m = b1 * m + (f(1) - b1) * g
        v = b2 * v + (f(1) - b2) * g * g
        if variant == "eps_in":
            den = np.sqrt(v / (bc2s * bc2s) + eps)
        else:
            den = np.sqrt(v) / bc2s + eps
        p = p - (lr / bc1) * m / den
        assert p.dtype == m.dtype == v.dtype == np.float32
        for key, val in zip("pmv", (p, m, v)):
            out[key].append(val.astype(np.float64))
    return {key: np.stack(val) for key, val in out.items()}
