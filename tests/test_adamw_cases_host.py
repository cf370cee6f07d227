"""tests/adamw_cases.py on the CPU: the float64 reference is float64 torch.optim.AdamW, the gradients keep float32 and float64
on the same function, float32 torch meets every bar with the stated spare, a float32 restatement of the kernels' formulas
meets them too, and the bars bite -- five short wrong restatements each exceed one on a named case."""
import numpy as np
import pytest
import torch

import adamw_cases as ac

SETS = range(len(ac.HYPERS))


@pytest.mark.parametrize("init", ac.INITS)
@pytest.mark.parametrize("hyper", SETS)
def test_reference_is_float64_torch_step_by_step(hyper, init):
    c = ac.case(hyper, init)
    t64 = ac.torch_adamw(c.p0, c.grads, c.h, torch.float64)
    for t in range(ac.T):
        for k in "pmv":
            scale = np.abs(c.ref[k][t]).max()
            assert np.abs(t64[k][t] - c.ref[k][t]).max() <= 2.0 ** -48 * scale, (k, t + 1)
        assert np.all(c.ref["a"][t] >= np.abs(c.ref["m"][t]) * (1 - 1e-12))


@pytest.mark.parametrize("hyper", SETS)
def test_cases_are_what_they_claim(hyper):
    c, cs = ac.case(hyper, "zero"), ac.case(hyper, "spread")
    assert c.grads.dtype == np.float32 and c.grads.shape == (ac.T, ac.N_BARS) and np.array_equal(c.grads, cs.grads)
    assert c.h == ac.widened(ac.HYPERS[hyper]) and all(float(np.float32(x)) == x for x in c.h)
    b2 = np.float32(c.h[2])
    assert float(np.float32(1) - b2) == 1.0 - c.h[2]                      # the kernel's 1.0f - beta2 is exact
    g = np.abs(c.grads)
    tiny = float(np.finfo(np.float32).tiny)
    g2 = g * g
    assert g2.dtype == np.float32 and float(g2.min()) >= tiny and float(g2.max()) < 2.0 ** 120
    assert float(((np.float32(1) - b2) * g2).min()) >= tiny              # (1 - beta2) g^2 stays a normal float32 number
    assert 1e-13 < float(g.max(0).min()) < 1e-10 and 1e10 < float(g.max()) < 1e14      # 24 decades across the elements
    ratio = g.max(0) / np.median(g, axis=0)
    assert float(ratio.max()) < 1e3                                        # ... and not inside one element's history
    assert not c.p0.any() and cs.p0.dtype == np.float32
    assert 0 < float(np.abs(cs.p0).min()) < 1e-3 and 1e2 < float(np.abs(cs.p0).max()) < 1e4
    short = cs.prefix(7, ac.SHORT_STEPS)
    assert short.floor == cs.floor and short.grads.shape == (ac.SHORT_STEPS, 7) and short.ref["p"].shape == (ac.SHORT_STEPS, 7)
    again = ac.reference(short.p0, short.grads, short.h)
    assert all(np.array_equal(again[k], short.ref[k]) for k in "pmva")      # an element's history is its own


def test_floors_and_float32_torch_against_the_bars():
    """Prints the floor and float32 torch's worst error / bar per case -- the figures of DESIGN 3.29 -- and asserts the spare:
    0.5 of the zero bar, 0.75 of the spread bar, 0.5 of the moment bars."""
    floors, bad = [], []
    for hyper in SETS:
        for init in ac.INITS:
            c = ac.case(hyper, init)
            w = ac.worst(c, ac.torch_adamw(c.p0, c.grads, c.h, torch.float32))
            print(f"{c.name}: floor {c.floor:.3g}  float32 torch error / bar: p {w['p']:.3g}  exp_avg {w['m']:.3g}  "
                  f"exp_avg_sq {w['v']:.3g}")
            floors.append(c.floor)
            spare = dict(p=0.5 if init == "zero" else 0.75, m=0.5, v=0.5)
            bad += [f"{c.name} {k}: {w[k]:.3g} > {spare[k]}" for k in "pmv" if not w[k] <= spare[k]]
    # a narrower and a shifted gradient range give the same floor: it is a property of float32 AdamW, not of one draw
    for hyper, decades in ((0, (-6.0, 6.0)), (1, (-12.0, 0.0)), (3, (0.0, 12.0))):
        c = ac.case(hyper, "zero", decades)
        print(f"{c.name} decades {decades}: floor {c.floor:.3g}")
        floors.append(c.floor)
    print(f"floors: {min(floors):.3g} to {max(floors):.3g}")
    assert 5e-8 < min(floors) and max(floors) < ac.FLOOR_MAX, floors
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("init", ac.INITS)
@pytest.mark.parametrize("hyper", SETS)
def test_float32_restatement_of_the_kernels_meets_every_bar(hyper, init):
    """The formulas as the kernels have them (bias corrections in double from the float betas, rounded once), in float32
    numpy: inside every bar -- the wrong restatements below differ from THIS by one line each."""
    c = ac.case(hyper, init)
    w = ac.worst(c, ac.emulate(c, "host"))
    print(f"{c.name}: float32 restatement error / bar: {w}")
    assert max(w.values()) <= 0.75, w


def _p_worst(hyper, init, variant):
    c = ac.case(hyper, init)
    w = ac.worst(c, ac.emulate(c, variant))["p"]
    print(f"{variant} on {c.name}: error / bar = {w:.3g}")
    return w


@pytest.mark.parametrize("hyper", [0, 1, 2, 3])
def test_powf_bias_corrections_in_float32_break_the_zero_cases(hyper):
    """1.0f - powf(beta2, t): beta2^t is rounded next to 1 before the subtraction (what dg_adamw_flat_devstep did).  Outside
    the zero bar on every (., .999) and (., .9999) set -- by 1.7, 1.7, 2.6 and 26 -- and outside the spread bar too; sets 5
    and 6 (beta2 = .99, .9) stay inside, where 1 - beta2^t is large."""
    assert _p_worst(hyper, "zero", "powf") > 1
    assert _p_worst(hyper, "spread", "powf") > 1
    # ... from the second step on: the first step is exact (powf(b, 1) == b)
    c = ac.case(hyper, "zero")
    first = ac.p_ratio(c, 1, ac.emulate(c, "powf")["p"][0])
    assert float(first.max()) <= 0.5


@pytest.mark.parametrize("variant,hyper,init", [
    ("no_bc2", 1, "zero"),        # the trainer's default: sqrt(1 - .999^t) is 0.03 at t = 1
    ("no_bc2", 5, "zero"),        # beta2 = .9, where the correction is closest to 1
    ("eps_in", 0, "zero"),        # elements with |g| << eps = 1e-8: sqrt(v + eps) = 1e-4 against sqrt(v) + eps = 1e-8
    ("eps_in", 4, "spread"),      # eps = 1e-6
    ("l2", 0, "spread"),          # wd p against gradients of 1e-12: the decay becomes a full-size Adam step
    ("l2", 4, "spread"),          # weight_decay = .1
    ("step_off", 1, "zero"),      # bias corrections of step t + 1
    ("step_off", 5, "spread"),
])
def test_wrong_restatements_exceed_a_bar(variant, hyper, init):
    assert _p_worst(hyper, init, variant) > 100


def test_l2_decay_also_shows_in_the_moments_and_equals_decoupled_decay_without_decay():
    c = ac.case(0, "spread")
    w = ac.worst(c, ac.emulate(c, "l2"))
    assert w["m"] > 100 and w["v"] > 100
    c = ac.case(3, "spread")       # weight_decay = 0: the two are the same function
    assert ac.worst(c, ac.emulate(c, "l2")) == ac.worst(c, ac.emulate(c, "host"))


def test_a_wrong_element_is_named_and_a_non_finite_one_fails():
    c = ac.case(0, "spread").prefix(257, ac.SHORT_STEPS)
    p, m, v = (c.ref[k][1].copy() for k in "pmv")
    assert ac.failures(c, 2, p, m, v) == []
    p[5] += 2 * 2 * (4 * ac.U32 * abs(p[5]) + 4 * c.floor * c.h[0])      # twice the bar of step 2
    v[256] *= 1 + 32 * ac.U32 * 2
    m[3] = float("nan")
    lines = ac.failures(c, 2, p, m, v, label="t")
    assert len(lines) == 3, lines
    assert any(" p:" in ln and "element 5" in ln for ln in lines)
    assert any("exp_avg_sq" in ln and "element 256" in ln for ln in lines)
    assert any("exp_avg:" in ln and "element 3" in ln and "inf" in ln for ln in lines)
