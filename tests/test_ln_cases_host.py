"""tests/ln_cases.py on the CPU: the rows are what they claim, a plain float32 evaluation of the reference formulas meets
every bar with a factor 4 to spare, and the bars bite -- short wrong restatements of LayerNorm exceed them on the rows that
were planted for them."""
import pytest
import torch

import kernel_math as km
import ln_cases as lc

SEEDS = (0, 1, 2, 3, 4)
R = 67


def _case(C, seed, dtype=torch.float32):
    z, where = lc.plant(R, C, seed, dtype)
    gamma, beta, dy, tz = lc.operands(R, C, seed, dtype)
    return z, where, gamma, beta, dy, tz


def _rows_named(where, name):
    return [r for r, n in where.items() if n == name]


@pytest.mark.parametrize("C", [8, 128, 1024])
def test_rows_are_what_they_claim(C):
    r = lc.rows(C, 0)
    assert set(r) == set(lc.NAMES)
    for name, z in r.items():
        assert z.dtype == torch.float64 and torch.equal(z, z.float().double()), name
        assert C * float((z * z).max()) < 2.0 ** 126
    stat = lambda z: (float(z.mean()), float(((z - z.mean()) ** 2).mean()))
    kappa = lambda z: 1 + float(z.abs().max()) / (stat(z)[1] + lc.EPS) ** 0.5
    assert stat(r["const"]) == (float(torch.tensor(3.7).float()), 0.0)          # variance exactly 0 in float64
    assert stat(r["zero"]) == (0.0, 0.0)
    assert kappa(r["off1e6"]) > 1e5 and 1e3 < kappa(r["off1e4"]) < 1e5
    assert 1e14 < float(r["huge"].abs().max()) < 1e16 and stat(r["huge"])[1] > 1e28
    assert 0 < float(r["tiny"].abs().max()) < 1e-17 and stat(r["tiny"])[1] < 1e-6 * lc.EPS      # variance << eps
    assert float(r["spike"].sum()) == 1.0 and float(r["spike"][C - 1]) == 1.0 and int((r["spike"] != 0).sum()) == 1
    d = r["const_ulps"] - 1
    assert int((d != 0).sum()) == 1 and float(d.max()) == 2.0 ** -20 and stat(r["const_ulps"])[1] < 1e-12
    assert torch.equal(r["alt"].abs(), torch.full((C,), 1e3, dtype=torch.float64)) and stat(r["alt"]) == (0.0, 1e6)
    assert float(r["outlier"].max()) == 1e8 and int((r["outlier"].abs() > 10).sum()) == 1
    # the bf16 rows are bf16 values
    for name, z in lc.rows(C, 0, torch.bfloat16).items():
        assert torch.equal(z, z.bfloat16().double()), name


def test_plant_hits_the_boundaries_with_every_name():
    seen = {}
    for seed in range(11):
        z, where = lc.plant(R, 128, seed)
        assert z.shape == (R, 128) and set(lc.boundary_positions(R)) <= set(where)
        assert all(sum(n == name for n in where.values()) == 3 for name in lc.NAMES)
        for p, name in where.items():
            seen.setdefault(p, set()).add(name)
            assert torch.equal(z[p], lc.rows(128, seed + 17 * list(where).index(p))[name])
    assert lc.boundary_positions(R) == [0, 15, 16, 63, 64, 65, 66]
    assert all(seen[p] == set(lc.NAMES) for p in lc.boundary_positions(R))      # over the seeds: every name at every boundary
    z, where = lc.plant(4099, 256, 0, positions=[4096, 4097, 4098, 0, 1, 2], names=("huge", "zero", "const"))
    assert where == {4096: "huge", 4097: "zero", 4098: "const", 0: "huge", 1: "zero", 2: "const"}
    z, where = lc.plant(2, 768, 0)
    assert sorted(where) == [0, 1]


def test_float32_reference_meets_every_bar_with_a_factor_four_to_spare():
    """kernel_math in float32, and float32 torch layer_norm on the forward, against float64: within K / 4 of every bar at
    every width and seed, without and with a residual summed in float32.  Prints the worst ratio per quantity -- the figures
    in the docstring of tests/ln_cases.py."""
    worst, worst_torch, bad = {}, {}, []
    for C in lc.WIDTHS:
        for seed in SEEDS:
            z, where, gamma, beta, dy, tz = _case(C, seed)
            want = lc.reference(z, gamma, beta, dy, tz)
            bound = lc.bounds(z, gamma, beta, dy, tz)
            got = lc.reference(z, gamma, beta, dy, tz, dtype=torch.float32)
            bad += lc.failures(f"float32 C={C} seed={seed}", got, want, bound, where, lc.FORWARD + lc.FIRST + lc.SECOND,
                               k=lc.K / 4, worst=worst)
            y, mean, rstd = torch.native_layer_norm(z.float(), (C,), gamma.float(), beta.float(), lc.EPS)
            bad += lc.failures(f"layer_norm C={C} seed={seed}", dict(y=y, mean=mean.reshape(-1), rstd=rstd.reshape(-1)), want,
                               bound, where, lc.FORWARD, k=lc.K / 4, worst=worst_torch)
        a, r, zs = lc.split_residual(z, C)
        want = lc.reference(zs, gamma, beta, dy, tz)
        bound = lc.bounds(zs, gamma, beta, dy, tz, summed=(a, r))
        got = lc.reference((a.float() + r.float()).double(), gamma, beta, dy, tz, dtype=torch.float32)
        bad += lc.failures(f"float32 a + r C={C}", got, want, bound, where, lc.FORWARD + lc.FIRST + lc.SECOND, k=lc.K / 4,
                           worst=worst)
    lc.report("kernel_math in float32", worst)
    lc.report("torch layer_norm in float32", worst_torch)
    assert not bad, "\n".join(bad)
    # K is four times the worst ratio of the float32 reference, rounded up to a power of two, and at most 64
    top = max(worst.values())
    assert lc.K <= 64 and lc.K / 2 < 4 * top <= lc.K, top


def test_float32_reference_on_given_statistics_meets_the_bars():
    """The backward formulas on statistics rounded from float64 (what tests/test_hip_ln_range.py hands the backward copies)."""
    bad, worst = [], {}
    for seed in SEEDS:
        z, where, gamma, beta, dy, tz = _case(128, seed)
        stats = lc.round_stats(z)
        want = lc.reference(z, gamma, beta, dy, tz, stats=stats)
        bound = lc.bounds(z, gamma, beta, dy, tz, stats=stats)
        got = lc.reference(z, gamma, beta, dy, tz, stats=stats, dtype=torch.float32)
        bad += lc.failures(f"given statistics seed={seed}", got, want, bound, where, lc.FIRST + lc.SECOND, k=lc.K / 4,
                           worst=worst)
    lc.report("kernel_math in float32 on given statistics", worst)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the bars bite
def _forward32(z, gamma, beta, mean_of, var_of, rstd_of):
    """A float32 LayerNorm forward from three restatable pieces -> the FORWARD dict."""
    z, gamma, beta = z.float(), gamma.float(), beta.float()
    mu = mean_of(z)
    rstd = rstd_of(var_of(z, mu))
    return dict(y=(z - mu) * rstd * gamma + beta, mean=mu.squeeze(-1), rstd=rstd.squeeze(-1))


_MEAN = lambda z: z.mean(-1, keepdim=True)
_VAR = lambda z, mu: ((z - mu) ** 2).mean(-1, keepdim=True)
_RSTD = lambda var: torch.rsqrt(var + lc.EPS)


def _worst_on(name, C, wrong, quantities=("y", "rstd"), seed=0):
    """The largest ratio of a wrong forward over the rows planted as ``name``; the correct pieces pass on the same rows."""
    z, where, gamma, beta, _, _ = _case(C, seed)
    want, bound = lc.reference(z, gamma, beta), lc.bounds(z, gamma, beta)
    picked = _rows_named(where, name)
    assert picked
    worst = lambda got: max(float(lc.ratios(got[q], want[q], bound[q])[picked].max()) for q in quantities)
    assert worst(_forward32(z, gamma, beta, _MEAN, _VAR, _RSTD)) <= lc.K / 4
    return worst(_forward32(z, gamma, beta, **wrong))


@pytest.mark.parametrize("name", ["off1e4", "off1e6"])
@pytest.mark.parametrize("C", [8, 128, 640])
def test_one_pass_variance_breaks_the_offset_rows(name, C):
    one_pass = lambda z, mu: (z * z).mean(-1, keepdim=True) - mu * mu
    assert _worst_on(name, C, dict(mean_of=_MEAN, var_of=one_pass, rstd_of=_RSTD)) > lc.K


@pytest.mark.parametrize("C,padded", [(12, 32), (640, 1024)])
def test_variance_over_the_padded_width_breaks_ordinary_rows(C, padded):
    """A lane group of 8 / 64 lanes with 1 / 4 quads each holds 32 / 1024 channels: 1 / C must not count the masked ones."""
    over_padded = lambda z, mu: ((z - mu) ** 2).sum(-1, keepdim=True) / padded
    for name in ("normal", "alt", "off1e4", "spike"):
        assert _worst_on(name, C, dict(mean_of=_MEAN, var_of=over_padded, rstd_of=_RSTD)) > lc.K, name


@pytest.mark.parametrize("name", ["const", "zero"])
@pytest.mark.parametrize("C", [12, 128])
def test_misplaced_eps_breaks_the_constant_rows(name, C):
    dropped = lambda var: torch.rsqrt(var)
    outside = lambda var: torch.rsqrt(var) + lc.EPS
    for rstd_of in (dropped, outside):
        assert _worst_on(name, C, dict(mean_of=_MEAN, var_of=_VAR, rstd_of=rstd_of)) > lc.K


@pytest.mark.parametrize("C", [4, 128, 516])
def test_a_mean_that_drops_the_last_channel_breaks_the_spike_row(C):
    short = lambda z: z[..., :-1].sum(-1, keepdim=True) / C
    assert _worst_on("spike", C, dict(mean_of=short, var_of=_VAR, rstd_of=_RSTD), quantities=("mean", "y")) > lc.K


def test_a_wrong_row_is_named_and_a_non_finite_element_fails():
    z, where, gamma, beta, dy, tz = _case(128, 0)
    want, bound = lc.reference(z, gamma, beta, dy, tz), lc.bounds(z, gamma, beta, dy, tz)
    got = {q: t.clone() for q, t in want.items()}
    assert lc.failures("exact", got, want, bound, where, lc.FORWARD + lc.FIRST + lc.SECOND) == []
    row = _rows_named(where, "huge")[0]
    got["dz"][row, 5] *= 1 + 1e-3                      # one element of one row among 67, relative 1e-3
    got["y"][3, 7] = float("nan")
    got["mean"][_rows_named(where, "zero")[0]] = 1e-30      # a zero row's mean is exactly 0
    lines = lc.failures("t", got, want, bound, where, lc.FORWARD + lc.FIRST + lc.SECOND)
    assert len(lines) == 3
    assert any(f"dz row {row} (huge)" in ln for ln in lines) and any("y row 3" in ln and "inf" in ln for ln in lines)
    assert any("(zero)" in ln and "mean" in ln for ln in lines)
    # bf16: one bf16 rounding of the output passes, two units do not
    zb, whereb, gb, bb, _, _ = _case(128, 1, torch.bfloat16)
    wantb, boundb = lc.reference(zb, gb, bb), lc.bounds(zb, gb, bb)
    assert lc.failures("bf16", dict(y=wantb["y"].bfloat16()), wantb, boundb, whereb, ("y",), bf16=True) == []
    assert lc.failures("bf16", dict(y=wantb["y"] * (1 + 2.0 ** -6)), wantb, boundb, whereb, ("y",), bf16=True)
