"""The input cases of tests/attn_range_cases.py are what they claim, and the bars of tests/test_hip_attn_range.py are
reachable by the reference alone (no GPU): float32 torch on the CPU stands in for a correct float32 kernel."""
import pytest
import torch

import attn_range_cases as arc

B = 3
SHAPES = arc.SHORT_SHAPES + [s for s in arc.LONG_SHAPES if s not in arc.SHORT_SHAPES]
# where a row has enough neighbours for the statistics the issue quotes ((3,49,16) ... (3,256,8))
WIDE = [(49, 16), (48, 128), (96, 64), (97, 8), (129, 32), (193, 32), (256, 8)]


def _spread(s):
    return (s.max(2).values - s.min(2).values)


@pytest.mark.parametrize("N,C", WIDE)
def test_existing_data_needs_no_max_subtraction_and_saturated_does(N, C):
    normal = arc.scores(arc.core_case("normal", B, N, C))
    assert arc.naive_softmax_broken(normal) == 0.0 and float(_spread(normal).max()) < 80
    s = arc.scores(arc.core_case("saturated", B, N, C))
    broken = arc.naive_softmax_broken(s)
    print(f"saturated N={N} C={C}: row max {float(s.max(2).values.max()):.3g}, median spread "
          f"{float(_spread(s).median()):.3g}, naive float32 exp broken in {100 * broken:.0f} %")
    assert broken >= 0.5
    assert float(s.max(2).values.max()) > 1e3 and float(_spread(s).median()) > 100


@pytest.mark.parametrize("N,C", SHAPES)
def test_far_negative_has_every_row_maximum_far_below_zero(N, C):
    s = arc.scores(arc.core_case("far_negative", B, N, C))
    m = s.max(2).values
    assert float(m.max()) <= -150
    assert arc.naive_softmax_broken(s) == 1.0           # exp(s - 0) == 0 for every neighbour: 0 / 0
    assert bool((torch.exp(s.float()) == 0).all())
    assert float(s.min()) > -1e4      # and nothing near the float32 range: the scores themselves are ordinary numbers


@pytest.mark.parametrize("case", ["max_last", "max_first"])
@pytest.mark.parametrize("N,C", SHAPES)
def test_the_dominant_neighbour_sits_where_the_case_says(N, C, case):
    s = arc.scores(arc.core_case(case, B, N, C))
    at = N - 1 if case == "max_last" else 0
    assert bool((s.argmax(2) == at).all())
    if N > 1:       # by a margin: exp(-4) of the weight at most for any other neighbour
        top2 = s.topk(2, dim=2).values
        assert float((top2[:, :, 0] - top2[:, :, 1]).min()) > 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,C", SHAPES)
def test_ties_have_an_exactly_zero_gate(N, C, dtype):
    ops = arc.core_case("ties", B, N, C, dtype)
    e = ops["e"]
    assert set(e.unique().tolist()) <= {0.0, -1.0} and (N == 1 or e.unique().numel() == 2)
    assert bool((e * e + e == 0).all()) and bool((arc.scores(ops) == 0).all())
    ref = arc.core_reference(ops)
    assert torch.equal(ref["o"], ops["v"].mean(1, keepdim=True).expand_as(ref["o"]).contiguous()) or \
        arc.row_err(ref["o"], ops["v"].mean(1, keepdim=True).expand_as(ref["o"]), B, N) < 1e-15
    assert bool((ref["dq"] == 0).all()) and bool((ref["dk"] == 0).all())


def test_half_cases_reach_the_same_score_regimes():
    N = 49
    for case, check in (("saturated", lambda s: arc.naive_softmax_broken(s) >= 0.5),
                        ("far_negative", lambda s: arc.naive_softmax_broken(s) == 1.0 and float(s.max()) <= -150),
                        ("max_last", lambda s: bool((s.argmax(2) == N - 1).all())),
                        ("max_first", lambda s: bool((s.argmax(2) == 0).all())),
                        ("ties", lambda s: bool((s == 0).all()))):
        for dtype in (torch.float32, torch.bfloat16):
            h = arc.half_case(case, B, N, dtype)
            s = arc.half_forward_reference(h, wdtype=torch.bfloat16 if dtype == torch.bfloat16 else None)["s"]
            assert check(s), (case, dtype)


@pytest.mark.parametrize("case", arc.CORE_CASES)
@pytest.mark.parametrize("N,C", SHAPES)
def test_float32_reference_is_finite_and_meets_the_float32_bars_in_another_summation_order(N, C, case):
    """What the GPU test asks of a float32 kernel -- row_err <= max(TOL, 2 E_ref) first order, max(5 TOL, 2 E_ref) second
    order -- holds for the float32 reference itself when its sums run over the neighbours in an order that E_ref was not
    measured in.  E_ref is the worst of three orders (arc.reference_orders): with one dominant neighbour the second
    order's true results are exp(-gap) small against their terms, and the float32 error of ONE order then depends on where
    the dominant term enters the sums -- between the given and the reversed order it differs by up to 150x
    ((3,193,32) max_last gq: 1.3e-6 against 1.9e-4), so a single order is no measure of what float32 can reach."""
    ops = arc.core_case(case, B, N, C)
    want = arc.core_reference(ops)
    e_ref = arc.reference_error(ops, want, B, N)
    other = torch.randperm(N, generator=torch.Generator().manual_seed(1000 + N))
    got = arc.core_reference(ops, dtype=torch.float32, order=other)
    for name in arc.FIRST + arc.SECOND:
        assert bool(torch.isfinite(got[name]).all()) and bool(torch.isfinite(want[name]).all()), name
        assert e_ref[name] < float("inf"), name
        err = arc.row_err(got[name], want[name], B, N)
        assert err <= arc.float32_bar(name, e_ref[name]), (name, err, e_ref[name])


def test_row_err_sees_one_wrong_row_in_a_tiny_molecule_and_the_whole_tensor_norm_does_not():
    N, C = 49, 16
    ops = arc.core_case("molecule_scales", B, N, C)
    want = arc.core_reference(ops)["o"]
    assert float(want[0].abs().max()) < 1e-10 < 1e10 < float(want[2].abs().max())
    got = want.clone()
    got[0, 7] *= 1 + 1e-4
    assert arc.rel(got, want) < 1e-20
    assert 0.5e-4 < arc.row_err(got, want, B, N) < 2e-4
    # an edge tensor in its [R, C] flattening, and a non-finite element
    de = arc.core_reference(ops)["de"]
    bad = de.clone()
    bad[1, 3] *= 1 + 1e-4
    assert 0.5e-4 < arc.row_err(bad.reshape(-1, C), de, B, N) < 2e-4
    bad[2, 0, 0, 0] = float("nan")
    assert arc.row_err(bad, de, B, N) == float("inf")
    assert arc.row_err(de, de, B, N) == 0.0
