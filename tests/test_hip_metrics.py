"""GPU tests of the fingerprint metrics (`dg_fp_pack`, `dg_fp_tanimoto` through druggen_amd/metrics.py): against what the
reference returned on the seeded main case (tests/golden/tanimoto_ref.npz) and against the exact numpy restatement of
tests/tanimoto_ref.py over the shapes the kernel's tiling distinguishes.  Maxima and indices are compared exactly; a
mean is a float64 sum of float32 quotients, each carrying one rounding of at most 2^-24 relative, so it lies within
2^-23 (relative) of the exact mean -- float64 accumulation is negligible beside that."""
import os

import numpy as np
import pytest
import torch

import tanimoto_cases as tc
import tanimoto_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tanimoto_ref.npz")
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def case():
    return tc.default_case()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _within(ours, reference, exact):
    """|ours - ref| <= |ref - exact| + 2^-23 exact (triangle inequality through the exact value) and |ours - exact| <= 2^-23 exact."""
    ours, reference, exact = (np.asarray(v, dtype=np.float64) for v in (ours, reference, exact))
    print(f"max |ours - ref| = {np.max(np.abs(ours - reference)):.3e}, max |ref - exact| = {np.max(np.abs(reference - exact)):.3e}, "
          f"max |ours - exact| / exact = {np.max(np.abs(ours - exact) / np.abs(exact)):.3e}")
    assert np.all(np.abs(ours - reference) <= np.abs(reference - exact) + EPS * np.abs(exact))
    assert np.all(np.abs(ours - exact) <= EPS * np.abs(exact))


def test_main_case_max_and_snn_equal_the_reference_bit_for_bit(case, golden):
    from druggen_amd import metrics
    got = metrics.average_agg_tanimoto(case["stock"], case["gen"], agg="max", intdiv=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (tc.GEN,)
    assert np.array_equal(got, golden["max"])
    snn = metrics.average_agg_tanimoto(case["stock"], case["gen"])
    assert isinstance(snn, float) and snn == float(golden["snn"])
    want = ref.aggregate(case["stock"], case["gen"])
    sim, idx = metrics.tanimoto_aggregate(case["stock"], case["gen"], return_index=True)
    assert sim.dtype == torch.float64 and idx.dtype == torch.int32 and sim.is_cuda and idx.is_cuda
    assert np.array_equal(sim.cpu().numpy(), golden["max"])
    assert np.array_equal(idx.cpu().numpy(), want["idx"])
    assert int(idx[100]) == 200 and float(sim[100]) == 1.0           # the duplicate row
    assert int(idx[7]) == 11 and float(sim[7]) == 1.0                # empty gen row: 0 / 0 -> 1 at the empty stock row
    # an empty gen row against a stock without an empty row: every quotient is 0, the tie goes to index 0
    sim0, idx0 = metrics.tanimoto_aggregate(np.delete(case["stock"], 11, axis=0), case["gen"][7:8], return_index=True)
    assert float(sim0[0]) == 0.0 and int(idx0[0]) == 0


def test_main_case_mean_within_the_derived_bound(case, golden):
    from druggen_amd import metrics
    got = metrics.average_agg_tanimoto(case["stock"], case["gen"], agg="mean", intdiv=True)
    assert got.dtype == np.float64
    want = ref.aggregate(case["stock"], case["gen"])
    _within(got, golden["mean"], want["exact_mean"])
    assert np.array_equal(got, want["mean"]) or np.max(np.abs(got - want["mean"])) <= 2.0 ** -50      # same terms, other summation order


def test_internal_diversity_within_the_derived_bound(case, golden):
    from druggen_amd import metrics
    mean, std = metrics.internal_diversity(case["self"])
    exact = 1 - ref.aggregate(case["self"], case["self"])["exact_mean"]
    _within([mean, std], golden["intdiv"], [np.mean(exact), np.std(exact)])
    packed = metrics.pack_fingerprints(case["self"])
    assert metrics.internal_diversity(packed) == (mean, std)


def _compare(stock, gen, want=None):
    from druggen_amd import metrics
    want = want or ref.aggregate(stock, gen)
    ps, pg = metrics.pack_fingerprints(stock), metrics.pack_fingerprints(gen)
    sim, idx = metrics.tanimoto_aggregate(ps, pg, return_index=True)
    assert np.array_equal(sim.cpu().numpy(), want["max"].astype(np.float64))
    assert np.array_equal(idx.cpu().numpy(), want["idx"])
    assert torch.equal(metrics.tanimoto_aggregate(ps, pg), sim)      # without the index output
    mean = metrics.tanimoto_aggregate(ps, pg, agg="mean").cpu().numpy()
    exact = want["exact_mean"]
    assert np.all(np.abs(mean - exact) <= EPS * exact)
    return sim, idx, mean


SPLIT_S = 40000      # rows of a stock that is cut into several slices at every G below (the header's slice rule)


@pytest.mark.parametrize("G", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("S", [1, 2, 255, 6001, SPLIT_S])
def test_shapes_match_restatement(S, G):
    from druggen_amd import _lib
    stock, gen = tc.shape_case(S, G, 1024, 1000 * G + S)
    if S > 300:
        gen[0] = stock[S - 1]          # a maximum in the last slice
        stock[S // 2] = stock[3]       # a tie across slices: the smaller index wins
        gen[G - 1] = stock[3]
    need = _lib.load().dg_fp_tanimoto_workspace_bytes(S, G)
    assert (need > 0) == (S >= 255), "the slice rule moved: S = 1, 2 take one slice, 255 and above several"
    sim, idx, _ = _compare(stock, gen)
    if S > 300:
        assert int(idx[G - 1]) == 3 and float(sim[G - 1]) == 1.0
        if G > 1:
            assert int(idx[0]) == S - 1


@pytest.mark.parametrize("nbits", [1024, 2048])
@pytest.mark.parametrize("S,G", [(6001, 1100), (SPLIT_S, 1025)])
def test_split_ties_with_many_gen_blocks(S, G, nbits):
    """More than a thousand gen rows at both specialised widths, several slices and the combine launch -- with a maximum in the
    last slice, ties placed across slices and a row whose quotients are all 0."""
    from druggen_amd import _lib
    stock, gen = tc.shape_case(S, G, nbits, 7 * G + S + nbits)
    gen[0] = stock[S - 1]
    stock[S // 2] = stock[3]
    stock[S - 2] = stock[3]
    gen[G - 1] = stock[3]
    gen[64] = stock[3]
    gen[G // 2] = 0                    # all quotients 0: the tie over every slice goes to index 0
    assert _lib.load().dg_fp_tanimoto_workspace_bytes(S, G) // (8 * G) > 2
    sim, idx, _ = _compare(stock, gen)
    assert int(idx[0]) == S - 1 and int(idx[G - 1]) == 3 and int(idx[64]) == 3 and float(sim[64]) == 1.0
    assert int(idx[G // 2]) == 0 and float(sim[G // 2]) == 0.0


@pytest.mark.parametrize("nbits", [32, 96, 1024, 2048, 4096])
@pytest.mark.parametrize("S,G", [(2, 1), (128, 65), (700, 130), (300, 1100)])
def test_every_word_count_matches_restatement(nbits, S, G):
    stock, gen = tc.shape_case(S, G, nbits, nbits + S)
    stock[S - 1, nbits - 1] = 1        # the last bit of the last word counts
    gen[G - 1] = 0
    gen[G - 1, nbits - 1] = 1
    _compare(stock, gen)


def test_empty_rows_and_identical_sets():
    stock, gen = tc.shape_case(300, 70, 1024, 77)
    zeros = np.zeros_like(stock)
    sim, idx, mean = _compare(zeros, gen)                      # all-zero stock: every quotient is 0
    assert not sim.any() and not idx.any() and not mean.any()
    sim, idx, mean = _compare(stock, np.zeros_like(gen))       # all-zero gen
    assert not sim.any() and not idx.any()
    sim, idx, mean = _compare(zeros, np.zeros_like(gen))       # both: 0 / 0 -> 1 everywhere
    assert (sim == 1).all() and not idx.any() and (mean == 1).all()
    sim, idx, _ = _compare(stock, stock.copy())                # stock identical to gen
    assert (sim == 1).all() and np.array_equal(idx.cpu().numpy(), np.arange(300))


@pytest.mark.parametrize("nbits", [32, 96, 1024, 2048])
def test_device_packing_equals_host_packing(nbits):
    from druggen_amd import metrics
    rng = np.random.default_rng(nbits)
    bits = tc.random_bits(rng, 131, nbits, 0.0, 0.6)
    words, counts = tc.pack_host(bits), bits.sum(1)
    with np.errstate(invalid="ignore"):
        soft = bits.astype(np.float32) * rng.choice(np.array([-2.5, 0.125, 1.0, 3e-39, np.inf, np.nan], np.float32), size=bits.shape)
    soft[bits == 0] = rng.choice(np.array([0.0, -0.0], np.float32), size=int((bits == 0).sum()))
    for dense in (torch.from_numpy(bits), torch.from_numpy(bits.astype(bool)), torch.from_numpy(bits * 201), torch.from_numpy(soft),
                  torch.from_numpy(bits.astype(np.int64))):
        got = metrics.pack_fingerprints(dense.cuda())
        assert got.nbits == nbits and got.words.dtype == torch.int32 and got.counts.dtype == torch.int32
        assert np.array_equal(got.words.cpu().numpy().view(np.uint32), words), dense.dtype
        assert np.array_equal(got.counts.cpu().numpy(), counts), dense.dtype
    up = metrics.pack_fingerprints(bits)                       # the host route uploads the same words
    assert np.array_equal(up.words.cpu().numpy().view(np.uint32), words) and np.array_equal(up.counts.cpu().numpy(), counts)


def test_two_runs_and_a_side_stream_give_the_same_bits():
    from druggen_amd import metrics
    stock, gen = tc.shape_case(20000, 300, 1024, 9)
    ps, pg = metrics.pack_fingerprints(stock), metrics.pack_fingerprints(gen)
    first = [metrics.tanimoto_aggregate(ps, pg, return_index=True), metrics.tanimoto_aggregate(ps, pg, agg="mean")]
    again = [metrics.tanimoto_aggregate(ps, pg, return_index=True), metrics.tanimoto_aggregate(ps, pg, agg="mean")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = [metrics.tanimoto_aggregate(ps, pg, return_index=True), metrics.tanimoto_aggregate(ps, pg, agg="mean")]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for run in (again, other):
        assert torch.equal(run[0][0], first[0][0]) and torch.equal(run[0][1], first[0][1])
        assert torch.equal(run[1].view(torch.int64), first[1].view(torch.int64))


def test_graph_capture_replays_on_new_contents():
    from druggen_amd import metrics
    stock, gen = tc.shape_case(9000, 200, 1024, 21)
    stock2, gen2 = tc.shape_case(9000, 200, 1024, 22)
    dense_s, dense_g = torch.from_numpy(stock).cuda(), torch.from_numpy(gen).cuda()      # the static input buffers
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up outside the capture
        metrics.tanimoto_aggregate(dense_s, dense_g, return_index=True)
        metrics.tanimoto_aggregate(dense_s, dense_g, agg="mean")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # device packing, both aggregations and their combine launches
        sim, idx = metrics.tanimoto_aggregate(dense_s, dense_g, return_index=True)
        mean = metrics.tanimoto_aggregate(dense_s, dense_g, agg="mean")
    dense_s.copy_(torch.from_numpy(stock2))
    dense_g.copy_(torch.from_numpy(gen2))
    graph.replay()
    torch.cuda.synchronize()
    e_sim, e_idx = metrics.tanimoto_aggregate(stock2, gen2, return_index=True)
    e_mean = metrics.tanimoto_aggregate(stock2, gen2, agg="mean")
    assert torch.equal(sim, e_sim) and torch.equal(idx, e_idx) and torch.equal(mean.view(torch.int64), e_mean.view(torch.int64))
    want = ref.aggregate(stock2, gen2)
    assert np.array_equal(sim.cpu().numpy(), want["max"].astype(np.float64)) and np.array_equal(idx.cpu().numpy(), want["idx"])


def test_empty_inputs():
    from druggen_amd import metrics
    bits = tc.random_bits(np.random.default_rng(1), 5, 64)
    none = np.zeros((0, 64), np.uint8)
    for stock, gen in ((bits, none), (none, none)):
        sim, idx = metrics.tanimoto_aggregate(stock, gen, return_index=True)
        assert sim.shape == (0,) and idx.shape == (0,) and sim.dtype == torch.float64 and idx.dtype == torch.int32
        assert metrics.tanimoto_aggregate(stock, gen, agg="mean").shape == (0,)
        assert metrics.average_agg_tanimoto(stock, gen, intdiv=True).shape == (0,)
    # no stock: the reference's values -- nothing raised the zero-initialised maxima, the mean is 0 / 0
    sim, idx = metrics.tanimoto_aggregate(none, bits, return_index=True)
    assert sim.tolist() == [0.0] * 5 and idx.tolist() == [-1] * 5
    assert torch.isnan(metrics.tanimoto_aggregate(none, bits, agg="mean")).all()
    empty = metrics.pack_fingerprints(torch.zeros(0, 64, dtype=torch.uint8, device="cuda"))
    assert empty.words.shape == (0, 2) and empty.counts.shape == (0,)
