"""GPU tests of the canonical forms (`dg_mol_canon`, `dg_mol_canon_match` through `druggen_amd.canon`) against the plain-Python
restatement of tests/mol_canon_ref.py.  Batches are built from label tensors -- logits = 4 x one-hot -- so the decode is known;
the reference molecules come from tests/decode_graph_ref.py, not from the GPU decode.  Every output is an integer: every
comparison is `==`."""
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import decode_graph_ref as dref
import mol_canon_ref as ref

pytestmark = pytest.mark.gpu

M = 4      # atom labels 0..3


def _decode(atoms, labels, E, cap=None, out=None):
    from druggen_amd import decode
    node, edge = dref.one_hot_logits(atoms, labels, M, E)
    return decode.decode_molecule_graphs(torch.from_numpy(4.0 * node).cuda(), torch.from_numpy(4.0 * edge).cuda(),
                                         bond_cap=cap, out=out)


def _mols(atoms, labels):
    return [dref.decode_labels(atoms[b], labels[b]) for b in range(len(atoms))]


def _finish(*objects, limit=20.0):
    """Wait for the launches so far with a time limit of this step's own (the kernels' loops are bounded; this bounds the
    test's patience too), then hand back the host copies."""
    done = torch.cuda.Event()
    done.record()
    deadline = time.monotonic() + limit
    while not done.query():
        if time.monotonic() > deadline:
            pytest.fail(f"the GPU step did not finish within {limit} s")
    return [o.cpu() for o in objects]


def _check(atoms, labels, E, cap=None, scope="largest", stock=None, key_bits=64):
    """Forms and matches of the batch against the restatement; the form read back through `order` is the input."""
    from druggen_amd import canon
    forms = canon.canonical_forms(_decode(atoms, labels, E, cap), scope)
    want = ref.canon_batch(_mols(atoms, labels), cap, canon.SCOPES[scope])
    stock_set = stock_want = None
    if stock is not None:
        s_atoms, s_labels = stock
        stock_set = canon.CanonicalSet.from_forms(canon.canonical_forms(_decode(s_atoms, s_labels, E), scope), key_bits)
        stock_want = ref.canon_batch(_mols(s_atoms, s_labels), None, canon.SCOPES[scope])
    matches = canon.match_forms(forms, stock_set, key_bits)
    forms, matches = _finish(forms, matches)
    ref.assert_forms_equal(forms, want)
    for b, w in enumerate(want):
        if w["n_splits"] >= 0:
            n, nb = int(forms.n_atoms[b]), int(forms.n_bonds[b])
            ref.check_order(atoms[b], labels[b], forms.order[b, :n].tolist(), forms.canon_atoms[b, :n].tolist(),
                            forms.canon_bonds[b, :nb, :3].tolist())
    match, tot = ref.match(want, stock_want)
    assert np.array_equal(matches.match, match), (matches.match[(matches.match != match).any(1)], match[(matches.match != match).any(1)])
    assert np.array_equal(matches.tot, tot), (matches.tot, tot)
    return forms, matches


def _clip(labels, E):
    return np.minimum(labels, E - 1)


def _stack(graphs):
    return np.stack([g[0] for g in graphs]), np.stack([g[1] for g in graphs])


def _family(name, rng, B, N, E):
    """B molecules of N positions, labels below E."""
    if name in ("molecule-like", "one label"):
        graphs = [ref.molecule_like(rng, N, (0, 1, 2, 4)[b % 4], name == "one label") for b in range(B)]
    elif name == "dense":      # a random label per pair: the untrained generator's regime
        graphs = [(rng.integers(0, M, N), np.tril(rng.integers(0, E, (N, N)), -1)) for _ in range(B)]
    elif name == "no bonds":
        graphs = [(np.full(N, 1 + b % 2), dref.empty_graph(N)) for b in range(B)]
    elif name == "all pad":
        graphs = [(np.zeros(N, dtype=np.int64), dref.empty_graph(N)) for _ in range(B)]
    elif name == "cycles and a star":
        graphs = [ref.cycle(N) if b % 2 == 0 else (np.ones(N, dtype=np.int64), dref.star(N, b % N)) for b in range(B)]
    else:                      # two components of equal size (N even) or sizes that differ by one
        graphs = [(1 + (np.arange(N) + b) % 2 * (b % 2), dref.two_equal_components(N)) for b in range(B)]
    atoms, labels = _stack(graphs)
    return atoms, _clip(labels, E)


FAMILIES = ("molecule-like", "one label", "dense", "no bonds", "all pad", "cycles and a star", "two components")
SHAPES = [(1, 1), (3, 2), (5, 9), (4, 45), (3, 64), (3, 65), (2, 256), (257, 5)]


@pytest.mark.parametrize("E", [2, 5])
@pytest.mark.parametrize("B,N", SHAPES)
def test_forms_match_the_restatement(B, N, E):
    """Every family at this shape, with an ample bond list and with one a row short of the largest molecule (truncation); the two
    components under both scopes.  (2, 256) holds the worst case: no bonds and one label take 255 splits."""
    rng = np.random.default_rng([B, N, E])
    for name in FAMILIES:
        atoms, labels = _family(name, rng, B, N, E)
        scopes = ("largest", "whole") if name in ("two components", "all pad", "molecule-like") else ("largest",)
        most = max(int(np.count_nonzero(l)) for l in labels)
        for scope in scopes:
            forms, _ = _check(atoms, labels, E, scope=scope)
            if name == "no bonds" and scope == "largest":
                assert (forms.n_atoms == 1).all()
        forms, matches = _check(atoms, labels, E, scope="whole", cap=max(most - 1, 0))
        if most > 0:
            assert matches.total("n_truncated") >= 1 and (forms.n_splits == -2).any()
        if name == "no bonds":
            assert (forms.n_splits == N - 1).all() and (forms.n_rounds == N).all()


def test_all_graphs_on_five_vertices_are_34_distinct_forms():
    pairs = [(i, j) for i in range(5) for j in range(i)]
    atoms, labels = _stack([ref.from_edges(5, [pairs[k] for k in range(10) if mask >> k & 1]) for mask in range(1 << 10)])
    forms, matches = _check(atoms, labels, 2, scope="whole")
    assert matches.total("n_distinct") == 34 and matches.unique_fraction == 34 / 1024
    assert len({forms.form(b) for b in range(1024)}) == 34


def _planted(rng, N=12):
    """A batch with renumbered copies of molecules 0 and 1 planted at 3, 5 and 6, and a stock with renumbered copies of 1 and 4."""
    base = [ref.molecule_like(rng, N, c) for c in (1, 2, 0, 4, 2)]
    again = lambda g: ref.renumbered(rng, *g)
    batch = [base[0], base[1], base[2], again(base[0]), base[3], again(base[1]), again(base[0]), base[4]]
    stock = [ref.molecule_like(rng, N, 1), again(base[4]), ref.molecule_like(rng, N, 2), again(base[1]), again(base[4])]
    return _stack(batch), _stack(stock)


def test_planted_renumberings_are_found_and_the_positional_statistics_miss_them():
    from druggen_amd import monitor
    (atoms, labels), stock = _planted(np.random.default_rng(77))
    for b in (3, 5, 6):      # renumbered for real: no copy is positionally equal to its original
        src = {3: 0, 5: 1, 6: 0}[b]
        assert not (np.array_equal(atoms[b], atoms[src]) and np.array_equal(labels[b], labels[src]))
    forms, matches = _check(atoms, labels, 5, stock=stock)
    assert matches.duplicate_of.tolist() == [-1, -1, -1, 0, -1, 1, 0, -1]
    assert matches.stock_hit.tolist() == [-1, 3, -1, -1, -1, 3, -1, 1]
    assert matches.total("n_distinct") == 5 and matches.total("n_in_stock") == 3 and matches.total("n_novel") == 5
    assert matches.unique_fraction == 5 / 8 and matches.novel_fraction == 5 / 8
    positional = monitor.molecule_statistics(_decode(atoms, labels, 5)).cpu()
    assert positional.column("duplicate_of").tolist() == [-1] * 8 and positional.distinct_fraction == 1.0


def test_result_does_not_depend_on_the_key_width():
    """At 1 bit about every second pair of forms is a key match, so the byte comparison carries the result -- in the batch and in
    the stock, which is sorted under the same width."""
    rng = np.random.default_rng(17)
    B, N = 70, 9
    pool = [ref.molecule_like(rng, N, k % 3) for k in range(6)]
    batch = [ref.renumbered(rng, *pool[k]) for k in rng.integers(0, 6, B)]
    for b in range(0, B, 5):      # near misses: one atom label or one bond label away
        a, l = batch[b]
        if b % 2:
            a = a.copy()
            a[b % N] = 1 + a[b % N] % 3
        else:
            i, j = np.argwhere(l)[0]
            l = l.copy()
            l[i, j] = 1 + l[i, j] % 4
        batch[b] = (a, l)
    atoms, labels = _stack(batch)
    stock = _stack([ref.renumbered(rng, *pool[k]) for k in (4, 2, 4, 0)] + [batch[5], batch[10]])
    results = [_check(atoms, labels, 5, stock=stock, key_bits=bits)[1] for bits in (1, 2, 64)]
    assert all(np.array_equal(r.buffer, results[0].buffer) for r in results[1:])
    assert results[0].total("n_distinct") <= 6 + 14 and results[0].total("n_in_stock") > 0 < results[0].total("n_novel")


def test_stock_run_longer_than_one_step_of_the_scan():
    """600 stock forms under 1 key bit: a run of equal keys is longer than the 256 positions the four waves cover per step, so
    the scan of the stock takes a second step (within the batch only B = 257 gets that far).  One form's only copies sit at the
    original indices 450 and 590 -- in different steps of the scan -- and the smaller one is reported; another's only copy at 530."""
    from druggen_amd import canon
    rng = np.random.default_rng(600)
    N, E, S = 9, 5, 600
    stock = [ref.molecule_like(rng, N, k % 3) for k in range(S)]
    batch = [ref.molecule_like(rng, N, k % 3) for k in range(8)]
    stock[450], stock[590] = ref.renumbered(rng, *batch[2]), ref.renumbered(rng, *batch[2])
    stock[530] = ref.renumbered(rng, *batch[5])
    stock = _stack(stock)
    keys = canon.CanonicalSet.from_forms(canon.canonical_forms(_decode(*stock, E)), key_bits=1).keys
    assert set(keys.tolist()) <= {0, 1} and max(int((keys == 0).sum()), int((keys == 1).sum())) > 256
    _, matches = _check(*_stack(batch), E, stock=stock, key_bits=1)
    assert matches.duplicate_of.tolist() == [-1] * 8
    assert matches.stock_hit.tolist() == [-1, -1, 450, -1, -1, 530, -1, -1]


def test_two_launches_are_bit_identical_and_no_output_is_stale():
    from druggen_amd import canon
    rng = np.random.default_rng(31)
    atoms, labels = _family("molecule-like", rng, 6, 45, 5)
    atoms[4], labels[4] = ref.renumbered(rng, atoms[1], labels[1])
    labels[5] = np.tril(rng.integers(0, 5, (45, 45)), -1)      # more bonds than the list below holds: truncated
    cap = 60
    batch = _decode(atoms, labels, 5, cap)
    stock = canon.CanonicalSet.from_forms(canon.canonical_forms(_decode(atoms[1:3], labels[1:3], 5, cap)))
    outs = []
    for fill in (0x00, 0xFF, 0xFF):
        forms, matches = canon.CanonicalForms.empty(6, 45, cap, "cuda"), canon.FormMatches.empty(6, "cuda")
        forms.buffer.fill_(fill)
        matches.buffer.fill_(fill)
        assert canon.canonical_forms(batch, out=forms) is forms and canon.match_forms(forms, stock, out=matches) is matches
        outs.append(_finish(forms, matches))
    assert np.array_equal(outs[1][0].buffer, outs[2][0].buffer) and np.array_equal(outs[1][1].buffer, outs[2][1].buffer)
    # over zeros and over 0xFF every FIELD is the same (the packed buffer has alignment gaps between its fields)
    for name in ("n_atoms", "n_bonds", "n_splits", "n_rounds", "key", "order", "canon_atoms", "canon_bonds"):
        assert np.array_equal(getattr(outs[0][0], name), getattr(outs[1][0], name)), name
    assert np.array_equal(outs[0][1].buffer, outs[1][1].buffer)
    ref.assert_forms_equal(outs[0][0], ref.canon_batch(_mols(atoms, labels), cap))
    assert outs[0][1].match.tolist() == [[-1, -1], [-1, 0], [-1, 1], [-1, -1], [1, 0], [-2, -2]]
    # an empty batch writes its totals too
    empty = canon.FormMatches.empty(0, "cuda")
    empty.buffer.fill_(0xFF)
    none = canon.canonical_forms(_decode(atoms[:0], labels[:0], 5, cap))
    assert canon.match_forms(none, stock, out=empty).cpu().tot.tolist() == [0] * 8
    with pytest.raises(ValueError, match="out="):
        canon.canonical_forms(batch, out=canon.CanonicalForms.empty(5, 45, cap, "cuda"))
    with pytest.raises(ValueError, match="out="):
        canon.match_forms(forms_dev := canon.canonical_forms(batch), out=canon.FormMatches.empty(5, "cuda"))
    with pytest.raises(ValueError, match="key_bits"):
        canon.match_forms(forms_dev, stock, key_bits=8)
    with pytest.raises(ValueError, match="N = 9"):
        canon.match_forms(forms_dev, canon.CanonicalSet.from_forms(canon.canonical_forms(_decode(atoms[:1, :9], labels[:1, :9, :9], 5))))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        canon.canonical_forms(batch.cpu())


@functools.lru_cache(maxsize=None)
def _store_graphs(n, N, E, seed):
    """Molecule-like graphs as the per-molecule objects `ResidentMolecules.from_graphs` takes, and as label arrays."""
    rng = np.random.default_rng([n, N, E, seed])
    atoms, labels = _family("molecule-like", rng, n, N, E)
    graphs = []
    for a, l in zip(atoms, labels):
        x = np.zeros((N, M), dtype=np.float32)
        x[np.arange(N), a] = 1.0
        full = l + l.T
        src, dst = np.nonzero(full)
        graphs.append(SimpleNamespace(x=x, edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=full[src, dst]))
    return tuple(graphs), atoms, labels


def test_canonical_set_from_a_resident_store_in_uneven_chunks():
    from druggen_amd import canon
    from druggen_amd.resident import ResidentMolecules
    graphs, atoms, labels = _store_graphs(11, 9, 5, 1)
    store = ResidentMolecules.from_graphs(graphs, device="cuda", m_dim=M, b_dim=5)
    want = ref.canon_batch(_mols(atoms, labels))
    sets = [canon.CanonicalSet.from_store(store, chunk=chunk) for chunk in (4, 11, 64)]
    for s in sets:
        assert len(s) == 11 and s.key_bits == 64
        ref.assert_forms_equal(s.forms.cpu(), want)
        keys, index = s.keys.cpu().numpy(), s.index.cpu().numpy()
        assert np.array_equal(keys, np.sort([w["key"] for w in want])) and sorted(index.tolist()) == list(range(11))
        assert np.array_equal(keys, np.array([want[i]["key"] for i in index]))
    # the store's own molecules, renumbered, are all found in it
    rng = np.random.default_rng(5)
    again = _stack([ref.renumbered(rng, atoms[k], labels[k]) for k in (10, 0, 3)])
    _, matches = canon.uniqueness_novelty(_decode(*again, 5), stock=sets[0])
    hits = ref.match(ref.canon_batch(_mols(*again)), want)[0][:, 1].tolist()
    assert matches.cpu().stock_hit.tolist() == hits and all(h >= 0 for h in hits) and matches.cpu().novel_fraction == 0.0
    with pytest.raises(ValueError, match="scope"):
        canon.uniqueness_novelty(_decode(*again, 5), stock=sets[0], scope="whole")


def test_decode_forms_and_matches_replay_from_a_captured_graph():
    """The three calls captured into one hipGraph, replayed on new logits: the eager results."""
    from druggen_amd import canon, decode
    rng = np.random.default_rng(41)
    B, N, E = 5, 9, 5
    sets = []
    for k in range(3):
        atoms, labels = _family("molecule-like", rng, B, N, E)
        atoms[B - 1], labels[B - 1] = ref.renumbered(rng, atoms[k], labels[k])
        sets.append((atoms, labels))
    stock = canon.CanonicalSet.from_forms(canon.canonical_forms(_decode(*sets[1], E)))
    stock_want = ref.canon_batch(_mols(*sets[1]))
    node, edge = (torch.from_numpy(4.0 * t).cuda() for t in dref.one_hot_logits(*sets[0], M, E))
    decoded = decode.MoleculeBatch.empty(B, N, N * (N - 1) // 2, False, "cuda")
    forms, matches = canon.CanonicalForms.empty(B, N, decoded.cap, "cuda"), canon.FormMatches.empty(B, "cuda")

    def chain():
        decode.decode_molecule_graphs(node, edge, out=decoded)
        canon.canonical_forms(decoded, out=forms)
        canon.match_forms(forms, stock, out=matches)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    seen = []
    for k, (atoms, labels) in enumerate(sets[1:] + sets[:1]):
        n, e = dref.one_hot_logits(atoms, labels, M, E)
        node.copy_(torch.from_numpy(4.0 * n))
        edge.copy_(torch.from_numpy(4.0 * e))
        forms.buffer.fill_(0xFF)
        matches.buffer.fill_(0xFF)
        graph.replay()
        got_forms, got = _finish(forms, matches)
        want = ref.canon_batch(_mols(atoms, labels))
        ref.assert_forms_equal(got_forms, want)
        match, tot = ref.match(want, stock_want)
        assert np.array_equal(got.match, match) and np.array_equal(got.tot, tot)
        assert got.duplicate_of[B - 1] == (k + 1) % 3
        seen.append(got.match.copy())
    assert seen[0][:, 1].tolist() == [0, 1, 2, 3, 1] and not np.array_equal(seen[0], seen[1])


def test_sampler_output_goes_straight_into_uniqueness_and_novelty():
    """`MoleculeSampler.sample` -> `uniqueness_novelty(batch, stock=drug_set)`: what the generator made, against the restatement."""
    from druggen_amd import canon, synth
    from druggen_amd.model import Generator
    from druggen_amd.resident import ResidentMolecules
    from druggen_amd.sampling import MoleculeSampler
    N, E, Mn, B = 9, 5, 13, 4
    net = Generator("relu", N, E, Mn, 0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
    params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=11)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    graphs, atoms, labels = _store_graphs(7, N, E, 2)
    for g in graphs:
        g.x = np.pad(g.x, ((0, 0), (0, Mn - g.x.shape[1])))
    drugs = ResidentMolecules.from_graphs(graphs, device="cuda", m_dim=Mn, b_dim=E)
    drug_set = canon.CanonicalSet.from_store(drugs, chunk=3)
    _, a, x = drugs.batch(torch.tensor([6, 2, 2, 0], device="cuda"))
    sampler = MoleculeSampler(net.cuda(), a, x, graph=False)
    batch = sampler.sample(a, x)
    forms, matches = canon.uniqueness_novelty(batch, stock=drug_set)
    host, forms, matches = _finish(batch, forms, matches)
    mols = [dict(atoms=host.atoms[b], bonds=host.edge_list(b), n_bonds=int(host.n_bonds[b]), component=host.component[b],
                 largest=int(host.largest[b])) for b in range(B)]
    want = ref.canon_batch(mols)
    ref.assert_forms_equal(forms, want)
    match, tot = ref.match(want, ref.canon_batch(_mols(atoms, labels)))
    assert np.array_equal(matches.match, match) and np.array_equal(matches.tot, tot)
    assert matches.total("B") == B and 0.0 <= matches.unique_fraction <= 1.0
