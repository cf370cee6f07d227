"""GPU tests of the molecule statistics (`dg_mol_stats` through `monitor.molecule_statistics`) against the numpy restatement of
tests/mol_stats_ref.py.  Batches are built from label tensors -- logits = 4 x one-hot -- so the decode is known; the reference
molecules come from tests/decode_graph_ref.py, not from the GPU decode.  Every output is an integer: every comparison is `==`."""
import numpy as np
import pytest
import torch

import decode_graph_ref as dref
import mol_stats_ref as ref

pytestmark = pytest.mark.gpu


def _order2(E):
    return [0, 2, 4, 6, 3][:E] if E <= 5 else [(3 * k) % 7 for k in range(E)]


def _decode(atoms, labels, M, E, cap=None, out=None):
    from druggen_amd import decode
    node, edge = dref.one_hot_logits(atoms, labels, M, E)
    return decode.decode_molecule_graphs(torch.from_numpy(4.0 * node).cuda(), torch.from_numpy(4.0 * edge).cuda(),
                                         bond_order2=_order2(E), bond_cap=cap, out=out)


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _stats(batch, in_atoms=None, in_labels=None, max_valence2=None, **kw):
    from druggen_amd import monitor
    return monitor.molecule_statistics(batch, in_atoms=_dev(in_atoms, torch.uint8), in_labels=_dev(in_labels, torch.int32),
                                       max_valence2=max_valence2, **kw)


def _want(atoms, labels, E, cap=None, **kw):
    mols = [dref.decode_labels(atoms[b], labels[b], _order2(E)) for b in range(len(atoms))]
    return ref.mol_stats(mols, cap=cap, **kw)


def _check(atoms, labels, M, E, cap=None, in_atoms=None, in_labels=None, max_valence2=None, key_bits=64):
    got = _stats(_decode(atoms, labels, M, E, cap), in_atoms, in_labels, max_valence2, key_bits=key_bits).cpu()
    mol, tot = _want(atoms, labels, E, cap, in_atoms=in_atoms, in_labels=in_labels, max_valence2=max_valence2)
    assert np.array_equal(got.mol, mol), (got.mol[(got.mol != mol).any(1)], mol[(got.mol != mol).any(1)])
    assert np.array_equal(got.tot, tot), (got.tot, tot)
    return got


def _random_graphs(rng, B, N, M, E, density=0.15):
    """Symmetric label matrices with a zero diagonal, as the dataset's (only i > j is decoded)."""
    atoms = rng.integers(0, M, (B, N))
    upper = np.triu((rng.random((B, N, N)) < density) * rng.integers(1, max(E, 2), (B, N, N)), 1) if E > 1 else \
        np.zeros((B, N, N), dtype=np.int64)
    return atoms, upper + upper.transpose(0, 2, 1)


SHAPES = [(1, 1), (3, 2), (5, 9), (65, 45), (257, 9), (3, 64), (3, 65), (2, 97), (2, 256)]


@pytest.mark.parametrize("E,M", [(2, 1), (2, 13), (5, 1), (5, 13)])
@pytest.mark.parametrize("B,N", SHAPES)
def test_statistics_match_the_restatement(B, N, E, M):
    """Random molecules; the input graph is the output with a tenth of the molecules changed, a fifth of the molecules are copies
    of an earlier one, the valence table is tight enough to be exceeded."""
    rng = np.random.default_rng([B, N, E, M])
    atoms, labels = _random_graphs(rng, B, N, M, E)
    for b in range(1, B):
        if rng.random() < 0.2:
            src = int(rng.integers(0, b))
            atoms[b], labels[b] = atoms[src], labels[src]
    in_atoms, in_labels = atoms.copy(), labels.copy()
    for b in range(B):
        if rng.random() < 0.5:
            in_atoms[b, rng.integers(0, N)] = rng.integers(0, M)
            i, j = rng.integers(0, N, 2)
            in_labels[b, i, j] = in_labels[b, j, i] = rng.integers(0, E)
    max_valence2 = [0xFFFF] + [int(v) for v in rng.integers(0, 12, M - 1)]
    if M > 1:
        max_valence2[1] = 0      # any bonded atom of label 1 is over
    got = _check(atoms, labels, M, E, in_atoms=in_atoms, in_labels=in_labels, max_valence2=max_valence2)
    assert got.total("B") == B and got.total("n_truncated") == 0
    if B >= 65:
        assert 0 < got.total("n_copies") < B and got.total("n_distinct") < B
    if B >= 65 and M > 1 and E > 1:
        assert got.total("n_over_valent") > 0


def _base(N=9, M=13, E=5):
    rng = np.random.default_rng(99)
    atoms, labels = _random_graphs(rng, 1, N, M, E, density=0.3)
    atoms[0, 0], labels[0, 3, 1], labels[0, 1, 3], labels[0, 8, 7], labels[0, 7, 8] = 5, 2, 2, 0, 0
    return atoms[0], labels[0]


def test_planted_duplicates():
    """Copies at the first, a middle and the last position (three of a kind: both later ones point to the FIRST); molecules that
    differ from it in one atom, in one bond label, in n_bonds only; a second pair among those."""
    x_atoms, x_labels = _base()
    one_atom = x_atoms.copy()
    one_atom[0] = 6
    one_label = x_labels.copy()
    one_label[3, 1] = one_label[1, 3] = 3
    one_more = x_labels.copy()
    one_more[8, 7] = one_more[7, 8] = 1      # n_bonds differs (the list is the same up to the new last row)
    other_atoms, other_labels = _random_graphs(np.random.default_rng(5), 1, 9, 13, 5)
    graphs = [(x_atoms, x_labels), (one_atom, x_labels), (x_atoms, one_label), (other_atoms[0], other_labels[0]),
              (x_atoms, x_labels), (x_atoms, one_more), (one_atom, x_labels), (x_atoms, one_label), (x_atoms, x_labels)]
    atoms, labels = np.stack([g[0] for g in graphs]), np.stack([g[1] for g in graphs])
    for bits in (64, 1):
        got = _check(atoms, labels, 13, 5, key_bits=bits)
        assert got.column("duplicate_of").tolist() == [-1, -1, -1, -1, 0, -1, 1, 2, 0]
        assert got.total("n_distinct") == 5 and got.distinct_fraction == 5 / 9
    assert got.column("n_bonds")[5] == got.column("n_bonds")[0] + 1


def test_planted_inputs():
    """Identity copies, one changed atom, one bond removed, one bond added -- against the same input graph."""
    x_atoms, x_labels = _base()
    one_atom = x_atoms.copy()
    one_atom[4] = (x_atoms[4] + 1) % 13
    removed = x_labels.copy()
    removed[3, 1] = removed[1, 3] = 0
    added = x_labels.copy()
    added[8, 7] = added[7, 8] = 4
    graphs = [(x_atoms, x_labels), (one_atom, x_labels), (x_atoms, removed), (x_atoms, added), (x_atoms, x_labels)]
    atoms, labels = np.stack([g[0] for g in graphs]), np.stack([g[1] for g in graphs])
    in_atoms, in_labels = np.stack([x_atoms] * 5), np.stack([x_labels] * 5)
    got = _check(atoms, labels, 13, 5, in_atoms=in_atoms, in_labels=in_labels)
    assert got.column("changed_atoms").tolist() == [0, 1, 0, 0, 0]
    assert got.column("changed_bonds").tolist() == [0, 0, 1, 1, 0]
    assert got.total("n_copies") == 2 and got.copy_fraction == 0.4
    # one input alone answers its own column; the copies need both
    got = _check(atoms, labels, 13, 5, in_atoms=in_atoms)
    assert (got.column("changed_bonds") == -1).all() and got.total("n_copies") == 0 and got.total("changed_atoms") == 1
    got = _check(atoms, labels, 13, 5, in_labels=in_labels)
    assert (got.column("changed_atoms") == -1).all() and got.total("changed_bonds") == 2
    # an input of upper-triangle entries only is never read
    got = _check(atoms, labels, 13, 5, in_labels=np.triu(in_labels))
    assert got.column("changed_bonds").tolist() == [int(np.count_nonzero(np.tril(l, -1))) for l in labels]


def test_valence_limits():
    """Atom 2 (label 6) carries a double and a single bond: valence2 = 6.  Over the limit at 5, exactly at it at 6, and without a
    limit at 0xFFFF; a label past the table has none either."""
    N = 5
    atoms = np.array([[1, 1, 6, 0, 0]] * 2)
    labels = np.zeros((2, N, N), dtype=np.int64)
    labels[:, 2, 0], labels[:, 2, 1] = 2, 1
    for limit, over in ((5, 1), (6, 0), (7, 0), (0xFFFF, 0), (0, 1)):
        table = [0xFFFF, 8, 8, 8, 8, 8, limit]
        got = _check(atoms, labels, 13, 5, max_valence2=table)
        assert got.column("over_valent").tolist() == [over, over] and got.total("n_over_valent") == 2 * over, limit
        assert got.over_valent_fraction == float(over)
    got = _check(atoms, labels, 13, 5, max_valence2=[0xFFFF, 3])      # label 1: atom 0 (double bond, 4) is over, atom 1 (2) is not
    assert got.column("over_valent").tolist() == [1, 1]
    got = _check(atoms, labels, 13, 5)                                # no table: the column is not answered
    assert (got.column("over_valent") == -1).all() and got.total("over_valent") == 0
    # a batch decoded without bond orders has no valence2 either
    from druggen_amd import decode, monitor
    node, edge = dref.one_hot_logits(atoms, labels, 13, 5)
    plain = decode.decode_molecule_graphs(torch.from_numpy(node).cuda(), torch.from_numpy(edge).cuda())
    assert (monitor.molecule_statistics(plain, max_valence2=[0xFFFF] * 13).cpu().column("over_valent") == -1).all()


def test_result_does_not_depend_on_the_key_width():
    """At 1 bit about every second pair is a key match, so the byte comparison carries the result."""
    rng = np.random.default_rng(17)
    B, N = 65, 9
    pool_atoms, pool_labels = _random_graphs(rng, 6, N, 3, 3, density=0.2)
    pick = rng.integers(0, 6, B)
    atoms, labels = pool_atoms[pick].copy(), pool_labels[pick].copy()
    for b in range(0, B, 5):                   # near misses of the pool: one atom or one label away
        if b % 2:
            atoms[b, b % N] = (atoms[b, b % N] + 1) % 3
        else:
            labels[b, 4, 2] = labels[b, 2, 4] = (labels[b, 4, 2] + 1) % 3
    results = [_check(atoms, labels, 3, 3, in_atoms=pool_atoms[pick], in_labels=pool_labels[pick], key_bits=bits)
               for bits in (1, 2, 64)]
    assert all(np.array_equal(r.buffer, results[0].buffer) for r in results[1:])
    assert results[0].total("n_distinct") <= 6 + 13      # the pool and the near misses
    from druggen_amd import monitor
    for bad in (0, 65, -1, 1.5, None,
                True):                         # (a bool is no width: canon's check, shared)
        with pytest.raises(ValueError, match="key_bits"):
            monitor.molecule_statistics(_decode(atoms[:2], labels[:2], 3, 3), key_bits=bad)


def test_truncated_molecules():
    atoms, labels = _random_graphs(np.random.default_rng(23), 7, 9, 13, 5, density=0.3)
    labels[1] = 0                                                  # no bond
    labels[2] = 0
    labels[2, 5, 3] = labels[2, 3, 5] = 2                          # one bond: fits a list of one row
    atoms[4], labels[4] = atoms[1], labels[1]                      # duplicates among the molecules that fit
    atoms[6], labels[6] = atoms[0], labels[0]                      # ... and among the truncated ones: not reported
    got = _check(atoms, labels, 13, 5, cap=1, in_atoms=atoms, in_labels=labels)
    assert got.column("duplicate_of").tolist() == [-2, -1, -1, -2, 1, -2, -2]
    assert got.column("changed_bonds").tolist() == [-1, 0, 0, -1, 0, -1, -1]
    assert got.total("n_truncated") == 4 and got.total("n_distinct") == 2 and got.total("n_copies") == 3
    got = _check(atoms, labels, 13, 5, cap=0)
    assert got.column("duplicate_of").tolist() == [-2, -1, -2, -2, 1, -2, -2] and got.total("n_truncated") == 5


def test_two_launches_are_bit_identical_and_no_output_is_stale():
    from druggen_amd import monitor
    rng = np.random.default_rng(31)
    atoms, labels = _random_graphs(rng, 65, 45, 13, 5)
    atoms[40], labels[40] = atoms[3], labels[3]
    batch = _decode(atoms, labels, 13, 5)
    in_atoms, in_labels = _dev(atoms, torch.uint8), _dev(np.roll(labels, 1, 0), torch.int32)
    table = [0xFFFF] + [6] * 12
    outs = []
    for fill in (0x00, 0xFF, 0xFF):
        out = monitor.MolStats.empty(65, 45, "cuda")
        out.buffer.fill_(fill)
        out._workspace.fill_(-1 if fill else 0)
        got = monitor.molecule_statistics(batch, in_atoms=in_atoms, in_labels=in_labels, max_valence2=table, out=out)
        assert got is out
        outs.append(out.cpu())
    assert np.array_equal(outs[0].buffer, outs[1].buffer) and np.array_equal(outs[1].buffer, outs[2].buffer)
    mol, tot = _want(atoms, labels, 5, in_atoms=atoms, in_labels=np.roll(labels, 1, 0), max_valence2=table)
    assert np.array_equal(outs[0].mol, mol) and np.array_equal(outs[0].tot, tot)
    # an empty batch writes its totals too
    empty = monitor.MolStats.empty(0, 45, "cuda")
    empty.buffer.fill_(0xFF)
    from druggen_amd.decode import MoleculeBatch
    assert monitor.molecule_statistics(MoleculeBatch.empty(0, 45, 990, True, "cuda"), out=empty).cpu().tot.tolist() == [0] * 16
    with pytest.raises(ValueError, match="out="):
        monitor.molecule_statistics(batch, out=monitor.MolStats.empty(64, 45, "cuda"))
    with pytest.raises(ValueError, match="in_labels"):
        monitor.molecule_statistics(batch, in_labels=in_labels[:, :44])
    with pytest.raises(ValueError, match="in_atoms"):
        monitor.molecule_statistics(batch, in_atoms=in_atoms.to(torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monitor.molecule_statistics(batch, in_atoms=in_atoms.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monitor.molecule_statistics(batch.cpu())


def test_decode_and_statistics_replay_from_a_captured_graph():
    """Both calls captured into one hipGraph, replayed on new logits and new input labels: the eager results."""
    from druggen_amd import decode, monitor
    rng = np.random.default_rng(41)
    B, N, M, E = 5, 9, 13, 5
    table = [0xFFFF] + [5] * 12
    sets = []
    for k in range(3):
        atoms, labels = _random_graphs(rng, B, N, M, E, density=0.3)
        atoms[B - 1], labels[B - 1] = atoms[k], labels[k]
        in_atoms, in_labels = atoms.copy(), labels.copy()
        in_atoms[k, 0] = (in_atoms[k, 0] + 1) % M
        in_labels[k + 1, 2, 1] = (in_labels[k + 1, 2, 1] + 1) % E
        sets.append((atoms, labels, in_atoms, in_labels))
    node, edge = (torch.from_numpy(4.0 * t).cuda() for t in dref.one_hot_logits(sets[0][0], sets[0][1], M, E))
    in_a, in_l = _dev(sets[0][2], torch.uint8), _dev(sets[0][3], torch.int32)
    decoded = decode.MoleculeBatch.empty(B, N, N * (N - 1) // 2, True, "cuda")
    stats = monitor.MolStats.empty(B, N, "cuda")

    def both():
        decode.decode_molecule_graphs(node, edge, bond_order2=_order2(E), out=decoded)
        monitor.molecule_statistics(decoded, in_atoms=in_a, in_labels=in_l, max_valence2=table, out=stats)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()      # warm-up: the two small tables are uploaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    seen = []
    for atoms, labels, in_atoms, in_labels in sets[1:] + sets[:1]:
        n, e = dref.one_hot_logits(atoms, labels, M, E)
        node.copy_(torch.from_numpy(4.0 * n))
        edge.copy_(torch.from_numpy(4.0 * e))
        in_a.copy_(torch.from_numpy(in_atoms).to(torch.uint8))
        in_l.copy_(torch.from_numpy(in_labels).to(torch.int32))
        stats.buffer.fill_(0xFF)
        graph.replay()
        got = stats.cpu()
        mol, tot = _want(atoms, labels, E, in_atoms=in_atoms, in_labels=in_labels, max_valence2=table)
        assert np.array_equal(got.mol, mol) and np.array_equal(got.tot, tot)
        eager = _stats(_decode(atoms, labels, M, E), in_atoms, in_labels, table).cpu()
        assert np.array_equal(eager.buffer, got.buffer)
        seen.append(got.mol.copy())
    assert not np.array_equal(seen[0], seen[1])
