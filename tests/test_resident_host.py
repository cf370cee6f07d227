"""Host side of the GPU-resident molecule set (druggen_amd/resident.py): the compact form `ResidentMolecules.pack` builds,
checked literally on hand-written molecules and against a numpy scatter on real ones; its refusals; the whole-dataset
split of `from_batch`; the slicing of `epoch`.  No GPU."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
from druggen_amd import smiles as sm
from druggen_amd.resident import ResidentMolecules, epoch_batches


def _mol(atom_labels, edges, m_dim=4):
    """edges: (row, col, label) as given (directed)."""
    x = np.zeros((len(atom_labels), m_dim), dtype=np.float32)
    x[np.arange(len(atom_labels)), atom_labels] = 1.0
    e = np.array(edges, dtype=np.int64).reshape(-1, 3)
    return SimpleNamespace(x=x, edge_index=e[:, :2].T.copy(), edge_attr=e[:, 2].copy())


def _word(row, col, label):
    return row | col << 8 | label << 16


def _dense_from_words(words, N):
    dense = np.zeros((N, N), dtype=np.int64)
    assert len(set((int(w) & 0xFFFF) for w in words)) == len(words), "(row, col) pairs must be unique"
    for w in words:
        w = int(w)
        assert w >> 24 == 0
        dense[w & 255, (w >> 8) & 255] = w >> 16
    return dense


def _dense_from_coo(g, N):
    dense = np.zeros((N, N), dtype=np.int64)
    np.add.at(dense, (np.asarray(g.edge_index[0]), np.asarray(g.edge_index[1])), np.asarray(g.edge_attr))
    return dense


def test_pack_hand_written_molecules_literally():
    chain = _mol([1, 2, 1], [(0, 1, 1), (1, 0, 1), (1, 2, 2), (2, 1, 2)])
    lonely = _mol([3, 0, 0], [])
    duplicate = _mol([1, 1, 0], [(0, 1, 1), (0, 1, 2), (1, 0, 3)])      # 1 + 2 -> 3 at (0, 1)
    one_way = _mol([2, 2, 2], [(2, 0, 1)])                              # asymmetric: kept as given
    atoms, ptr, entries = ResidentMolecules.pack([chain, lonely, duplicate, one_way], b_dim=4)
    assert atoms.dtype == np.uint8 and ptr.dtype == np.int64 and entries.dtype == np.uint32
    assert atoms.tolist() == [[1, 2, 1], [3, 0, 0], [1, 1, 0], [2, 2, 2]]
    assert ptr.tolist() == [0, 4, 4, 6, 7]
    assert entries.tolist() == [_word(0, 1, 1), _word(1, 0, 1), _word(1, 2, 2), _word(2, 1, 2),      # row-major per molecule
                                _word(0, 1, 3), _word(1, 0, 3),
                                _word(2, 0, 1)]
    assert entries.tolist()[:2] == [65792, 65537]
    # a duplicate pair that sums past b_dim is refused, and one that sums to zero is dropped
    with pytest.raises(ValueError, match=r"molecule 1.*label 4 outside \[0, 4\)"):
        ResidentMolecules.pack([chain, _mol([1, 1, 0], [(0, 1, 2), (0, 1, 2)])], b_dim=4)
    _, ptr0, entries0 = ResidentMolecules.pack([_mol([1, 1, 0], [(0, 1, 2), (0, 1, -2), (1, 0, 1)])], b_dim=4)
    assert ptr0.tolist() == [0, 1] and entries0.tolist() == [_word(1, 0, 1)]
    # CPU tensors are taken like numpy arrays
    as_tensors = SimpleNamespace(x=torch.from_numpy(chain.x), edge_index=torch.from_numpy(chain.edge_index),
                                 edge_attr=torch.from_numpy(chain.edge_attr))
    for got, want in zip(ResidentMolecules.pack([as_tensors]), ResidentMolecules.pack([chain])):
        assert np.array_equal(got, want)


def _smiles_graphs(count=6):
    rows = [ln.strip().split(",") for ln in open(os.path.join(os.path.dirname(cases.__file__), "chembl_like_smiles.csv"))
            if ln.strip() and not ln.startswith("#")][1:]
    strings = [r[2] for r in rows][:count]
    atom_enc, _, bond_enc, _, kept, _ = sm.build_encoders(strings, 45)
    graphs = [sm.molecule_graph(s, atom_enc, bond_enc, 45) for s in kept]
    assert len(graphs) >= 4 and all(g is not None for g in graphs)
    return graphs, len(atom_enc), len(bond_enc)


def test_pack_real_molecules_rebuilds_the_scattered_matrices():
    graphs, m_dim, b_dim = _smiles_graphs()
    atoms, ptr, entries = ResidentMolecules.pack(graphs, m_dim=m_dim, b_dim=b_dim)
    assert atoms.shape == (len(graphs), 45) and ptr[-1] == len(entries) == sum(g.edge_attr.size for g in graphs)
    for i, g in enumerate(graphs):
        assert np.array_equal(_dense_from_words(entries[ptr[i]:ptr[i + 1]], 45), _dense_from_coo(g, 45))
        assert np.array_equal(atoms[i], g.x.argmax(1))
        assert (atoms[i, g.num_atoms:] == 0).all()      # PAD = 0


def test_pack_refusals_name_the_molecule():
    good = _mol([1, 2, 1], [(0, 1, 1), (1, 0, 1)])
    soft = _mol([1, 2, 1], [])
    soft.x[1] = [0.5, 0.5, 0, 0]
    two_hot = _mol([1, 2, 1], [])
    two_hot.x[2, 3] = 1.0
    empty_row = _mol([1, 2, 1], [])
    empty_row.x[0] = 0
    for bad in (soft, two_hot, empty_row):
        with pytest.raises(ValueError, match=r"molecule 1: x is not one-hot.*--features"):
            ResidentMolecules.pack([good, bad])
    with pytest.raises(ValueError, match=r"molecule 2: node id outside \[0, 3\)"):
        ResidentMolecules.pack([good, good, _mol([1, 2, 1], [(0, 3, 1)])])
    with pytest.raises(ValueError, match=r"molecule 0: node id outside"):
        ResidentMolecules.pack([_mol([1, 2, 1], [(-1, 0, 1)])])
    with pytest.raises(ValueError, match=r"molecule 1: 4 atom positions, molecule 0 has 3"):
        ResidentMolecules.pack([good, _mol([1, 2, 1, 0], [])])
    with pytest.raises(ValueError, match=r"molecule 1.*label 5 outside \[0, 5\)"):
        ResidentMolecules.pack([good, _mol([1, 2, 1], [(0, 1, 5)])], b_dim=5)
    with pytest.raises(ValueError, match=r"molecule 0.*label -1 outside"):
        ResidentMolecules.pack([_mol([1, 2, 1], [(0, 1, -1)])])
    with pytest.raises(ValueError, match=r"molecule 0.*N = 257.*256"):
        ResidentMolecules.pack([_mol([0] * 257, [])])
    with pytest.raises(ValueError, match=r"b_dim = 17.*16"):
        ResidentMolecules.pack([good], b_dim=17)
    with pytest.raises(ValueError, match=r"m_dim = 256.*255"):
        ResidentMolecules.pack([_mol([1, 2, 1], [], m_dim=256)])
    with pytest.raises(ValueError, match="no molecules"):
        ResidentMolecules.pack([])
    ResidentMolecules.pack([_mol([0] * 256, [(255, 254, 15)], m_dim=255)], b_dim=16)      # the limits themselves are fine


def test_from_batch_split_equals_per_graph_pack_with_a_cross_graph_edge():
    graphs, m_dim, b_dim = _smiles_graphs(4)
    batch = sm.collate(graphs)
    split = ResidentMolecules.split_batch(batch, len(graphs))
    for got, want in zip(ResidentMolecules.pack(split, m_dim=m_dim, b_dim=b_dim),
                         ResidentMolecules.pack(graphs, m_dim=m_dim, b_dim=b_dim)):
        assert np.array_equal(got, want)
    # one hand-made edge from graph 1 (node 3) into graph 2 (node 7): it lands in graph 1 at (3, 7)
    assert _dense_from_coo(graphs[1], 45)[3, 7] == 0
    crossed = sm.GraphBatch(batch.x, torch.cat([batch.edge_index, torch.tensor([[45 + 3], [90 + 7]])], 1),
                            torch.cat([batch.edge_attr, torch.tensor([2])]), batch.batch)
    atoms, ptr, entries = ResidentMolecules.pack(ResidentMolecules.split_batch(crossed, len(graphs)), m_dim=m_dim, b_dim=b_dim)
    for i, g in enumerate(graphs):
        want = _dense_from_coo(g, 45)
        if i == 1:
            want[3, 7] = 2
        assert np.array_equal(_dense_from_words(entries[ptr[i]:ptr[i + 1]], 45), want)
    with pytest.raises(ValueError, match="node id outside"):
        ResidentMolecules.split_batch(sm.GraphBatch(batch.x, torch.tensor([[0], [4 * 45]]), torch.tensor([1]), batch.batch), 4)


def test_epoch_slicing():
    order = torch.arange(10)
    assert [b.tolist() for b in epoch_batches(order, 4, drop_last=True)] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert [b.tolist() for b in epoch_batches(order, 4, drop_last=False)] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert [b.tolist() for b in epoch_batches(order, 5, drop_last=True)] == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]
    assert list(epoch_batches(order, 11, drop_last=True)) == []
    perm = torch.tensor([3, 1, 4, 0, 2])
    assert [b.tolist() for b in epoch_batches(perm, 2, drop_last=False)] == [[3, 1], [4, 0], [2]]
    with pytest.raises(ValueError):
        list(epoch_batches(order, 0))
    # the method on a stub store: it needs `n` and a device only
    stub = SimpleNamespace(n=10, device=torch.device("cpu"))
    assert [b.tolist() for b in ResidentMolecules.epoch(stub, 4, shuffle=False)] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert [b.tolist() for b in ResidentMolecules.epoch(stub, 4, shuffle=False, drop_last=False)][-1] == [8, 9]
    shuffled = torch.cat(list(ResidentMolecules.epoch(stub, 3, drop_last=False, generator=torch.Generator().manual_seed(5))))
    assert shuffled.dtype == torch.int64 and sorted(shuffled.tolist()) == list(range(10))


def test_a_cpu_store_is_refused():
    atoms, ptr, entries = ResidentMolecules.pack([_mol([1, 2, 1], [(0, 1, 1)])])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ResidentMolecules.from_arrays(atoms, ptr, entries, 4, 2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ResidentMolecules.from_graphs([_mol([1, 2, 1], [(0, 1, 1)])], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ResidentMolecules(torch.from_numpy(atoms), torch.from_numpy(ptr), torch.from_numpy(entries.view(np.int32)), 4, 2)


def test_c_abi_argument_checks_need_no_gpu():
    import ctypes
    from druggen_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(buf)

    def call(N=9, M=5, E=5, B=2, x=p):
        return lib.dg_mol_gather(p, p, p, 3, p, B, N, M, E, p, p, x, p, None)
    for kw in (dict(N=257), dict(N=0), dict(E=17), dict(E=0), dict(M=256), dict(M=0), dict(B=-1)):
        assert call(**kw) == -1, kw
        assert b"1 <= N <= 256, 1 <= M <= 255, 1 <= E <= 16" in lib.dg_last_error_string()
    assert call(x=None) == -2 and b"dg_mol_gather: null pointer" in lib.dg_last_error_string()
    assert lib.dg_mol_gather(None, None, None, 0, None, 0, 9, 5, 5, None, None, None, None, None) == 0      # B == 0: nothing to do
