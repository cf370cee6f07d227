"""Host side of the molecule statistics (csrc/mol_stats.hip, druggen_amd/monitor.py): their rows of the ctypes table, every
argument refusal -- all of which return before a launch -- and the numpy restatement (tests/mol_stats_ref.py) on hand-written
molecules.  No GPU.  tests/test_host.py holds the table against include/druggen_hip.h."""
import ctypes

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_stats_ref as ref

SHAPE, ARG, WORKSPACE = -1, -2, -3      # DG_E_SHAPE, DG_E_ARG, DG_E_WORKSPACE of include/druggen_hip.h
ENTRIES = {"dg_mol_stats_workspace_bytes", "dg_mol_stats"}


def test_entries_are_in_the_ctypes_table():
    from druggen_amd import _lib
    assert ENTRIES <= set(_lib.SIGNATURES)


@pytest.fixture(scope="module")
def lib():
    from druggen_amd import _lib
    return _lib.load()


_buf = (ctypes.c_int64 * 8)()
P = ctypes.addressof(_buf)      # a non-null, 16-byte aligned pointer: no call below gets as far as reading it
assert P % 8 == 0


def _err(lib):
    return lib.dg_last_error_string()


def test_workspace_bytes(lib):
    size = lib.dg_mol_stats_workspace_bytes
    assert size(0) == 0 and size(-3) == 0
    assert size(1) == 8 and size(2048) == 8 * 2048      # one 64-bit key per molecule


def test_argument_checks(lib):
    """Every refusal; none of these calls launches (the last check, the workspace size, fails in each call that gets that far)."""
    base = P - P % 16 + 16 if P % 16 else P

    def stats(atoms=P, bonds=P, n_bonds=P, n_components=P, largest_size=P, valence2=None, in_atoms=None, in_labels=None,
              max_valence2=None, B=3, N=9, cap=36, M=0, key_bits=64, mol=base, tot=P, workspace=P, workspace_bytes=0):
        return lib.dg_mol_stats(atoms, bonds, n_bonds, n_components, largest_size, valence2, in_atoms, in_labels, max_valence2,
                                B, N, cap, M, key_bits, mol, tot, workspace, workspace_bytes, None)
    for kw in (dict(B=-1), dict(N=0), dict(N=257), dict(N=-4), dict(cap=-1)):
        assert stats(**kw) == SHAPE and b"dg_mol_stats: need B >= 0, 1 <= N <= 256" in _err(lib), kw
    for M in (0, -1, 257):
        assert stats(max_valence2=P, M=M) == SHAPE and b"max_valence2 holds 1..256 entries" in _err(lib), M
    for bits in (0, -1, 65, 128):
        assert stats(key_bits=bits) == ARG and b"key_bits must be in 1..64" in _err(lib), bits
    for name in ("atoms", "n_bonds", "n_components", "largest_size", "mol", "tot", "workspace"):
        assert stats(**{name: None}) == ARG and b"dg_mol_stats: null pointer" in _err(lib), name
    assert stats(tot=None, B=0) == ARG      # an empty batch still writes tot
    assert stats(bonds=None) == ARG and b"bonds with cap > 0" in _err(lib)
    for kw in (dict(bonds=P + 2), dict(mol=base + 4), dict(tot=P + 4), dict(workspace=P + 4)):
        assert stats(**kw) == ARG and b"aligned" in _err(lib), kw
    # the shape comes first, then key_bits, then the pointers
    assert stats(N=257, key_bits=0, atoms=None) == SHAPE and stats(key_bits=0, atoms=None) == ARG and b"key_bits" in _err(lib)
    # everything else in order: only the workspace is too small (3 molecules need 24 bytes)
    for kw in (dict(), dict(bonds=None, cap=0), dict(key_bits=1), dict(max_valence2=P, M=256, valence2=P),
               dict(in_atoms=P, in_labels=P), dict(N=1, cap=0), dict(N=256, cap=32640), dict(workspace_bytes=23)):
        assert stats(**kw) == WORKSPACE and b"need 24" in _err(lib), kw


def test_python_refusals_without_a_gpu():
    """`molecule_statistics` refuses host batches and CPU tensors like the other modules do; `MolStats` fractions read the host."""
    from druggen_amd import monitor
    from druggen_amd.decode import MoleculeBatch, _layout
    _, total = _layout(2, 3, 3, False)
    host = MoleculeBatch(np.zeros(total, dtype=np.uint8), 2, 3, 3, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monitor.molecule_statistics(host)
    with pytest.raises(TypeError):
        monitor.molecule_statistics(np.zeros(4))
    assert monitor.MOL_COLUMNS == ref.COLUMNS and len(monitor.TOT_FIELDS) == 13


# ---- the restatement on hand-written molecules -----------------------------------------------------------------------
ORDER2 = [0, 2, 4, 6, 3]


def _triangle(N=4, atom=6, label=1):
    """Atoms 0, 1, 2 bonded in a ring; the rest is padding (label 0)."""
    atoms = np.array([atom] * 3 + [0] * (N - 3))
    labels = np.zeros((N, N), dtype=np.int64)
    labels[1, 0] = labels[2, 0] = labels[2, 1] = label
    return atoms, labels


def test_restatement_on_a_triangle_its_copies_and_a_pad_only_molecule():
    N = 4
    tri_atoms, tri_labels = _triangle(N)
    pad_atoms, pad_labels = np.zeros(N, dtype=np.int64), np.zeros((N, N), dtype=np.int64)
    double = tri_labels.copy()
    double[2, 1] = 2      # one bond label differs: not a copy
    graphs = [(tri_atoms, tri_labels), (pad_atoms, pad_labels), (tri_atoms, tri_labels), (tri_atoms, double),
              (tri_atoms, tri_labels), (pad_atoms, pad_labels)]
    mols = [dref.decode_labels(a, l, ORDER2) for a, l in graphs]
    in_atoms = np.stack([tri_atoms] * 6)
    in_labels = np.stack([tri_labels + tri_labels.T] * 6)      # symmetric, as the dataset's: only i > j is read
    max_valence2 = [0xFFFF, 8, 8, 8, 8, 8, 4]                  # label 6: valence 2 -> exactly reached by two single bonds
    mol, tot = ref.mol_stats(mols, in_atoms=in_atoms, in_labels=in_labels, max_valence2=max_valence2)
    # atom_types: {6, 0} = 2 (the pad label counts), pad only = 1
    assert mol[:, 0].tolist() == [2, 1, 2, 2, 2, 1]
    assert mol[:, 1].tolist() == [3, 1, 3, 3, 3, 1]            # largest fragment
    assert mol[:, 2].tolist() == [2, 4, 2, 2, 2, 4]            # the ring and one pad atom; four pad atoms
    assert mol[:, 3].tolist() == [3, 0, 3, 3, 3, 0]
    assert mol[:, 4].tolist() == [0, 0, 0, 2, 0, 0]            # the double bond lifts atoms 1 and 2 to valence 3 > 2
    assert mol[:, 5].tolist() == [0, 3, 0, 0, 0, 3]
    assert mol[:, 6].tolist() == [0, 3, 0, 1, 0, 3]
    assert mol[:, 7].tolist() == [-1, -1, 0, -1, 0, 1]         # all later copies point to the FIRST
    assert tot.tolist() == [6, 10, 14, 16, 12, 2, 6, 7, 1, 3, 3, 0, 0, 0, 0, 0]
    # the host-side fractions of `MolStats` and `fractions_of` read exactly these totals
    from druggen_amd import monitor
    stats = monitor.MolStats(np.concatenate([tot.view(np.uint8), mol.reshape(-1).view(np.uint8)]), 6, N)
    assert stats.is_host and stats.cpu() is stats and np.array_equal(stats.mol, mol) and np.array_equal(stats.tot, tot)
    assert stats.column("duplicate_of").tolist() == mol[:, 7].tolist() and stats.total("n_copies") == 3
    assert stats.atom_types_mean == 10 / 6 - 1                 # the reference's Atom_types: mean of the counts, minus one
    assert stats.main_fragment_fraction == 14 / 6 / N and stats.distinct_fraction == 0.5
    assert stats.copy_fraction == 0.5 and stats.over_valent_fraction == 1 / 6
    assert monitor.fractions_of(tot, N) == {
        "atom_types_mean": 10 / 6 - 1, "main_fragment_fraction": 14 / (6 * N), "distinct_fraction": 0.5, "copy_fraction": 0.5,
        "over_valent_fraction": 1 / 6}
    # without the optional inputs the columns are -1 and are not summed
    mol, tot = ref.mol_stats(mols)
    assert (mol[:, 4:7] == -1).all() and tot[5:10].tolist() == [0, 0, 0, 0, 0] and tot[10] == 3
    # truncated at one row: nothing with bonds is compared, the pad-only molecules still are
    mol, tot = ref.mol_stats(mols, cap=1, in_atoms=in_atoms, in_labels=in_labels)
    assert mol[:, 6].tolist() == [-1, 3, -1, -1, -1, 3] and mol[:, 7].tolist() == [-2, -1, -2, -2, -2, 1]
    assert tot[11] == 4 and tot[10] == 1 and tot[9] == 0 and tot[7] == 6
    assert ref.atom_types([5, 5, 0, 3, 0]) == 3


def test_molecules_of_round_trips_a_host_batch():
    from druggen_amd.decode import MoleculeBatch, _layout
    N, cap = 4, 6
    _, total = _layout(2, N, cap, True)
    host = MoleculeBatch(np.zeros(total, dtype=np.uint8), 2, N, cap, True)
    atoms, labels = _triangle(N)
    want = dref.decode_labels(atoms, labels, ORDER2)
    host.atoms[0], host.n_bonds[0], host.n_components[0], host.largest_size[0] = atoms, 3, 2, 3
    host.bonds[0, :3, :3] = want["bonds"]
    host.valence2[0] = want["valence2"]
    host.n_components[1], host.largest_size[1] = 4, 1
    mols = ref.molecules_of(host)
    mol, _ = ref.mol_stats(mols)
    expect, _ = ref.mol_stats([want, dref.decode_labels(np.zeros(N, dtype=np.int64), np.zeros((N, N), dtype=np.int64), ORDER2)])
    assert np.array_equal(mol, expect)
