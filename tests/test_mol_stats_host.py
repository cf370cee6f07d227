"""Host side of the molecule statistics (include/druggen_hip_mol_stats.h, csrc/mol_stats.hip, druggen_amd/monitor.py): the add-on
header against its ctypes table, the exports, every argument refusal -- all of which return before a launch -- and the numpy
restatement (tests/mol_stats_ref.py) on hand-written molecules.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG, WORKSPACE = -1, -2, -3      # DG_E_SHAPE, DG_E_ARG, DG_E_WORKSPACE of include/druggen_hip.h
ENTRIES = {"dg_mol_stats_workspace_bytes", "dg_mol_stats"}


def test_ctypes_table_matches_the_add_on_header():
    """Parameter by parameter, as tests/test_row_gemm_any_host.py does for its header; disjoint from the other tables; exported
    by the library."""
    from druggen_amd import _lib
    header = open(os.path.join(ROOT, "include", "druggen_hip_mol_stats.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", " ", header, flags=re.M)
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header)
    assert len(protos) == len(ENTRIES)
    assert {name for _, name, _ in protos} == set(_lib.MOL_STATS_SIGNATURES) == ENTRIES
    for other in (_lib.SIGNATURES, _lib.EMBED_KEEP_SIGNATURES, _lib.EMBED_SMOOTH_SIGNATURES, _lib.MOL_FEATURES_SIGNATURES,
                  _lib.NODE_WIDE_SIGNATURES, _lib.ROW_GEMM_ANY_SIGNATURES):
        assert not set(_lib.MOL_STATS_SIGNATURES) & set(other)

    def kind(decl):
        decl = re.sub(r"\bconst\b", " ", decl).strip()
        if "*" in decl or re.match(r"dg_stream_t\b", decl):
            return "pointer"
        return decl.split()[0]

    named = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_void_p: "pointer", ctypes.c_size_t: "size_t"}
    lib = _lib.load()
    for ret, name, params in protos:
        res, args = _lib.MOL_STATS_SIGNATURES[name]
        assert [kind(ret)] + [kind(p) for p in params.split(",")] == [named[res]] + [named[a] for a in args], name
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res


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
