"""Host side of the feature plane of the GPU-resident molecule set (druggen_amd/resident.py, `pack_features`): node matrices
that are a one-hot atom type followed by F columns of 0 / 1 (the reference's --features) are split at `atom_dim` into today's
`atoms` byte and a bit plane, and a numpy unpack written here gives every `x` back exactly; the refusals; the default `pack`
as it was; the ctypes row of `dg_mol_gather_features` against `dg_mol_gather`'s, and its argument checks.  No GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from druggen_amd.resident import ResidentMolecules

BLOCKS = (5, 9, 6, 9, 1, 1, 5, 5, 5, 1, 7)      # the reference's descriptor blocks (dataset.py:161-185): 54 columns
N, ATOM_DIM, N_MOL = 6, 9, 5


def _features(rng, rows, F):
    """[rows, F] of 0 / 1.  F = 54: the reference's block layout, one-hot inside each multi-column block, a coin per
    single-column block.  Other widths: coins, with the first and the last column set in row 0 and the last row all ones."""
    if F == sum(BLOCKS):
        parts = []
        for width in BLOCKS:
            block = np.zeros((rows, width), dtype=np.float32)
            if width == 1:
                block[:, 0] = rng.integers(0, 2, size=rows)
            else:
                block[np.arange(rows), rng.integers(0, width, size=rows)] = 1.0
            parts.append(block)
        return np.concatenate(parts, 1)
    feats = rng.integers(0, 2, size=(rows, F)).astype(np.float32)
    feats[0, 0] = feats[0, -1] = 1.0
    feats[-1] = 1.0
    return feats


def _graphs(F, n=N_MOL, atom_dim=ATOM_DIM, seed=0):
    rng = np.random.default_rng([F, n, atom_dim, seed])
    graphs = []
    for i in range(n):
        x = np.zeros((N, atom_dim + F), dtype=np.float32)
        x[np.arange(N), rng.integers(0, atom_dim, size=N)] = 1.0
        x[:, atom_dim:] = _features(rng, N, F)
        upper = np.triu((rng.random((N, N)) < 0.4) * rng.integers(1, 5, size=(N, N)), 1)
        src, dst = np.nonzero(upper + upper.T)
        graphs.append(SimpleNamespace(x=x, edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=(upper + upper.T)[src, dst]))
    return graphs


def _unpack(atoms, bits, atom_dim, F):
    """x [n, N, atom_dim + F] float32 from the compact form: feature f is bit f % 32 of word f // 32."""
    x = np.zeros(atoms.shape + (atom_dim + F,), dtype=np.float32)
    np.put_along_axis(x, atoms[..., None].astype(np.int64), 1.0, axis=-1)
    for f in range(F):
        x[..., atom_dim + f] = (bits[..., f // 32] >> np.uint32(f % 32)) & np.uint32(1)
    return x


@pytest.mark.parametrize("F", [1, 31, 32, 33, 54, 64, 65, 246])
def test_pack_features_then_unpack_is_exact(F):
    graphs = _graphs(F)
    atoms, ptr, entries, bits = ResidentMolecules.pack_features(graphs, ATOM_DIM, b_dim=5)
    W = (F + 31) // 32
    assert atoms.dtype == np.uint8 and ptr.dtype == np.int64 and entries.dtype == np.uint32 and bits.dtype == np.uint32
    assert atoms.shape == (N_MOL, N) and bits.shape == (N_MOL, N, W)
    assert np.array_equal(_unpack(atoms, bits, ATOM_DIM, F), np.stack([g.x for g in graphs]))
    assert bits.any() and (bits[..., -1] >> np.uint32((F - 1) % 32) & np.uint32(1)).any()      # the top feature is in use
    if F % 32:
        assert not (bits[..., -1] >> np.uint32(F % 32)).any()      # unused high bits of the last word
    cut = [SimpleNamespace(x=g.x[:, :ATOM_DIM], edge_index=g.edge_index, edge_attr=g.edge_attr) for g in graphs]
    for got, want in zip((atoms, ptr, entries), ResidentMolecules.pack(cut, b_dim=5)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    # the widths may be stated, and atom_dim == m_dim is a plane without a column
    for got, want in zip(ResidentMolecules.pack_features(graphs, ATOM_DIM, m_dim=ATOM_DIM + F, b_dim=5), (atoms, ptr, entries, bits)):
        assert np.array_equal(got, want)
    assert ResidentMolecules.pack_features(cut, ATOM_DIM, b_dim=5)[3].shape == (N_MOL, N, 0)


def test_the_reference_layout_is_one_hot_inside_each_block():
    """(of the test's own F = 54 input: what the case above packs is the layout it claims to be)"""
    x = np.stack([g.x for g in _graphs(54)])[..., ATOM_DIM:]
    assert x.shape[-1] == 54
    start = 0
    for width in BLOCKS:
        if width > 1:
            assert (x[..., start:start + width].sum(-1) == 1).all()
        start += width


def test_pack_features_refusals_name_the_molecule():
    def bad(edit):
        g = _graphs(54, n=1, seed=1)[0]
        edit(g.x)
        return g
    good = _graphs(54, n=2)

    def two(x):
        x[3, ATOM_DIM + 7] = 2.0

    def half(x):
        x[0, ATOM_DIM + 53] = 0.5

    def two_hot(x):
        x[2, :ATOM_DIM] = 0
        x[2, [1, 4]] = 1.0

    def empty_row(x):
        x[5, :ATOM_DIM] = 0
    for edit in (two, half):
        with pytest.raises(ValueError, match=r"molecule 2: a feature column.*other than 0 or 1"):
            ResidentMolecules.pack_features(good + [bad(edit)], ATOM_DIM)
    for edit in (two_hot, empty_row):
        with pytest.raises(ValueError, match=r"molecule 2: the first atom_dim = 9 columns of x are not one-hot"):
            ResidentMolecules.pack_features(good + [bad(edit)], ATOM_DIM)
    with pytest.raises(ValueError, match=r"molecule 0: atom_dim = 0 outside \[1, m_dim = 63\]"):
        ResidentMolecules.pack_features(good, 0)
    with pytest.raises(ValueError, match=r"molecule 0: atom_dim = 64 outside \[1, m_dim = 63\]"):
        ResidentMolecules.pack_features(good, 64)
    with pytest.raises(ValueError, match=r"molecule 2: x has 42 columns, m_dim is 63"):
        ResidentMolecules.pack_features(good + _graphs(33, n=1), ATOM_DIM)
    with pytest.raises(ValueError, match=r"molecule 0.*m_dim = 256.*255"):
        ResidentMolecules.pack_features(_graphs(247, n=1), ATOM_DIM)
    # the bond part is pack's: its refusals come through unchanged
    broken = _graphs(54, n=1)[0]
    broken.edge_index = np.array([[0], [N]])
    broken.edge_attr = np.array([1])
    with pytest.raises(ValueError, match=rf"molecule 2: node id outside \[0, {N}\)"):
        ResidentMolecules.pack_features(good + [broken], ATOM_DIM)


def test_default_pack_still_refuses_feature_matrices():
    """The three refusals of tests/test_resident_host.py::test_pack_refusals_name_the_molecule, and a --features matrix
    itself: the default call did not change."""
    def mol(labels, m_dim=4):
        x = np.zeros((len(labels), m_dim), dtype=np.float32)
        x[np.arange(len(labels)), labels] = 1.0
        return SimpleNamespace(x=x, edge_index=np.zeros((2, 0), dtype=np.int64), edge_attr=np.zeros(0, dtype=np.int64))
    good, soft, two_hot, empty_row = (mol([1, 2, 1]) for _ in range(4))
    soft.x[1] = [0.5, 0.5, 0, 0]
    two_hot.x[2, 3] = 1.0
    empty_row.x[0] = 0
    for bad in (soft, two_hot, empty_row):
        with pytest.raises(ValueError, match=r"molecule 1: x is not one-hot.*--features"):
            ResidentMolecules.pack([good, bad])
    with pytest.raises(ValueError, match=r"molecule 1: x is not one-hot.*--features"):
        ResidentMolecules.pack([mol([0] * N, m_dim=ATOM_DIM + 54), _graphs(54, n=1)[0]])
    assert len(ResidentMolecules.pack([good])) == 3


def test_gather_features_extends_the_parameter_list_of_gather():
    """dg_mol_gather's parameters, in its order, with the plane after `entries` and (W, atom_dim) after E (tests/test_host.py
    holds both rows against include/druggen_hip.h)."""
    from druggen_amd import _lib
    base = list(_lib.SIGNATURES["dg_mol_gather"][1])
    assert _lib.SIGNATURES["dg_mol_gather_features"][1] == base[:3] + [ctypes.c_void_p] + base[3:9] + [ctypes.c_int] * 2 + base[9:]


def test_argument_validation_needs_no_gpu():
    from druggen_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(buf)

    def call(N=9, M=67, E=5, B=2, W=2, atom_dim=13, bits=p, x=p):
        return lib.dg_mol_gather_features(p, p, p, bits, 3, p, B, N, M, E, W, atom_dim, p, p, x, p, None)
    for kw in (dict(N=257), dict(N=0), dict(E=17), dict(E=0), dict(M=256, W=8), dict(M=0), dict(B=-1)):
        assert call(**kw) == -1, kw
        assert b"dg_mol_gather_features: need B >= 0, 1 <= N <= 256, 1 <= M <= 255, 1 <= E <= 16" in lib.dg_last_error_string()
    for kw in (dict(W=1), dict(W=3), dict(W=0), dict(atom_dim=0, W=3), dict(atom_dim=68, W=0), dict(atom_dim=-1, W=3),
               dict(atom_dim=3), dict(M=78)):      # (atom_dim 3: F = 64 is two words -- W fits, so that one passes the check)
        want = 0 if kw == dict(atom_dim=3) else -1
        got = call(B=0, **kw)      # B = 0: the shape checks come first, and nothing further is looked at
        assert got == want, kw
        if want:
            assert b"1 <= atom_dim <= M and W == ceil((M - atom_dim) / 32)" in lib.dg_last_error_string()
    assert call(W=1) == -1 and call(atom_dim=0, W=3) == -1      # ... and with B > 0
    assert call(bits=None) == -2 and b"dg_mol_gather_features: null pointer" in lib.dg_last_error_string()
    assert call(x=None) == -2 and b"dg_mol_gather_features: null pointer" in lib.dg_last_error_string()
    assert call(bits=p + 2) == -2 and b"dg_mol_gather_features: misaligned pointer" in lib.dg_last_error_string()
    assert call(bits=p + 1) == -2
    assert lib.dg_mol_gather_features(None, None, None, None, 0, None, 0, 9, 67, 5, 2, 13, None, None, None, None, None) == 0      # B == 0
