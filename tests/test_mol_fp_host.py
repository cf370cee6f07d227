"""Host side of the circular fingerprint (csrc/mol_fp.hip, druggen_amd/fingerprint.py): the plain-Python restatement
(tests/mol_fp_ref.py) against feature counts derived by hand, ring flags, invariance under atom order, the scope rules and the
min-id rule; the third public header against its ctypes table, every argument refusal of the C entry -- all of which return
before a launch -- and the host checks of fingerprint.py.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_fp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -1, -2      # DG_E_SHAPE, DG_E_ARG of include/druggen_hip.h
ATOM_LABEL = {z: l for l, z in ref.ATOM_DECODER.items()}
BOND_LABEL = {t: l for l, t in ref.BOND_DECODER.items()}


def from_smiles(s):
    """(atom labels, bond rows (hi, lo, label)) of a SMILES string, by the project's own parser."""
    from druggen_amd import smiles
    z, _, bonds = smiles.parse_smiles(s)
    return [ATOM_LABEL[a] for a in z], [(max(i, j), min(i, j), BOND_LABEL[t]) for i, j, t in bonds]


def _mol(atoms, labels):
    return dref.decode_labels(atoms, labels)


def _fp(atoms, labels, scope=ref.WHOLE, **kw):
    m = _mol(atoms, labels)
    return ref.fingerprint(m["atoms"], m["bonds"], n_bonds=m["n_bonds"], scope=scope, component=m["component"],
                           largest=m["largest"], **kw)


# ---- 1. feature counts derived by hand -------------------------------------------------------------------------------------
@pytest.mark.parametrize("smiles,radius,count", [
    ("CC", 2, 2),             # one id at layer 0; one shared environment at layer 1; nothing new at layer 2
    ("CCC", 2, 4),            # 2 at layer 0; ends share an id, middle its own at layer 1; all environments seen by layer 2
    ("c1ccccc1", 2, 3),       # one id per layer, six distinct environments each
    ("c1ccccc1", 3, 4),       # the six atoms share one new environment
    ("c1ccccc1", 4, 4),       # ... which layer 4 sees again
    ("C", 2, 1),              # a single atom
    ("CN", 2, 3),             # two ids at layer 0, one shared environment at layer 1: the smaller id
    ("CC", 0, 1), ("CCC", 1, 4), ("CCCC", 1, 4), ("CCCC", 2, 5),
])
def test_hand_derived_feature_counts(smiles, radius, count):
    atoms, rows = from_smiles(smiles)
    got = ref.fingerprint(atoms, rows, radius, 4096)
    assert got["n_features"] == count
    assert got["count"] <= count and got["count"] == len(ref.bit_set(got))


def test_all_pads_have_no_feature_under_whole_and_one_under_largest():
    pads = np.zeros(4, dtype=np.int64), dref.empty_graph(4)
    assert _fp(*pads, scope=ref.WHOLE) == dict(words=[0] * 32, count=0, n_features=0)
    one = _fp(*pads, scope=ref.LARGEST)
    assert (one["n_features"], one["count"]) == (1, 1)      # the single pad of component 0


# ---- 2. ring flags ---------------------------------------------------------------------------------------------------------------
def test_ring_flags():
    atoms, rows = from_smiles("C1CC1C")
    assert ref.ring_flags(4, rows) == [1, 1, 1, 0]
    atoms, rows = from_smiles("c1ccccc1-c1ccccc1")      # biphenyl: every atom in a ring, the linking bond a bridge
    assert ref.ring_flags(12, rows) == [1] * 12
    link = [k for k, (i, j, l) in enumerate(rows) if l == 1]
    at = {a: [k for k, (i, j, _) in enumerate(rows) if a in (i, j)] for a in range(12)}
    assert len(link) == 1 and not ref._connected(rows[link[0]][0], rows[link[0]][1], rows, at, link[0])
    assert all(ref._connected(i, j, rows, at, k) for k, (i, j, _) in enumerate(rows) if k != link[0])
    atoms, rows = from_smiles("c1ccccc1Cc1ccccc1")      # a bridge atom between two rings: in the 2-core, on no cycle
    assert ref.ring_flags(13, rows) == [1] * 6 + [0] + [1] * 6
    atoms, rows = from_smiles("C1CC12CC2")              # spiro
    assert ref.ring_flags(5, rows) == [1] * 5
    atoms, rows = from_smiles("C1CCC2CCCCC2C1C")        # fused, with a methyl
    assert ref.ring_flags(11, rows) == [1] * 10 + [0]
    assert ref.ring_flags(5, from_smiles("CC(C)CC")[1]) == [0] * 5
    # the flag enters the id: a ring carbon with two single bonds differs from a chain carbon with two
    _, ids, ring, _ = ref.features(*from_smiles("C1CC1"), 0, detail=True)
    _, chain, _, _ = ref.features(*from_smiles("CCC"), 0, detail=True)
    assert ids[0][0] != chain[0][1] and ring == [1, 1, 1]


# ---- 3. invariance under atom order -------------------------------------------------------------------------------------------
def _seeded_graphs():
    rng = np.random.default_rng(327)
    graphs = []
    for k in range(50):
        N = int(rng.integers(2, 21))
        kind = k % 5
        if kind == 0:                                         # sparse
            g = cref.molecule_like(rng, N, k % 4)
        elif kind == 1:                                       # dense
            g = rng.integers(0, 7, N), np.tril(rng.integers(0, 5, (N, N)), -1)
        elif kind == 2:                                       # disconnected
            a, l = cref.molecule_like(rng, N, 1)
            l[N // 2:, :N // 2] = 0
            g = a, l
        elif kind == 3:                                       # with pads, bonded and isolated
            a, l = cref.molecule_like(rng, N, 2)
            a = a.copy()
            a[rng.integers(0, N, 2)] = 0
            l[-1, :] = 0
            g = a, l
        else:                                                 # one label: many equal environments and ids
            g = cref.molecule_like(rng, N, 3, True)
        graphs.append((np.asarray(g[0]), np.asarray(g[1])))
    return rng, graphs


def test_outputs_do_not_depend_on_the_atom_order():
    rng, graphs = _seeded_graphs()
    distinct = set()
    for atoms, labels in graphs:
        base = _fp(atoms, labels, radius=3, nbits=1024)
        distinct.add(tuple(base["words"]))
        for _ in range(20):
            assert _fp(*cref.renumbered(rng, atoms, labels), radius=3, nbits=1024) == base
    assert len(distinct) >= 35


# ---- 4. scope, no graph, the min-id rule, popcounts --------------------------------------------------------------------------
def test_scope_rules():
    atoms = np.array([1, 2, 1, 3, 1, 2, 1, 0, 0])
    labels = np.pad(dref.two_equal_components(6), ((0, 3), (0, 3)))      # C-C-C and N-O-N, a lone C, two lone pads
    whole, largest = _fp(atoms, labels, ref.WHOLE), _fp(atoms, labels, ref.LARGEST)
    assert largest == ref.fingerprint(*from_smiles("CCC"))
    assert whole["n_features"] == 4 + 4 + 1      # CCC, NON, the lone atom; the pads are outside
    assert ref.bit_set(largest) < ref.bit_set(whole)
    # a bonded pad is inside the scope; rows that leave the scope, loops and ends >= N do not count
    assert ref.fingerprint([1, 0], [(1, 0, 1)])["n_features"] == 3
    m = _mol(atoms, labels)
    rows = [tuple(r) for r in m["bonds"]] + [(3, 3, 1), (200, 0, 1), (0, 9, 2)]
    assert ref.fingerprint(atoms, rows, scope=ref.WHOLE) == whole
    assert ref.fingerprint(atoms, rows + [(1, 0, 1)], scope=ref.LARGEST, component=m["component"], largest=m["largest"]) == largest
    # labels without a table row take the word 0xFFFFFFFF and order2 0
    a, b = ref.features([9, 1], [(1, 0, 7)], 1, detail=True)[1], ref.features([8, 1], [(1, 0, 6)], 1, detail=True)[1]
    assert a == b and a[0][0] == ref.mix64((ref.mix64((ref.mix64((ref.mix64(0xFFFFFFFF) + 1) & ref.M64) + 0) & ref.M64) + 0) & ref.M64)


def test_molecules_without_a_graph():
    atoms, rows = from_smiles("CCCC")
    blank = dict(words=[0] * 32, count=0, n_features=ref.NO_GRAPH)
    assert ref.fingerprint(atoms, rows[:2], n_bonds=3, cap=2) == blank
    assert ref.fingerprint(atoms, rows, flag=-2) == blank
    assert ref.fingerprint(atoms, rows, n_bonds=3, cap=3)["n_features"] == 5
    assert ref.fingerprint(atoms, rows, n_bonds=-5, cap=3)["n_features"] == 1      # a negative count reads no row


def test_an_environment_shared_by_atoms_with_different_ids_gives_the_smaller():
    atoms, rows = from_smiles("CN")
    F, ids, _, _ = ref.features(atoms, rows, 2, detail=True)
    assert ids[1][0] != ids[1][1] and F == {ids[0][0], ids[0][1], min(ids[1].values())}
    # O=C-N... the star N(C)(O)S: at layer 2 every atom's environment is all three bonds
    atoms, rows = from_smiles("N(C)(O)S")
    F, ids, _, _ = ref.features(atoms, rows, 2, detail=True)
    assert len(set(ids[2].values())) == 4
    assert F == set(ids[0].values()) | set(ids[1].values())
    assert len(F) == 4 + 4      # layer 1: three single-bond environments and the centre's; layer 2: all seen (the centre's)
    atoms, rows = from_smiles("CCN")      # layer 2: the two ends share the environment of the middle atom's layer 1
    F, ids, _, _ = ref.features(atoms, rows, 2, detail=True)
    assert F == set(ids[0].values()) | set(ids[1].values()) and len(F) == 6


@pytest.mark.parametrize("nbits", [32, 1024, 4096])
def test_counts_are_popcounts_and_features_grow_with_the_radius(nbits):
    rng = np.random.default_rng(nbits)
    atoms, labels = cref.molecule_like(rng, 24, 3)
    m = _mol(atoms, labels)
    before = set()
    for radius in range(ref.MAX_RADIUS + 1):
        F = ref.features(m["atoms"], m["bonds"], radius)
        got = ref.fingerprint(m["atoms"], m["bonds"], radius, nbits)
        assert before <= F and got["n_features"] == len(F) and len(got["words"]) == nbits // 32
        assert ref.bit_set(got) == {v % nbits for v in F} and got["count"] == len({v % nbits for v in F})
        before = F
    assert len(before) > 24


# ---- 5. the third header against the third table ---------------------------------------------------------------------------
def _kind(decl):
    decl = re.sub(r"\bconst\b", " ", decl).strip()
    if "*" in decl or re.match(r"dg_stream_t\b", decl):
        return "pointer"
    kind = decl.split()[0]
    assert kind in ("int", "int64_t", "size_t", "float", "double"), decl
    return kind


def test_fp_header_matches_its_ctypes_table_parameter_by_parameter():
    from druggen_amd import _lib, build
    named = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
             ctypes.c_double: "double", ctypes.c_char_p: "pointer", ctypes.c_void_p: "pointer"}
    path = os.path.join(ROOT, "include", "druggen_hip_fp.h")
    assert path in [os.path.abspath(h) for h in build.HEADERS]
    header = open(path).read()
    assert re.search(r'^#include "druggen_hip.h"', header, flags=re.M)
    macro = {k: int(v) for k, v in re.findall(r"^#define\s+(DG_FP_[A-Z_]+)\s+\(?(-?\d+)\)?", header, flags=re.M)}
    assert macro == {"DG_FP_NO_GRAPH": ref.NO_GRAPH, "DG_FP_MAX_RADIUS": ref.MAX_RADIUS}
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    header = re.sub(r"^\s*#.*$", " ", header, flags=re.M)
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header)
    names = [name for _, name, _ in protos]
    assert names == list(_lib.FP_SIGNATURES) == ["dg_mol_fingerprint"]
    assert not set(names) & set(_lib.SIGNATURES) and not set(names) & set(_lib.TEXT_SIGNATURES)
    for other in ("druggen_hip.h", "druggen_hip_text.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(rf"\b{name}\s*\(", text) for name in names), other
    lib = _lib.load()
    for ret, name, params in protos:
        res, args = _lib.FP_SIGNATURES[name]
        want = [_kind(ret)] + [_kind(p) for p in params.split(",")]
        assert want == [named[res]] + [named[a] for a in args], (name, want)
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, name
    assert lib.dg_version() == 232


# ---- 6. every refusal of the C entry ---------------------------------------------------------------------------------------
_buf = (ctypes.c_int64 * 8)()
P = ctypes.addressof(_buf)      # a non-null, 8-byte aligned pointer: no call below gets as far as reading it


def test_entry_argument_checks():
    """None of these calls launches, and B == 0 returns 0 without one."""
    from druggen_amd import _lib
    lib = _lib.load()
    names = ("atoms", "bonds", "n_bonds", "component", "largest", "flags", "atom_words", "bond_table", "words", "counts",
             "n_features")

    def call(B=3, N=9, cap=36, scope=1, radius=2, nbits=1024, n_atom_labels=7, n_bond_labels=5, **ptrs):
        p = {n: P for n in names}
        p.update(ptrs)
        return lib.dg_mol_fingerprint(p["atoms"], p["bonds"], p["n_bonds"], p["component"], p["largest"], p["flags"],
                                      p["atom_words"], n_atom_labels, p["bond_table"], n_bond_labels, B, N, cap, scope, radius,
                                      nbits, p["words"], p["counts"], p["n_features"], None)

    def err():
        return lib.dg_last_error_string()
    for kw in (dict(B=-1), dict(N=0), dict(N=257), dict(N=-4), dict(N=1 << 20), dict(cap=-1), dict(radius=-1), dict(radius=5),
               dict(nbits=0), dict(nbits=31), dict(nbits=48), dict(nbits=1000), dict(nbits=4128), dict(nbits=8192), dict(nbits=-32),
               dict(n_atom_labels=0), dict(n_atom_labels=256), dict(n_bond_labels=0), dict(n_bond_labels=257)):
        assert call(**kw) == SHAPE and b"dg_mol_fingerprint: need B >= 0, 1 <= N <= 256" in err(), kw
    for scope in (-1, 2, 3, 256):
        assert call(scope=scope) == ARG and b"scope must be 0 (whole) or 1 (largest)" in err(), scope
    for name in ("atoms", "n_bonds", "atom_words", "bond_table", "words", "counts", "n_features", "bonds", "component", "largest"):
        assert call(**{name: None}) == ARG and b"dg_mol_fingerprint: null pointer" in err(), name
    for name in ("bonds", "n_bonds", "largest", "flags", "atom_words", "bond_table", "words", "counts", "n_features"):
        assert call(**{name: P + 2}) == ARG and b"aligned" in err(), name
    # the shape comes first, then the scope, then the pointers
    assert call(N=257, scope=5, atoms=None) == SHAPE and call(scope=5, atoms=None) == ARG and b"scope" in err()
    # an empty batch is no launch; the optional pointers may be null, B == 0 still checks the rest; every legal extreme passes
    assert call(B=0) == 0 and call(B=0, flags=None) == 0 and call(B=0, cap=0, bonds=None) == 0
    assert call(B=0, scope=0, component=None, largest=None) == 0
    assert call(B=0, N=256, cap=32640, radius=4, nbits=4096, n_atom_labels=255, n_bond_labels=256) == 0
    assert call(B=0, N=1, cap=0, radius=0, nbits=32, n_atom_labels=1, n_bond_labels=1) == 0
    assert call(B=0, scope=1, component=None) == ARG and call(B=0, words=None) == ARG and call(B=0, scope=2) == ARG


# ---- 7. fingerprint.py -----------------------------------------------------------------------------------------------------------
def test_tables_from_decoders():
    from druggen_amd import fingerprint
    atom_words, bond_rows = fingerprint.table_words(ref.ATOM_DECODER, ref.BOND_DECODER)
    assert atom_words.tolist() == ref.ATOM_WORDS and atom_words.dtype == np.uint32
    assert [tuple(r) for r in bond_rows.tolist()] == ref.BOND_ROWS and bond_rows.dtype == np.uint32
    assert fingerprint.table_words({0: 0, 1: 14, 2: 53}, {0: 0})[0].tolist() == [0, 14, 53]
    for bad in ({0: 0, 1: 1}, {0: 0, 1: 55}, {0: 0, 1: -6}):
        with pytest.raises(ValueError, match="atomic number"):
            fingerprint.table_words(bad, ref.BOND_DECODER)
    with pytest.raises(ValueError, match="bond type"):
        fingerprint.table_words(ref.ATOM_DECODER, {0: 0, 1: 4})
    for bad in ({}, {1: 6}, {0: 0, 2: 6}):
        with pytest.raises(ValueError, match="labels 0..n-1"):
            fingerprint.table_words(bad, ref.BOND_DECODER)
    with pytest.raises(ValueError, match="256 labels"):
        fingerprint.table_words({l: 6 for l in range(256)}, ref.BOND_DECODER)
    tables = fingerprint.FingerprintTables.from_decoders(ref.ATOM_DECODER, ref.BOND_DECODER, "cpu")
    assert (tables.n_atom_labels, tables.n_bond_labels) == (7, 5) and tables.bonds.shape == (5, 2)
    assert (fingerprint.NO_GRAPH, fingerprint.MAX_RADIUS) == (ref.NO_GRAPH, ref.MAX_RADIUS)


def test_python_refusals_without_a_gpu():
    """fingerprint.py refuses host batches, other sources, other tables, a bad scope, radius, nbits and out= -- all before any
    launch -- and its result is a metrics.PackedFingerprints."""
    import torch
    from druggen_amd import fingerprint, metrics
    from druggen_amd.decode import MoleculeBatch, _layout
    tables = fingerprint.FingerprintTables.from_decoders(ref.ATOM_DECODER, ref.BOND_DECODER, "cpu")
    host = MoleculeBatch(np.zeros(_layout(2, 3, 3, False)[1], dtype=np.uint8), 2, 3, 3, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fingerprint.circular_fingerprints(host, tables)
    with pytest.raises(TypeError, match="MoleculeBatch"):
        fingerprint.circular_fingerprints(np.zeros(4), tables)

    class Device:      # stands in for a device buffer: the checks below come before anything touches it
        is_cuda, device = True, "cuda:0"
    host.is_host, host.buffer = False, Device()
    with pytest.raises(ValueError, match="scope must be"):
        fingerprint.circular_fingerprints(host, tables, scope="fragment")
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="radius"):
            fingerprint.circular_fingerprints(host, tables, radius=bad)
    for bad in (0, 48, 8192):
        with pytest.raises(ValueError, match="multiple of 32"):
            fingerprint.circular_fingerprints(host, tables, nbits=bad)
    with pytest.raises(TypeError, match="FingerprintTables"):
        fingerprint.circular_fingerprints(host, (ref.ATOM_WORDS, ref.BOND_ROWS))
    with pytest.raises(ValueError, match="the tables live on cpu"):
        fingerprint.circular_fingerprints(host, tables)
    tables.device = "cuda:0"
    for out in (np.zeros(3), fingerprint.CircularFingerprints.empty(2, 1024, "cpu"), fingerprint.CircularFingerprints.empty(3, 64, "cpu")):
        with pytest.raises(ValueError, match="out="):      # not fingerprints; host ones; another shape
            fingerprint.circular_fingerprints(host, tables, nbits=64, out=out)
    fps = fingerprint.CircularFingerprints.empty(3, 64, "cpu")
    assert isinstance(fps, metrics.PackedFingerprints) and len(fps) == 3 and fps.words.shape == (3, 2)
    assert fps.n_features.dtype == torch.int32 and metrics.pack_fingerprints(fps) is fps
