"""Host side of the scaffolds (csrc/mol_scaf.hip, druggen_amd/scaffolds.py): the plain-Python restatement
(tests/mol_scaf_ref.py) against results worked by hand through `parse_smiles` and against the hand-worked fixture rows, its
behaviour under atom order, the derived graph against the decode's restatement, the similarity counts against a `Counter` over
forms; the seventh public header against its ctypes table, every argument refusal of the C entry -- all of which return before a
launch -- and the host checks of scaffolds.py and its record.  No GPU."""
import ctypes
import json
import math
import os
import re
from collections import Counter

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_desc_ref as descref
import mol_fp_ref as fref
import mol_scaf_ref as ref
import mol_valid_ref as vref
from test_mol_desc_host import fixture_tables
from test_mol_valid_host import _kind, from_smiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -1, -2      # DG_E_SHAPE, DG_E_ARG of include/druggen_hip.h


def graph_of(smiles, N=None):
    """(atom labels [N], dense bond labels [N,N]) of a SMILES string under mol_fp_ref's decoders."""
    atoms, rows = from_smiles(smiles)
    N = N or len(atoms)
    a, labels = np.zeros(N, dtype=np.int64), np.zeros((N, N), dtype=np.int64)
    a[:len(atoms)] = atoms
    for i, j, l in rows:
        labels[i, j] = l
    return a, labels


def scaffold_of(atoms, labels, scope=descref.WHOLE, **tables):
    """The restatement chain decode -> validity -> descriptors -> scaffold of one molecule; (result, molecule dict, descriptors)."""
    m = dref.decode_labels(atoms, labels)
    kw = dict(scope=scope, component=m["component"], largest=m["largest"])
    valid = vref.validity(m["atoms"], m["bonds"], **kw, **tables.get("vtab", {}))
    desc = descref.describe(m["atoms"], m["bonds"], valid, **kw, **tables.get("dtab", {}))
    bond_rows = tables.get("dtab", {}).get("bond_rows", vref.BOND_ROWS)
    return ref.scaffold(m["atoms"], m["bonds"], desc, bond_rows), m, desc


def _fields(result):
    return dict(zip(ref.MOL_FIELDS, result["mol"]))


def _hist(**bins):
    return [bins.get(f"s{name}", 0) for name in (3, 4, 5, 6, 7, 8, 9, 13)]


# ---- 1. results worked by hand ------------------------------------------------------------------------------------------------------
SIX = dict(n_scaffold_atoms=6, n_scaffold_bonds=6, n_exo=0, n_linker_atoms=0, n_ring_atoms=6, n_ring_bonds=6, n_rings=1,
           n_ring_systems=1, largest_system_atoms=6, min_ring=6, max_ring=6)


@pytest.mark.parametrize("smiles,want,hist", [
    # aspirin, paracetamol, ibuprofen: every substituent hangs on the ring by a single bond and ends without a ring: the bare
    # six-ring, 6 atoms and 6 bonds of size 6
    ("CC(=O)Oc1ccccc1C(=O)O", dict(SIX, n_heavy=13), _hist(s6=6)),
    ("CC(=O)Nc1ccc(O)cc1", dict(SIX, n_heavy=11), _hist(s6=6)),
    ("CC(C)Cc1ccc(cc1)C(C)C(=O)O", dict(SIX, n_heavy=15), _hist(s6=6)),
    # caffeine: the purine core 9 atoms / 10 ring bonds (5 + 6 - the shared one), the two carbonyl O are exo (2 more atoms and
    # bonds), the three methyls go; 10 - 9 + 1 = 2 rings; the fusion bond lies in the five-ring: 5 bonds of size 5, 5 of size 6
    ("Cn1cnc2c1c(=O)n(C)c(=O)n2C", dict(n_heavy=14, n_scaffold_atoms=11, n_scaffold_bonds=12, n_exo=2, n_linker_atoms=0, n_ring_atoms=9,
                                        n_ring_bonds=10, n_rings=2, n_ring_systems=1, largest_system_atoms=9, min_ring=5, max_ring=6),
     _hist(s5=5, s6=5)),
    # biphenyl: two rings and the bond between them: 12 atoms, 13 bonds, 2 systems, no linker ATOM
    ("c1ccccc1-c1ccccc1", dict(n_scaffold_atoms=12, n_scaffold_bonds=13, n_linker_atoms=0, n_ring_systems=2, n_rings=2,
                               largest_system_atoms=6), _hist(s6=12)),
    # diphenylmethane: the CH2 is a linker: 13 atoms, 12 + 2 bonds
    ("c1ccccc1Cc1ccccc1", dict(n_scaffold_atoms=13, n_scaffold_bonds=14, n_linker_atoms=1, n_exo=0, n_ring_systems=2), _hist(s6=12)),
    # benzophenone: 12 ring atoms + the linker C = 13 core atoms, its O is exo: 14 atoms, 12 + 2 + 1 = 15 bonds
    ("O=C(c1ccccc1)c1ccccc1", dict(n_scaffold_atoms=14, n_scaffold_bonds=15, n_linker_atoms=1, n_exo=1, n_ring_atoms=12), _hist(s6=12)),
    # 2-methylcyclohexanone: the ring, its =O; the methyl goes: 6 + 1 atoms, 6 + 1 bonds
    ("CC1CCCCC1=O", dict(n_heavy=8, n_scaffold_atoms=7, n_scaffold_bonds=7, n_exo=1, n_ring_atoms=6, n_rings=1), _hist(s6=6)),
    # hexane: peeling eats the chain from both ends: empty
    ("CCCCCC", dict(n_heavy=6, n_scaffold_atoms=0, n_scaffold_bonds=0, n_rings=0, n_ring_systems=0, largest_system_atoms=0, min_ring=0,
                    max_ring=0), _hist()),
    # naphthalene: 10 atoms, 11 bonds, one system, 11 - 10 + 1 = 2 rings; every bond, the shared one too, lies in a six-ring
    ("c1ccc2ccccc2c1", dict(n_scaffold_atoms=10, n_ring_bonds=11, n_ring_systems=1, n_rings=2, largest_system_atoms=10), _hist(s6=11)),
    # spiro[4.5]decane: the rings share one ATOM, so their bonds are one connected set: 1 system; 5 bonds of 5, 6 of 6
    ("C1CCC2(C1)CCCCC2", dict(n_ring_atoms=10, n_ring_bonds=11, n_ring_systems=1, n_rings=2, min_ring=5, max_ring=6), _hist(s5=5, s6=6)),
    # cubane: 8 atoms, 12 bonds, 12 - 8 + 1 = 5 rings, every bond in a square
    ("C12C3C4C1C5C2C3C45", dict(n_ring_atoms=8, n_ring_bonds=12, n_rings=5, n_ring_systems=1, min_ring=4, max_ring=4), _hist(s4=12)),
    # the double bond sits one atom away from the ring: its carbon is no core atom and is bonded to the ring by a SINGLE bond
    ("C1CC1C(=C(C)C)C", dict(n_heavy=8, n_scaffold_atoms=3, n_scaffold_bonds=3, n_exo=0, n_rings=1), _hist(s3=3)),
    # two cyclopropyls on CH2-C(=O)-CH2: three linkers, the O is exo on a LINKER: 6 + 3 + 1 atoms, 6 + 4 + 1 bonds
    ("C1CC1CC(=O)CC1CC1", dict(n_heavy=10, n_scaffold_atoms=10, n_scaffold_bonds=11, n_exo=1, n_linker_atoms=3, n_ring_atoms=6,
                               n_ring_systems=2, n_rings=2, largest_system_atoms=3), _hist(s3=6)),
])
def test_hand_worked_results(smiles, want, hist):
    got, m, desc = scaffold_of(*graph_of(smiles))
    fields = _fields(got)
    assert fields["status"] == 0 and {k: fields[k] for k in want} == want and got["hist"] == hist, (fields, got["hist"])
    assert fields["n_rings"] == desc["desc"][5] and got["mol"][13:] == [0, 0, 0]
    assert fields["n_scaffold_atoms"] == fields["n_exo"] + fields["n_linker_atoms"] + fields["n_ring_atoms"]
    # two exo atoms are never bonded to each other, and each has exactly one bond into the core
    for i, j, _ in got["s_rows"]:
        assert not (i in got["exo"] and j in got["exo"])
    for x in got["exo"]:
        assert sum(1 for i, j, _ in got["s_rows"] if x in (i, j)) == 1
    # the derived graph is the decode's restatement of the scaffold graph: rows in the list's order, components by its tie rule
    d = got["derived"]
    assert [tuple(r) for r in d["bonds"].tolist()] == got["s_rows"] and d["n_bonds"] == fields["n_scaffold_bonds"]
    assert d["atoms"].tolist() == got["s_atoms"] and d["n_components"] == len(m["atoms"]) - fields["n_scaffold_atoms"] + (fields["n_scaffold_atoms"] > 0)


def test_roles_systems_and_sizes_by_hand():
    # 2-methylcyclohexanone C C1 C C C C C1 =O: atom 0 the methyl, 1..6 the ring, 7 the O
    got, _, _ = scaffold_of(*graph_of("CC1CCCCC1=O"))
    assert got["role"] == [ref.SIDE] + [ref.RING] * 6 + [ref.EXO] and got["system"] == [255] + [1] * 6 + [255]
    assert got["s_atoms"] == [0, 1, 1, 1, 1, 1, 1, 3] and sorted(got["sizes"]) == [0, 0] + [6] * 6
    # benzophenone O=C(c1ccccc1)c1ccccc1: O exo, C linker, two systems named by their smallest atoms 2 and 8
    got, _, _ = scaffold_of(*graph_of("O=C(c1ccccc1)c1ccccc1"))
    assert got["role"] == [ref.EXO, ref.LINKER] + [ref.RING] * 12 and got["system"] == [255, 255] + [2] * 6 + [8] * 6
    # hexane: all side chain; the derived batch is N one-atom components, largest 0 of size 1
    got, _, _ = scaffold_of(*graph_of("CCCCCC"))
    d = got["derived"]
    assert got["role"] == [ref.SIDE] * 6 and got["s_atoms"] == [0] * 6 and got["s_rows"] == []
    assert (d["n_bonds"], d["n_components"], d["largest"], d["largest_size"]) == (0, 6, 0, 1) and d["component"].tolist() == list(range(6))
    # naphthalene's fusion bond lies in two six-rings: size 6; norbornane-like bicyclo[2.2.1]: every bond in a five-ring
    assert set(scaffold_of(*graph_of("c1ccc2ccccc2c1"))[0]["sizes"]) == {6}
    assert scaffold_of(*graph_of("C1CC2CCC1C2"))[0]["hist"] == _hist(s5=8)
    # a pad position and a second fragment under both scopes: outside the scope is role 0, label 0
    atoms, labels = cref.from_edges(9, [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (5, 6), (3, 6)])      # a triangle, a square, two pads
    atoms[7:] = 0
    whole, _, _ = scaffold_of(atoms, labels, descref.WHOLE)
    largest, _, _ = scaffold_of(atoms, labels, descref.LARGEST)
    assert whole["role"] == [4] * 7 + [0, 0] and _fields(whole)["n_ring_systems"] == 2 and whole["hist"] == _hist(s3=3, s4=4)
    assert largest["role"] == [0] * 3 + [4] * 4 + [0, 0] and largest["s_atoms"] == [0, 0, 0, 1, 1, 1, 1, 0, 0]
    assert (largest["derived"]["largest"], largest["derived"]["largest_size"], largest["derived"]["n_components"]) == (3, 4, 6)
    assert (whole["derived"]["largest"], whole["derived"]["largest_size"], whole["derived"]["n_components"]) == (3, 4, 4)


def test_a_status_other_than_valid_gives_the_empty_result():
    got, m, desc = scaffold_of(*graph_of("c1cccc1"))      # not kekulisable
    assert desc["desc"][0] == 5 and got["hist"] == [0] * 8 and got["s_rows"] == []
    assert got["mol"] == [5] + [0] * 15 and got["role"] == [0] * 5 and got["system"] == [255] * 5 and got["sizes"] == [0] * 5
    d = got["derived"]
    assert d["atoms"].tolist() == [0] * 5 and (d["n_bonds"], d["n_components"], d["largest"], d["largest_size"]) == (0, 5, 0, 1)


def test_saturation_and_long_structures():
    """Cycles of 254, 255 and 256 atoms read 254, 255 and 255; a 256-chain is empty; a triangle with a long tail keeps the
    triangle; two triangles joined by a linker keep everything."""
    for n, size in ((254, 254), (255, 255), (256, 255)):
        got, _, _ = scaffold_of(*cref.cycle(n))
        assert set(got["sizes"]) == {size} and got["hist"] == [0] * 7 + [n] and _fields(got)["n_rings"] == 1
    got, _, _ = scaffold_of(*cref.from_edges(256, [(i, i + 1) for i in range(255)]))
    assert _fields(got)["n_scaffold_atoms"] == 0 and got["role"] == [ref.SIDE] * 256
    got, _, _ = scaffold_of(*cref.from_edges(256, [(0, 1), (1, 2), (0, 2)] + [(i, i + 1) for i in range(2, 255)]))
    assert _fields(got)["n_scaffold_atoms"] == 3 and got["role"] == [4] * 3 + [1] * 253
    edges = [(0, 1), (1, 2), (0, 2)] + [(i, i + 1) for i in range(2, 253)] + [(253, 254), (254, 255), (253, 255)]
    got, _, _ = scaffold_of(*cref.from_edges(256, edges))
    f = _fields(got)
    assert (f["n_scaffold_atoms"], f["n_linker_atoms"], f["n_ring_systems"], f["n_scaffold_bonds"]) == (256, 250, 2, 257)


# ---- 2. the fixture molecules ------------------------------------------------------------------------------------------------------
def golden_scaffold_rows():
    with open(os.path.join(ROOT, "tests", "golden", "chembl_like_scaffolds.json")) as f:
        return json.load(f)


def fixture_wanted(scope):
    """(strings, molecule dicts, descriptor results, scaffold results) of the fixture molecules under `scope`."""
    strings, atoms, labels, atom_dec, bond_dec, vtab, dtab = fixture_tables()
    out = [scaffold_of(atoms[b], labels[b], scope, vtab=vtab, dtab=dtab) for b in range(len(strings))]
    return strings, [m for _, m, _ in out], [d for _, _, d in out], [w for w, _, _ in out]


def test_fixture_molecules_have_their_hand_worked_rows():
    """tests/golden/chembl_like_scaffolds.json: the eight molecules of chembl_like_smiles.csv, every row worked by hand in its
    comment; both scopes (the molecules are connected)."""
    golden = golden_scaffold_rows()
    for scope in (descref.WHOLE, descref.LARGEST):
        strings, _, descs, want = fixture_wanted(scope)
        assert [g["smiles"] for g in golden] == strings and all(g["comment"] for g in golden)
        for g, d, w in zip(golden, descs, want):
            assert _fields(w) == {k: g[k] for k in ref.MOL_FIELDS} and w["hist"] == g["ring_hist"], g["smiles"]
            assert w["mol"][8] == d["desc"][5] and w["mol"][6] == d["desc"][6]
    assert [g["status"] for g in golden] == [0] * 7 + [5]
    first, second = golden[:2]
    assert (first["n_scaffold_atoms"], first["n_linker_atoms"], first["n_ring_systems"], first["n_rings"]) == (30, 6, 4, 5)
    assert first["ring_hist"] == _hist(s3=3, s5=5, s6=17) and second["ring_hist"] == _hist(s5=5, s6=23)
    assert (second["n_scaffold_atoms"], second["n_linker_atoms"], second["n_ring_systems"], second["n_rings"]) == (27, 0, 4, 5)


# ---- 3. atom order -------------------------------------------------------------------------------------------------------------------
def test_roles_and_sizes_permute_with_the_atoms():
    rng = np.random.default_rng(33)
    for smiles in ("Cn1cnc2c1c(=O)n(C)c(=O)n2C", "C1CC1CC(=O)CC1CC1", "O=C(c1ccccc1)c1ccccc1", "CC1CCCCC1=O"):
        atoms, labels = graph_of(smiles)
        base, m, _ = scaffold_of(atoms, labels)
        size_of = {frozenset(r[:2]): s for r, s in zip(m["bonds"].tolist(), base["sizes"])}
        for _ in range(3):
            a, l, perm = vref.renumbered(rng, atoms, labels)      # new position p holds old atom perm[p]
            got, pm, _ = scaffold_of(a, l)
            old = {p: int(perm[p]) for p in range(len(perm))}
            assert got["mol"] == base["mol"] and got["hist"] == base["hist"]
            assert got["role"] == [base["role"][old[p]] for p in range(len(perm))]
            assert [s == 255 for s in got["system"]] == [base["system"][old[p]] == 255 for p in range(len(perm))]
            assert got["sizes"] == [size_of[frozenset((old[i], old[j]))] for i, j, _ in pm["bonds"].tolist()]
            # ... and the scaffolds are the same labelled graph
            forms = [cref.form_of(cref.canon(w["derived"]["atoms"], w["derived"]["bonds"], scope=cref.WHOLE)) for w in (base, got)]
            assert forms[0] == forms[1]


# ---- 4. the similarity counts ----------------------------------------------------------------------------------------------------------
def test_similarity_counts_against_a_counter_over_forms():
    """Equal scaffolds of differently decorated molecules are one form: toluene, phenol and aspirin share the bare six-ring;
    biphenyl and 4-methylbiphenyl share theirs."""
    def wants(strings):
        return [scaffold_of(*graph_of(s))[0] for s in strings]
    stock = wants(["c1ccccc1-c1ccccc1", "Cc1ccc(cc1)-c1ccccc1", "c1ccc2ccccc2c1", "Cc1ccccc1", "CCCC", "c1ccccc1Cc1ccccc1"])
    gen = wants(["c1ccccc1-c1ccccc1", "c1ccc2ccccc2c1", "Cc1ccc2ccccc2c1", "Oc1ccc2ccccc2c1", "C1CC1CC(=O)CC1CC1", "CC", "c1cccc1"])
    # min_rings 2: stock {biphenyl 2, naphthalene 1, diphenylmethane 1}; gen {biphenyl 1, naphthalene 3, the diketone-like 1}
    assert ref.similarity_counts(gen, stock, 2) == (1 * 2 + 3 * 1, 1 + 9 + 1, 4 + 1 + 1)
    # min_rings 1: the six-ring of toluene joins the stock; nothing of gen has it
    assert ref.similarity_counts(gen, stock, 1) == (5, 11, 7)
    assert ref.similarity_counts(gen, stock, 3) == (0, 0, 0) and math.isnan(ref.similarity(0, 0, 0))
    forms = ref.kept_forms(stock, 2)
    assert sorted(forms.values()) == [1, 1, 2] and isinstance(forms, Counter)
    assert ref.similarity(5, 11, 6) == 5 / math.sqrt(66.0) and math.isnan(ref.similarity(0, 3, 0))


# ---- 5. the seventh header against the seventh table -----------------------------------------------------------------------------------
def test_scaf_header_matches_its_ctypes_table_parameter_by_parameter():
    from druggen_amd import _lib, build, scaffolds
    named = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
             ctypes.c_double: "double", ctypes.c_char_p: "pointer", ctypes.c_void_p: "pointer"}
    path = os.path.join(ROOT, "include", "druggen_hip_scaf.h")
    others = build.HEADERS + [build.DESC_HEADER, build.SUB_HEADER]
    assert os.path.abspath(build.SCAF_HEADER) == path and path not in [os.path.abspath(h) for h in others]
    header = open(path).read()
    assert re.search(r'^#include "druggen_hip_desc.h"', header, flags=re.M)
    macro = {k: int(v) for k, v in re.findall(r"^#define\s+(DG_SCAF_[A-Z_]+)\s+\(?(-?\d+)\)?", header, flags=re.M)}
    assert macro == {"DG_SCAF_MOL_FIELDS": ref.N_MOL, "DG_SCAF_HIST_BINS": ref.HIST_BINS, "DG_SCAF_MAX_RING": ref.MAX_RING,
                     "DG_SCAF_NO_SYSTEM": ref.NO_SYSTEM, "DG_SCAF_ROLE_NONE": ref.NONE, "DG_SCAF_ROLE_SIDE": ref.SIDE,
                     "DG_SCAF_ROLE_EXO": ref.EXO, "DG_SCAF_ROLE_LINKER": ref.LINKER, "DG_SCAF_ROLE_RING": ref.RING}
    assert scaffolds.MOL_FIELDS == ref.MOL_FIELDS and len(scaffolds.HIST_BINS) == ref.HIST_BINS and len(scaffolds.ROLES) == 5
    assert (scaffolds.MAX_RING, scaffolds.NO_SYSTEM) == (ref.MAX_RING, ref.NO_SYSTEM)
    for word in ("NOT checked against it", "no ring is enumerated", "Kekule"):
        assert word in header, word
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    header = re.sub(r"^\s*#.*$", " ", header, flags=re.M)
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header)
    names = [name for _, name, _ in protos]
    assert names == list(_lib.SCAF_SIGNATURES) == ["dg_mol_scaffold"]
    for table in (_lib.SIGNATURES, _lib.TEXT_SIGNATURES, _lib.FP_SIGNATURES, _lib.VALID_SIGNATURES, _lib.DESC_SIGNATURES, _lib.SUB_SIGNATURES):
        assert not set(names) & set(table)
    for other in others:
        text = open(other).read()
        assert not any(re.search(rf"\b{name}\s*\(", text) for name in names), other
    lib = _lib.load()
    for ret, name, params in protos:
        res, args = _lib.SCAF_SIGNATURES[name]
        want = [_kind(ret)] + [_kind(p) for p in params.split(",")]
        assert want == [named[res]] + [named[a] for a in args], (name, want)
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, name
    assert lib.dg_version() == 232


# ---- 6. every refusal of the C entry ------------------------------------------------------------------------------------------------
_buf = (ctypes.c_int64 * 8)()
P = ctypes.addressof(_buf)      # a non-null, 8-byte aligned pointer: no call below gets as far as reading it
NAMES = ("atoms", "bonds", "n_bonds", "desc", "atom_key", "bond_class", "bond_table", "mol", "ring_hist", "atom_role", "atom_system",
         "bond_ring_size", "s_atoms", "s_bonds", "s_n_bonds", "s_component", "s_n_components", "s_largest", "s_largest_size")


def test_entry_argument_checks():
    """None of these calls launches, and B == 0 returns 0 without one."""
    from druggen_amd import _lib
    lib = _lib.load()

    def call(B=3, N=9, cap=36, n_bond_labels=5, **ptrs):
        p = {n: P for n in NAMES}
        p.update(ptrs)
        return lib.dg_mol_scaffold(*(p[n] for n in NAMES[:7]), n_bond_labels, B, N, cap, *(p[n] for n in NAMES[7:]), None)

    def err():
        return lib.dg_last_error_string()
    for kw in (dict(B=-1), dict(N=0), dict(N=257), dict(N=-4), dict(N=1 << 20), dict(cap=-1), dict(n_bond_labels=0), dict(n_bond_labels=257)):
        assert call(**kw) == SHAPE and b"dg_mol_scaffold: need B >= 0, 1 <= N <= 256" in err(), kw
    for name in NAMES:
        assert call(**{name: None}) == ARG and b"dg_mol_scaffold: null pointer" in err(), name
    for name in ("bonds", "n_bonds", "desc", "atom_key", "bond_table", "mol", "ring_hist", "s_bonds", "s_n_bonds", "s_n_components",
                 "s_largest", "s_largest_size"):
        assert call(**{name: P + 2}) == ARG and b"aligned" in err(), name
    # the shape comes first, then the pointers
    assert call(N=257, atoms=None) == SHAPE and call(atoms=None, mol=P + 2) == ARG and b"null pointer" in err()
    # an empty batch is no launch; the four bond arrays may be null without a bond row; every legal extreme passes
    assert call(B=0) == 0 and call(B=0, cap=0, bonds=None, bond_class=None, bond_ring_size=None, s_bonds=None) == 0
    assert call(B=0, atoms=P + 1, bond_class=P + 3, atom_role=P + 1, s_component=P + 3) == 0
    assert call(B=0, N=256, cap=32640, n_bond_labels=256) == 0 and call(B=0, N=1, cap=0, n_bond_labels=1) == 0
    assert call(B=0, mol=None) == ARG and call(B=0, cap=1, s_bonds=None) == ARG and call(B=0, N=257) == SHAPE


# ---- 7. scaffolds.py -------------------------------------------------------------------------------------------------------------------
def test_python_refusals_and_the_record_without_a_gpu():
    import torch
    from druggen_amd import descriptors, scaffolds, validity
    from druggen_amd._packed import PackedRecord
    from druggen_amd.decode import MoleculeBatch, _layout
    from druggen_amd.sampling import MoleculeSampler
    dtables = descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    vtables = validity.ValenceTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    host = MoleculeBatch(np.zeros(_layout(2, 3, 3, False)[1], dtype=np.uint8), 2, 3, 3, False)
    described = descriptors.MoleculeDescriptors.empty(2, 3, 3, "cpu")
    assert host.scaffolds is None and MoleculeBatch.scaffolds is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scaffolds.murcko_scaffolds(host, described, dtables)
    with pytest.raises(TypeError, match="MoleculeBatch"):
        scaffolds.murcko_scaffolds(np.zeros(4), described, dtables)

    class Device:      # stands in for a device buffer: the checks below come before anything touches it
        is_cuda, device = True, "cuda:0"
    host.is_host, host.buffer = False, Device()
    with pytest.raises(TypeError, match="DescriptorTables"):
        scaffolds.murcko_scaffolds(host, described, vtables)
    with pytest.raises(ValueError, match="the tables live on cpu"):
        scaffolds.murcko_scaffolds(host, described, dtables)
    dtables.device = "cuda:0"
    for bad in (None, np.zeros(3), described, described.cpu(), descriptors.MoleculeDescriptors.empty(3, 3, 3, "cpu")):
        with pytest.raises(ValueError, match="descriptors="):
            scaffolds.murcko_scaffolds(host, bad, dtables)
    described.buffer = Device()      # now it passes for this batch's record; every out= below is refused before a launch
    wrong_n = scaffolds.MoleculeScaffolds.empty(2, 4, 3, "cpu")
    no_batch = scaffolds.MoleculeScaffolds.empty(2, 3, 3, "cpu")
    no_batch.batch = None
    with_valence = scaffolds.MoleculeScaffolds.empty(2, 3, 3, "cpu")
    with_valence.batch = MoleculeBatch.empty(2, 3, 3, True, "cpu")
    for bad in (np.zeros(3), wrong_n, no_batch, with_valence, scaffolds.MoleculeScaffolds.empty(2, 3, 3, "cpu").cpu(),
                scaffolds.MoleculeScaffolds.empty(2, 3, 3, "cpu")):      # (the last: on another device than the batch)
        with pytest.raises(ValueError, match="out="):
            scaffolds.murcko_scaffolds(host, described, dtables, out=bad)

    class Store:
        device, vertexes = "cuda:0", 3

        def __len__(self):
            return 2
    for bad in (0, -3):
        with pytest.raises(ValueError, match="chunk"):
            scaffolds.scaffold_store(Store(), vtables, dtables, chunk=bad)
    with pytest.raises(ValueError, match="scope must be"):
        scaffolds.scaffold_store(Store(), vtables, dtables, scope=1)
    with pytest.raises(TypeError, match="ValenceTables"):
        scaffolds.scaffold_store(Store(), dtables, dtables)
    with pytest.raises(TypeError, match="DescriptorTables"):
        scaffolds.scaffold_store(Store(), vtables, vtables)
    with pytest.raises(ValueError, match="ValenceTables live on"):
        scaffolds.scaffold_store(Store(), vtables, dtables)

    class Tensor:
        is_cuda = True
    for kw in (dict(), dict(validity=vtables), dict(descriptors=dtables)):
        with pytest.raises(ValueError, match="needs validity="):
            MoleculeSampler(None, Tensor(), Tensor(), graph=False, scaffolds=True, **kw)

    # the record: one packed buffer and the derived batch; cpu() keeps both
    size = scaffolds.MoleculeScaffolds.layout(3, 5, 2)[1]
    rec = scaffolds.MoleculeScaffolds(torch.zeros(size, dtype=torch.uint8), 3, 5, 2, MoleculeBatch.empty(3, 5, 2, False, "cpu"))
    assert isinstance(rec, PackedRecord) and len(rec) == 3 and rec.mol.shape == (3, 16) and rec.mol.dtype == torch.int32
    assert rec.ring_hist.shape == (3, 8) and rec.atom_role.shape == rec.atom_system.shape == (3, 5) and rec.bond_ring_size.shape == (3, 2)
    assert rec.atom_role.dtype == torch.uint8 and scaffolds.MoleculeScaffolds.layout(3, 5, 2)[0]["ring_hist"][0] == 192
    rec.mol[:] = torch.arange(48, dtype=torch.int32).view(3, 16)
    rec.batch.buffer.zero_()
    host_rec = rec.cpu()
    assert isinstance(host_rec.mol, np.ndarray) and host_rec.batch.is_host and host_rec.batch.atoms.shape == (3, 5) and host_rec.cpu() is host_rec
    for r in (rec, host_rec):
        for k, name in enumerate(ref.MOL_FIELDS):
            assert [int(x) for x in getattr(r, name)] == [k, 16 + k, 32 + k]
    for bad in (None, host_rec):
        with pytest.raises((TypeError, RuntimeError), match="MoleculeScaffolds"):
            scaffolds.ScaffoldStock.from_scaffolds(bad)
    with pytest.raises(TypeError, match="MoleculeScaffolds"):
        scaffolds.scaffold_similarity(np.zeros(3), None)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="min_rings"):
            scaffolds.ScaffoldStock.from_scaffolds(rec, min_rings=bad)
    with pytest.raises(ValueError, match="key_bits"):
        scaffolds.ScaffoldStock.from_scaffolds(rec, key_bits=65)
    with pytest.raises(TypeError, match="ScaffoldStock"):
        scaffolds.scaffold_similarity(rec, None)
    text = scaffolds.__doc__
    assert "NOT RDKit's bit for bit" in text and "No SSSR" in text and "Kekule" in text and "has not been" in text
