"""Host side of the validity check (csrc/mol_valid.hip, druggen_amd/validity.py): the plain-Python restatement
(tests/mol_valid_ref.py) against results derived by hand, the fixture molecules against their recorded statuses, invariance
under atom order and the families whose deficiency is known by construction; the fourth public header against its ctypes
table, every argument refusal of the C entry -- all of which return before a launch -- and the host checks of validity.py.
No GPU."""
import csv
import ctypes
import json
import os
import re

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_fp_ref as fref
import mol_valid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -1, -2      # DG_E_SHAPE, DG_E_ARG of include/druggen_hip.h
ATOM_LABEL = {z: l for l, z in fref.ATOM_DECODER.items()}
BOND_LABEL = {t: l for l, t in fref.BOND_DECODER.items()}


def from_smiles(s):
    """(atom labels, bond rows (hi, lo, label)) of a SMILES string, by the project's own parser (which drops hydrogens and
    charges: the decoded graph carries none)."""
    from druggen_amd import smiles
    z, _, bonds = smiles.parse_smiles(s)
    return [ATOM_LABEL[a] for a in z], [(max(i, j), min(i, j), BOND_LABEL[t]) for i, j, t in bonds]


def _fields(result):
    return dict(zip(ref.MOL_FIELDS, result["mol"]))


# ---- 1. results derived by hand --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smiles,want", [
    ("c1ccccc1", dict(status=0, n_atoms=6, n_h=6, mass=780468, deficiency=0)),      # 6 C + 6 H
    ("c1ccncc1", dict(status=0, n_h=5, n_acceptors=1, n_donors=0)),          # N: sigma 2 < 3, a candidate, no H left
    ("c1ccoc1", dict(status=0, n_h=4, n_acceptors=1, n_donors=0)),           # O: 2 -> 2, no candidate; the four C pair up
    ("c1ccsc1", dict(status=0, n_h=4, n_acceptors=0)),                       # S: the smallest allowed valence >= 2 is 2
    ("c1ccc2ccccc2c1", dict(status=0, n_h=8, n_atoms=10)),                   # naphthalene
    ("c1ccc2cccc2cc1", dict(status=0, n_h=8, n_atoms=10)),                   # azulene: a five- and a seven-ring, both odd
    ("c1cc[nH]c1", dict(status=5, deficiency=1, n_h=0, mass=0)),             # the graph has no H: five candidates in a ring
    ("C1=CNC=C1", dict(status=0, n_h=5, n_donors=1, n_acceptors=1)),         # the same ring with its bonds drawn
    ("C:C", dict(status=4, deficiency=-1, n_over=0)),                        # an aromatic bond that is a bridge
    ("c1ccccc1:c1ccccc1", dict(status=4)),                                   # ... between two rings
    ("C(C)(C)(C)(C)C", dict(status=3, n_over=1, deficiency=-1)),             # five bonds at a carbon
    ("CS(=O)(=O)C", dict(status=0, n_h=6, n_acceptors=2, n_donors=0)),       # S: sigma 6 -> 6
    ("CS(=O)C", dict(status=0, n_h=6)),                                      # S: sigma 4 -> 4
    ("CCO", dict(status=0, n_h=6, n_donors=1, n_acceptors=1, mass=460417)),  # 2 C + O + 6 H
    ("C", dict(status=0, n_atoms=1, n_h=4, mass=160312)),                    # a lone atom: methane
    ("N(=O)=O", dict(status=3, n_over=1)),                                   # a nitro group without charges: N at 4
    ("c1ccccc1C", dict(status=0, n_h=8)),                                    # toluene: the substituted C is still a candidate
    ("C1=CC=CC=C1", dict(status=0, n_h=6, mass=780468)),                     # benzene with its bonds drawn
    ("c1cccc1", dict(status=5, deficiency=1)),                               # an odd carbon ring
    ("C#N", dict(status=0, n_h=1, n_donors=0, n_acceptors=1)),
])
def test_hand_derived_results(smiles, want):
    atoms, rows = from_smiles(smiles)
    got = _fields(ref.validity(atoms, rows))
    assert {k: got[k] for k in want} == want, got


def test_hydrogens_per_atom_and_the_sulfur_valences():
    atoms, rows = from_smiles("CS(=O)(=O)C")
    r = ref.validity(atoms, rows)
    assert r["hcount"] == [3, 0, 0, 0, 3] and r["w0"][1] == 6 and not r["candidates"]
    r = ref.validity(*from_smiles("c1ccsc1"))
    assert r["hcount"] == [1, 1, 1, 0, 1] and r["candidates"] == {0, 1, 2, 4}
    r = ref.validity(*from_smiles("CCO"))
    assert r["hcount"] == [3, 2, 1]
    # outside the scope: 0xFF; any status but 0: 0xFF everywhere
    r = ref.validity([1, 0, 1, 0], [(2, 0, 1)])
    assert r["mol"][:2] == [0, 2] and r["hcount"] == [3, 0xFF, 3, 0xFF]
    assert ref.validity(*from_smiles("C:C"))["hcount"] == [0xFF, 0xFF]


def test_all_pads_empty_lists_and_molecules_without_a_graph():
    pads = np.zeros(4, dtype=np.int64)
    assert ref.validity(pads, [])["mol"] == [ref.EMPTY, 0, 0, -1, 0, 0, 0, 0]
    m = dref.decode_labels(pads, dref.empty_graph(4))      # under `largest` the scope is the pad of component 0: no table row
    assert ref.validity(m["atoms"], m["bonds"], scope=ref.LARGEST, component=m["component"], largest=m["largest"])["mol"][:2] == [2, 1]
    atoms, rows = from_smiles("CCCC")
    blank = [ref.NO_GRAPH, 0, 0, -1, 0, 0, 0, 0]
    assert ref.validity(atoms, rows[:2], n_bonds=3, cap=2)["mol"] == blank
    assert ref.validity(atoms, rows, flag=-2)["mol"] == blank
    assert ref.validity(atoms, rows, n_bonds=3, cap=3)["mol"][:5] == [0, 4, 0, 0, 10]
    assert ref.validity(atoms, rows, n_bonds=-5, cap=3)["mol"][:5] == [0, 4, 0, 0, 16]      # a negative count reads no row


def test_unknown_labels_and_rows_outside_the_scope():
    assert ref.validity([1, 7], [(1, 0, 1)])["mol"][0] == ref.UNKNOWN_LABEL       # no atom row
    assert ref.validity([1, 0], [(1, 0, 1)])["mol"][0] == ref.UNKNOWN_LABEL       # a bonded pad: an empty row
    assert ref.validity([1, 1], [(1, 0, 5)])["mol"][0] == ref.UNKNOWN_LABEL       # no bond row
    assert ref.validity([1, 1], [(1, 0, 0)])["mol"][0] == ref.UNKNOWN_LABEL       # order 0
    # unknown comes before over-valent; rows that leave the scope, loops and ends >= N do not count
    assert ref.validity([1, 1, 1, 1, 1, 1, 0], [(k, 0, 1) for k in range(1, 7)])["mol"][:3] == [2, 7, 0]
    assert ref.validity([1, 1], [(1, 0, 1), (1, 1, 9), (200, 0, 9), (0, 9, 9)])["mol"][:2] == [0, 2]
    nine = [(0, 0, 0, 0), (4 | 9 << 8, 120000, 0, 0)]
    assert ref.validity([1, 1], [(1, 0, 1)], atom_rows=nine)["mol"][0] == ref.UNKNOWN_LABEL      # a valence byte of 9
    for word in (0, 4, 1 | 2 << 8, 2 | 1 << 8, 1 | 1 << 9):
        assert ref.bond_row(word) is None, word
    assert ref.bond_row(3) == (3, 0) and ref.bond_row(0x101) == (1, 1)
    assert ref.allowed_valences(ref.S_VALENCES) == [2, 4, 6] and ref.allowed_valences(0) is None
    assert ref.allowed_valences(3 | 0 << 8 | 5 << 16) == [3]      # zero-terminated


# ---- 2. the fixture molecules ------------------------------------------------------------------------------------------------------
def fixture_molecules():
    """(strings, atom label arrays, dense bond label arrays, decoders) of tests/golden/chembl_like_smiles.csv."""
    from druggen_amd import smiles
    with open(os.path.join(ROOT, "tests", "golden", "chembl_like_smiles.csv")) as f:
        strings = [r["SMILES"] for r in csv.DictReader(line for line in f if not line.startswith("#"))]
    atom_enc, atom_dec, bond_enc, bond_dec, kept, N = smiles.build_encoders(strings, 64)
    assert kept == strings and len(strings) == 8
    atoms, labels = np.zeros((8, N), dtype=np.int64), np.zeros((8, N, N), dtype=np.int64)
    for b, s in enumerate(strings):
        z, _, bonds = smiles.parse_smiles(s)
        atoms[b, :len(z)] = [atom_enc[a] for a in z]
        for i, j, t in bonds:
            labels[b, max(i, j), min(i, j)] = bond_enc[t]
    return strings, atoms, labels, atom_dec, bond_dec


def test_fixture_molecules_have_their_recorded_statuses():
    """Every molecule of the fixture list under the decoders `smiles.build_encoders` gives it and the tables
    `validity.table_rows` makes of them, against tests/golden/chembl_like_validity.json (recorded from the restatement; the
    comment of each row that is not valid derives it by hand)."""
    from druggen_amd import validity
    strings, atoms, labels, atom_dec, bond_dec = fixture_molecules()
    atom_rows, bond_rows = validity.table_rows(atom_dec, bond_dec)
    with open(os.path.join(ROOT, "tests", "golden", "chembl_like_validity.json")) as f:
        golden = json.load(f)
    assert [g["smiles"] for g in golden] == strings
    for b, g in enumerate(golden):
        m = dref.decode_labels(atoms[b], labels[b])
        for scope in (ref.WHOLE, ref.LARGEST):
            got = _fields(ref.validity(m["atoms"], m["bonds"], atom_rows=atom_rows.tolist(), bond_rows=bond_rows.tolist(),
                                       scope=scope, component=m["component"], largest=m["largest"]))
            assert {k: got[k] for k in ("status", "n_atoms", "deficiency", "n_h")} == {k: g[k] for k in ("status", "n_atoms", "deficiency", "n_h")}, (b, got)
        assert g["status"] == 0 or g["comment"]
    assert sum(g["status"] == 0 for g in golden) >= 6


# ---- 3. invariance under atom order ---------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_atom_order():
    rng = np.random.default_rng(328)
    seen = set()
    for k in range(50):
        atoms, labels = ref.aromatic_like(rng, int(rng.integers(2, 31)), k % 2 == 0)
        m = dref.decode_labels(atoms, labels)
        base = ref.validity(m["atoms"], m["bonds"])
        seen.add(base["mol"][0])
        for _ in range(20):
            a2, l2, perm = ref.renumbered(rng, atoms, labels)
            m2 = dref.decode_labels(a2, l2)
            got = ref.validity(m2["atoms"], m2["bonds"])
            assert got["mol"] == base["mol"] and got["hcount"] == [base["hcount"][p] for p in perm], k
    assert {0, 5} <= seen and len(seen) >= 4


# ---- 4. families whose deficiency is known by construction -----------------------------------------------------------------------
def test_families_agree_with_their_derivation():
    """The families the GPU tests run at N = 255 / 256, where the restatement refuses, here at sizes it accepts: the
    derivation (mol_valid_ref.fused_chain) against the exhaustive matching."""
    for sizes in ([5], [6], [7], [5, 5], [5, 7], [7, 5, 7], [5, 7, 5, 7], [6, 6, 6, 5], [5, 6, 6, 6, 7], [6, 6, 5], [7, 7, 7]):
        n = ref.chain_atoms(sizes)
        atoms, labels, used = ref.fused_chain(sizes, n + 2)
        assert used == n
        for shift in range(0, n + 2, 3):
            m = dref.decode_labels(*ref.rotated(atoms, labels, shift))
            got = _fields(ref.validity(m["atoms"], m["bonds"]))
            assert (got["status"], got["n_atoms"], got["deficiency"]) == ((5, n, 1) if n % 2 else (0, n, 0)), (sizes, shift, got)
            assert got["n_h"] == (0 if n % 2 else n - 2 * (len(sizes) - 1))      # one H per atom but the fusion atoms
    atoms, labels, used = ref.disjoint([[5], [7], [5, 5], [5]], 30)
    m = dref.decode_labels(atoms, labels)
    got = _fields(ref.validity(m["atoms"], m["bonds"]))
    assert (got["status"], got["n_atoms"], got["deficiency"]) == (5, 25, 3)
    got = _fields(ref.validity(m["atoms"], m["bonds"], scope=ref.LARGEST, component=m["component"], largest=m["largest"]))
    assert (got["status"], got["n_atoms"], got["deficiency"]) == (0, 8, 0)          # the two fused five-rings
    with pytest.raises(ValueError, match="stops at 24"):
        m = dref.decode_labels(*ref.fused_chain([6] * 6, 26)[:2])
        ref.validity(m["atoms"], m["bonds"])


def test_the_certificate_check_catches_wrong_rows():
    atoms, rows = from_smiles("c1ccccc1C")
    want = ref.validity(atoms, rows)
    assert [r[:2] for r in rows] == [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (5, 0), (6, 5)]
    good = [r + (order,) for r, order in zip(rows, (2, 1, 2, 1, 2, 1, 1))]
    ref.check_certificate(want, rows, good)
    for k, order in ((0, 1), (1, 2), (6, 2), (6, 0), (3, 3)):
        bad = list(good)
        bad[k] = rows[k] + (order,)
        with pytest.raises(AssertionError):
            ref.check_certificate(want, rows, bad)
    with pytest.raises(AssertionError):
        ref.check_certificate(ref.validity(*from_smiles("c1cccc1")), from_smiles("c1cccc1")[1], [r + (1,) for r in from_smiles("c1cccc1")[1]])


# ---- 5. the fourth header against the fourth table ------------------------------------------------------------------------------
def _kind(decl):
    decl = re.sub(r"\bconst\b", " ", decl).strip()
    if "*" in decl or re.match(r"dg_stream_t\b", decl):
        return "pointer"
    kind = decl.split()[0]
    assert kind in ("int", "int64_t", "size_t", "float", "double"), decl
    return kind


def test_valid_header_matches_its_ctypes_table_parameter_by_parameter():
    from druggen_amd import _lib, build, validity
    named = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
             ctypes.c_double: "double", ctypes.c_char_p: "pointer", ctypes.c_void_p: "pointer"}
    path = os.path.join(ROOT, "include", "druggen_hip_valid.h")
    assert path in [os.path.abspath(h) for h in build.HEADERS] and len(build.HEADERS) == 4
    header = open(path).read()
    assert re.search(r'^#include "druggen_hip.h"', header, flags=re.M)
    macro = {k: int(v) for k, v in re.findall(r"^#define\s+(DG_VALID_[A-Z_]+)\s+\(?(-?\d+)\)?", header, flags=re.M)}
    assert macro == {"DG_VALID_OK": ref.VALID, "DG_VALID_NO_GRAPH": ref.NO_GRAPH, "DG_VALID_EMPTY": ref.EMPTY,
                     "DG_VALID_UNKNOWN_LABEL": ref.UNKNOWN_LABEL, "DG_VALID_OVER_VALENT": ref.OVER_VALENT,
                     "DG_VALID_AROMATIC_NOT_IN_RING": ref.AROMATIC_NOT_IN_RING, "DG_VALID_NOT_KEKULISABLE": ref.NOT_KEKULISABLE,
                     "DG_VALID_MOL_FIELDS": len(ref.MOL_FIELDS)}
    assert (validity.VALID, validity.NO_GRAPH, validity.EMPTY, validity.UNKNOWN_LABEL, validity.OVER_VALENT,
            validity.AROMATIC_NOT_IN_RING, validity.NOT_KEKULISABLE) == (0, -2, 1, 2, 3, 4, 5)
    assert sorted(validity.STATUS) == [-2, 0, 1, 2, 3, 4, 5] and validity.MOL_FIELDS == ref.MOL_FIELDS
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    header = re.sub(r"^\s*#.*$", " ", header, flags=re.M)
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header)
    names = [name for _, name, _ in protos]
    assert names == list(_lib.VALID_SIGNATURES) == ["dg_mol_validity"]
    for table in (_lib.SIGNATURES, _lib.TEXT_SIGNATURES, _lib.FP_SIGNATURES):
        assert not set(names) & set(table)
    for other in ("druggen_hip.h", "druggen_hip_text.h", "druggen_hip_fp.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(rf"\b{name}\s*\(", text) for name in names), other
    lib = _lib.load()
    for ret, name, params in protos:
        res, args = _lib.VALID_SIGNATURES[name]
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
    names = ("atoms", "bonds", "n_bonds", "component", "largest", "flags", "atom_table", "bond_table", "mol", "hcount", "kekule")

    def call(B=3, N=9, cap=36, scope=1, h_mass=10078, n_atom_labels=7, n_bond_labels=5, **ptrs):
        p = {n: P for n in names}
        p.update(ptrs)
        return lib.dg_mol_validity(p["atoms"], p["bonds"], p["n_bonds"], p["component"], p["largest"], p["flags"],
                                   p["atom_table"], n_atom_labels, p["bond_table"], n_bond_labels, B, N, cap, scope, h_mass,
                                   p["mol"], p["hcount"], p["kekule"], None)

    def err():
        return lib.dg_last_error_string()
    for kw in (dict(B=-1), dict(N=0), dict(N=257), dict(N=-4), dict(N=1 << 20), dict(cap=-1), dict(n_atom_labels=0),
               dict(n_atom_labels=256), dict(n_bond_labels=0), dict(n_bond_labels=257)):
        assert call(**kw) == SHAPE and b"dg_mol_validity: need B >= 0, 1 <= N <= 256" in err(), kw
    for scope in (-1, 2, 3, 256):
        assert call(scope=scope) == ARG and b"scope must be 0 (whole) or 1 (largest)" in err(), scope
    assert call(h_mass=-1) == ARG and b"h_mass" in err()
    for name in ("atoms", "n_bonds", "atom_table", "bond_table", "mol", "hcount", "bonds", "kekule", "component", "largest"):
        assert call(**{name: None}) == ARG and b"dg_mol_validity: null pointer" in err(), name
    for name in ("bonds", "n_bonds", "largest", "flags", "atom_table", "bond_table", "mol", "kekule"):
        assert call(**{name: P + 2}) == ARG and b"aligned" in err(), name
    # the shape comes first, then the scope, then the pointers
    assert call(N=257, scope=5, atoms=None) == SHAPE and call(scope=5, atoms=None) == ARG and b"scope" in err()
    assert call(scope=5, h_mass=-1) == ARG and b"scope" in err() and call(h_mass=-1, atoms=None) == ARG and b"h_mass" in err()
    # an empty batch is no launch; the optional pointers may be null, B == 0 still checks the rest; every legal extreme passes
    assert call(B=0) == 0 and call(B=0, flags=None) == 0 and call(B=0, cap=0, bonds=None, kekule=None) == 0
    assert call(B=0, scope=0, component=None, largest=None) == 0 and call(B=0, hcount=P + 1) == 0
    assert call(B=0, N=256, cap=32640, h_mass=0x7FFFFFFF, n_atom_labels=255, n_bond_labels=256) == 0
    assert call(B=0, N=1, cap=0, h_mass=0, n_atom_labels=1, n_bond_labels=1) == 0
    assert call(B=0, scope=1, component=None) == ARG and call(B=0, mol=None) == ARG and call(B=0, scope=2) == ARG


# ---- 7. validity.py ----------------------------------------------------------------------------------------------------------------
def test_tables_from_decoders():
    from druggen_amd import validity
    atom_rows, bond_rows = validity.table_rows(fref.ATOM_DECODER, fref.BOND_DECODER)
    assert [tuple(r) for r in atom_rows.tolist()] == ref.ATOM_ROWS and atom_rows.dtype == np.uint32
    assert bond_rows.tolist() == ref.BOND_ROWS and bond_rows.dtype == np.uint32
    every = {l: z for l, z in enumerate([0] + sorted(validity.VALENCES))}
    rows = validity.table_rows(every, fref.BOND_DECODER)[0].tolist()
    assert [r[1] for r in rows] == [0, 110093, 120000, 140031, 159949, 189984, 279769, 309738, 319721, 349689, 749216, 799165,
                                    789183, 1269045]
    assert [ref.allowed_valences(r[0]) for r in rows[1:]] == [[3], [4], [3], [2], [1], [4], [3, 5], [2, 4, 6], [1], [3, 5],
                                                              [2, 4, 6], [1], [1, 3, 5]]
    assert [r[2] for r in rows] == [0, 0, 0, 1, 1] + [0] * 9 and not any(r[3] for r in rows) and validity.H_MASS == ref.H_MASS
    with pytest.raises(ValueError, match="no valence row"):
        validity.table_rows({0: 0, 1: 26}, fref.BOND_DECODER)
    rows = validity.table_rows({0: 0, 1: 26}, fref.BOND_DECODER, valences={26: ((2, 3), 559349)})[0].tolist()
    assert rows[1] == [2 | 3 << 8, 559349, 0, 0]
    for bad in ({26: ((), 1)}, {26: ((9,), 1)}, {26: ((3, 2), 1)}, {26: ((1, 2, 3, 4, 5), 1)}, {26: ((2,), -1)}):
        with pytest.raises(ValueError, match="of atomic number 26"):
            validity.table_rows({0: 0, 1: 26}, fref.BOND_DECODER, valences=bad)
    for bad in ({0: 0, 1: 1}, {0: 0, 1: 55}, {0: 0, 1: -6}):
        with pytest.raises(ValueError, match="atomic number"):
            validity.table_rows(bad, fref.BOND_DECODER)
    with pytest.raises(ValueError, match="bond type"):
        validity.table_rows(fref.ATOM_DECODER, {0: 0, 1: 4})
    for bad in ({}, {1: 6}, {0: 0, 2: 6}):
        with pytest.raises(ValueError, match="labels 0..n-1"):
            validity.table_rows(bad, fref.BOND_DECODER)
    with pytest.raises(ValueError, match="256 labels"):
        validity.table_rows({l: 6 for l in range(256)}, fref.BOND_DECODER)
    tables = validity.ValenceTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    assert (tables.n_atom_labels, tables.n_bond_labels) == (7, 5) and tables.atoms.shape == (7, 4) and tables.bonds.shape == (5,)


def test_python_refusals_and_the_record_without_a_gpu():
    """validity.py refuses host batches, other sources, other tables, a bad scope and out= -- all before any launch; the record
    is one packed buffer whose columns are views."""
    import torch
    from druggen_amd import validity
    from druggen_amd._packed import PackedRecord
    from druggen_amd.decode import MoleculeBatch, _layout
    tables = validity.ValenceTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    host = MoleculeBatch(np.zeros(_layout(2, 3, 3, False)[1], dtype=np.uint8), 2, 3, 3, False)
    assert host.validity is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        validity.check_molecules(host, tables)
    with pytest.raises(TypeError, match="MoleculeBatch"):
        validity.check_molecules(np.zeros(4), tables)

    class Device:      # stands in for a device buffer: the checks below come before anything touches it
        is_cuda, device = True, "cuda:0"
    host.is_host, host.buffer = False, Device()
    with pytest.raises(ValueError, match="scope must be"):
        validity.check_molecules(host, tables, scope="fragment")
    with pytest.raises(TypeError, match="ValenceTables"):
        validity.check_molecules(host, (ref.ATOM_ROWS, ref.BOND_ROWS))
    with pytest.raises(ValueError, match="the tables live on cpu"):
        validity.check_molecules(host, tables)
    tables.device = "cuda:0"
    for out in (np.zeros(3), validity.MoleculeValidity.empty(2, 3, 3, "cpu"), validity.MoleculeValidity.empty(2, 3, 3, "cpu").cpu()):
        with pytest.raises(ValueError, match="out="):      # not a record; on another device; a host record
            validity.check_molecules(host, tables, out=out)

    class Store:
        device, vertexes = "cuda:0", 3

        def __len__(self):
            return 2
    for bad in (0, -3):
        with pytest.raises(ValueError, match="chunk"):
            validity.validity_store(Store(), tables, chunk=bad)
    with pytest.raises(ValueError, match="scope must be"):
        validity.validity_store(Store(), tables, scope=1)
    with pytest.raises(TypeError, match="ValenceTables"):
        validity.validity_store(Store(), None)

    rec = validity.MoleculeValidity(torch.arange(validity.MoleculeValidity.layout(3, 5, 2)[1], dtype=torch.uint8), 3, 5, 2)
    assert isinstance(rec, PackedRecord) and len(rec) == 3 and rec.mol.shape == (3, 8) and rec.mol.dtype == torch.int32
    assert rec.hcount.shape == (3, 5) and rec.kekule.shape == (3, 2, 4) and rec.hcount.dtype == torch.uint8
    rec.mol[:] = torch.tensor([[0, 4, 0, 0, 10, 580783, 0, 0], [5, 5, 0, 1, 0, 0, 0, 0], [-2, 0, 0, -1, 0, 0, 0, 0]], dtype=torch.int32)
    host_rec = rec.cpu()
    for r in (rec, host_rec):
        assert [int(v) for v in r.status] == [0, 5, -2] and [int(v) for v in r.deficiency] == [0, 1, -1]
        assert [int(v) for v in r.n_h] == [10, 0, 0] and [int(v) for v in r.mass] == [580783, 0, 0]
        assert [bool(v) for v in r.valid] == [True, False, False] and abs(float(r.valid_fraction()) - 1 / 3) < 1e-12
        for k, name in enumerate(ref.MOL_FIELDS):
            assert [int(v) for v in getattr(r, name)] == [int(v) for v in r.mol[:, k]]
    assert isinstance(host_rec.mol, np.ndarray)


# ---- 8. the matching of csrc/mol_match.h, run on the host --------------------------------------------------------------------------
def test_the_matching_header_on_the_host_equals_the_exhaustive_matching(tmp_path):
    """csrc/mol_match.h is plain C++ over pointers: tests/mol_match_harness.cpp runs it as the kernel's lane 0 does, here over
    random graphs of degree <= 7 with non-vertex slots in between, odd cycles, and fused ring chains.  The number of free vertices
    equals the exhaustive matching's, the mates form a matching of that size along edges, and the search state is left clean."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "mol_match_harness")
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=",
                           os.path.join(ROOT, "tests", "mol_match_harness.cpp"), "-o", exe])
    rng = np.random.default_rng(8)
    graphs = []
    for k in range(600):
        n = int(rng.integers(1, 21))
        slots = n + int(rng.integers(0, 4))
        where = sorted(rng.permutation(slots)[:n].tolist())
        edges, deg = set(), [0] * n
        for e in range(int(rng.integers(0, 2 * n + 2))):
            a, b = (e % n, (e + 1) % n) if k % 3 == 1 else rng.integers(0, n, 2).tolist()
            if a != b and (min(a, b), max(a, b)) not in edges and deg[a] < 7 and deg[b] < 7:
                edges.add((min(a, b), max(a, b)))
                deg[a] += 1
                deg[b] += 1
        graphs.append((slots, where, sorted(edges)))
    for sizes in ([5, 7, 5], [5, 7, 5, 7], [6, 6, 6, 5], [7, 5, 7, 5, 5], [3], [5, 5]):
        _, labels, used = ref.fused_chain(sizes, ref.chain_atoms(sizes))
        graphs.append((used, list(range(used)), [(int(j), int(i)) for i, j in np.argwhere(labels)]))
    text = []
    for slots, where, edges in graphs:
        flags = [0] * slots
        for v in where:
            flags[v] = 1
        text.append(f"{slots} {len(edges)}\n{' '.join(map(str, flags))}\n" + "".join(f"{where[a]} {where[b]}\n" for a, b in edges))
    out = subprocess.run([exe], input="".join(text), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(graphs)
    odd = 0
    for (slots, where, edges), line in zip(graphs, out):
        free_left, clean, *mates = map(int, line.split())
        n = len(where)
        want = n - 2 * ref.max_matching_size(set(range(n)), edges)
        assert clean == 1 and free_left == want, (slots, where, edges, line)
        real = {(where[a], where[b]) for a, b in edges}
        matched = [v for v in where if mates[v] >= 0]
        assert len(matched) == n - want and all(mates[mates[v]] == v and (min(v, mates[v]), max(v, mates[v])) in real for v in matched)
        assert all(mates[v] == -1 for v in range(slots) if v not in where)
        odd += want > 0
    assert 100 < odd < 500
