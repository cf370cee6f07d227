"""Host side of the descriptors (csrc/mol_desc.hip, druggen_amd/descriptors.py): the plain-Python restatement
(tests/mol_desc_ref.py) against results derived by hand and against the hand-worked fixture rows, its invariance under atom
order; the fifth public header against its ctypes table, every argument refusal of the C entry -- all of which return before a
launch -- the tables `DescriptorTables.from_decoders` makes, the host checks of descriptors.py and its record, and the key
packing and table search of csrc/mol_env.h run on the host.  No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_desc_ref as ref
import mol_fp_ref as fref
import mol_valid_ref as vref
from test_mol_valid_host import _kind, fixture_molecules, from_smiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -1, -2      # DG_E_SHAPE, DG_E_ARG of include/druggen_hip.h


def _describe(smiles):
    atoms, rows = from_smiles(smiles)
    valid = vref.validity(atoms, rows)
    return valid, ref.describe(atoms, rows, valid)


def _fields(result):
    return dict(zip(ref.DESC_FIELDS, result["desc"]))


# ---- 1. results derived by hand ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smiles,want", [
    # aspirin: OH 2023 + two O= 2 x 1707 + the ester O(-)- 923 = 6360; CH3-C ends in a methyl, C-O(ester), O-aryl and
    # aryl-C(acid) turn: 3; C-OH ends in the OH; one benzene ring
    ("CC(=O)Oc1ccccc1C(=O)O", dict(status=0, n_heavy=13, tpsa=6360, n_rot=3, n_rings=1, n_ring_atoms=6, n_aromatic_atoms=6,
                                   n_carbon=9, n_sp3_carbon=1, n_untyped=0)),
    # paracetamol: O= 1707 + NH 1203 + OH 2023 = 4933; C-N and N-aryl turn (the simple pattern keeps the amide bond): 2
    ("CC(=O)Nc1ccc(O)cc1", dict(status=0, tpsa=4933, n_rot=2, n_rings=1, n_carbon=8, n_sp3_carbon=1)),
    # caffeine: three n(-)(:): 3 x 493 + one n(:): 1289 + two O= 2 x 1707 = 1479 + 1289 + 3414 = 6182; the methyls have degree 1
    ("Cn1cnc2c1c(=O)n(C)c(=O)n2C", dict(status=0, tpsa=6182, n_rot=0, n_rings=2, n_ring_atoms=9, n_aromatic_atoms=9,
                                        n_sp3_carbon=3)),
    ("C1CN1", dict(status=0, tpsa=2194, n_rings=1, n_rot=0, n_ring_atoms=3)),      # aziridine: [NH](-)- in a three-ring
    ("C1CO1", dict(status=0, tpsa=1253, n_rings=1)),                                # oxirane: O(-)- in a three-ring
    ("CC#N", dict(status=0, tpsa=2379, n_rot=0, n_sp3_carbon=1)),                   # acetonitrile: N#
    ("CC#CC", dict(status=0, n_rot=0, n_carbon=4, n_sp3_carbon=2)),                 # but-2-yne: no bond between atoms of degree 2
    ("CCC#CCC", dict(status=0, n_rot=0)),                                           # hex-3-yne: CH2-C has a triple bond at one end
    ("c1ccccc1-c1ccccc1", dict(status=0, n_rot=1, n_rings=2, n_ring_atoms=12)),     # biphenyl
    ("C1CCCCC1", dict(status=0, n_rot=0, n_sp3_carbon=6, n_rings=1)),               # cyclohexane
    ("N", dict(status=0, n_untyped=1, tpsa=0, n_heavy=1)),                          # ammonia: (h 3, no bond) has no row
    ("O", dict(status=0, n_untyped=1, tpsa=0)),                                     # water
    ("NCCO", dict(status=0, tpsa=4625, n_rot=1)),                                   # NH2 2602 + OH 2023; only C-C turns
    ("CCCC", dict(status=0, n_rot=1, n_rings=0)),                                   # butane: the middle bond
    ("CN(C)C", dict(status=0, tpsa=324, n_rot=0)),                                  # N(-)(-)-
    ("CC=NC", dict(status=0, tpsa=1236, n_rot=0)),                                  # N(-)=: N-CH3 ends in a methyl
    ("CC=N", dict(status=0, tpsa=2385)),                                            # [NH]=
    ("c1ccncc1", dict(status=0, tpsa=1289, n_aromatic_atoms=6)),                    # pyridine
    ("c1ccoc1", dict(status=0, tpsa=1314)),                                         # furan
    ("C1CC1C1CC1", dict(status=0, n_rot=1, n_rings=2, n_ring_atoms=6)),             # a bridge between two rings
    ("c1cccc1", dict(status=5, n_heavy=0, n_rot=0, tpsa=0, n_rings=0)),             # not kekulisable: a row of zeros
    ("C:C", dict(status=4, n_heavy=0)),                                             # an aromatic bridge: never a valid molecule
])
def test_hand_derived_results(smiles, want):
    _, got = _describe(smiles)
    got = _fields(got)
    assert {k: got[k] for k in want} == want, got


def test_keys_and_bond_classes_by_hand():
    # ethanol C C O: rows (1, 0) and (2, 1); C: h 3, one single; C: h 2, two singles; O: h 1, one single
    valid, got = _describe("CCO")
    assert got["keys"] == [1 | 3 << 8 | 1 << 12, 1 | 2 << 8 | 2 << 12, 3 | 1 << 8 | 1 << 12] and got["classes"] == [1, 1]
    # aziridine: every atom in the triangle, every bond a ring bond
    _, got = _describe("C1CN1")
    assert got["keys"] == [1 | 2 << 8 | 2 << 12 | 1 << 24] * 2 + [2 | 1 << 8 | 2 << 12 | 1 << 24] and got["classes"] == [3, 3, 3]
    # toluene c1ccccc1C: six aromatic ring bonds and a bridge that ends in a methyl; the substituted c has one single bond
    _, got = _describe("c1ccccc1C")
    assert got["classes"] == [3] * 6 + [1] and got["keys"][5] == 1 | 0 << 8 | 1 << 12 | 2 << 21 and got["keys"][0] == 1 | 1 << 8 | 2 << 21
    # acetonitrile: n3 sits at bit 19; propene CC=C: n2 at bit 16
    assert _describe("CC#N")[1]["keys"][2] == 2 | 1 << 19 and _describe("CC=C")[1]["keys"][1] == 1 | 1 << 8 | 1 << 12 | 1 << 16
    # butane: the middle bond is rotatable; outside the scope and for an invalid molecule: no key, no class
    assert _describe("CCCC")[1]["classes"] == [1, 5, 1]
    valid = vref.validity([1, 0, 1, 0], [(2, 0, 1)])
    got = ref.describe([1, 0, 1, 0], [(2, 0, 1)], valid)
    assert got["keys"] == [1 | 3 << 8 | 1 << 12, ref.NO_KEY, 1 | 3 << 8 | 1 << 12, ref.NO_KEY] and got["desc"][:2] == [0, 2]
    _, got = _describe("c1cccc1")
    assert got["keys"] == [ref.NO_KEY] * 5 and got["classes"] == [0] * 5 and got["desc"] == [5] + [0] * 11


def test_every_field_of_the_key_fits_under_the_valence_bound():
    """h + n1 + 2 n2 + 3 n3 + na <= 8: the largest value of each field alone stays inside its bits; na = 8 reaches bit 24 and
    still meets no other reachable key."""
    seen = {}
    for h in range(9):
        for n1 in range(9 - h):
            for n2 in range((8 - h - n1) // 2 + 1):
                for n3 in range((8 - h - n1 - 2 * n2) // 3 + 1):
                    for na in range(8 - h - n1 - 2 * n2 - 3 * n3 + 1):
                        for r3 in ((0, 1) if n1 + n2 + n3 + na >= 2 else (0,)):
                            key = ref.key_of(5, h, n1, n2, n3, na, r3)
                            assert key >> 25 == 0 and key & 255 == 5
                            if na < 8:
                                assert ((key >> 8) & 15, (key >> 12) & 15, (key >> 16) & 7, (key >> 19) & 3, (key >> 21) & 7,
                                        key >> 24) == (h, n1, n2, n3, na, r3)
                                assert seen.setdefault(key, (h, n1, n2, n3, na, r3)) == (h, n1, n2, n3, na, r3)
                            else:      # the r3 bit is lost: both variants share the key, nobody else has it
                                assert key == 5 | 1 << 24 and seen.setdefault(key, "na 8") == "na 8"
    assert len(seen) > 300


def test_no_graph_truncated_lists_and_flags():
    atoms, rows = from_smiles("CCCC")
    valid = vref.validity(atoms, rows)
    assert ref.describe(atoms, rows, valid, n_bonds=3, cap=2) == dict(desc=[-2] + [0] * 11, keys=[ref.NO_KEY] * 4, classes=[0, 0])
    assert ref.describe(atoms, rows, valid, flag=-1)["desc"][0] == -2
    assert ref.describe(atoms, rows, valid, n_bonds=3, cap=3)["desc"][:3] == [0, 4, 1]
    assert ref.describe(atoms, rows, valid, n_bonds=3, cap=0)["classes"] == []


# ---- 2. the fixture molecules ------------------------------------------------------------------------------------------------------
def fixture_tables():
    """The fixture molecules and, under their decoders, the host rows of the validity and descriptor tables as the keyword
    arguments the two restatements take."""
    from druggen_amd import descriptors, validity
    strings, atoms, labels, atom_dec, bond_dec = fixture_molecules()
    atom_rows, bond_rows = validity.table_rows(atom_dec, bond_dec)
    tables = descriptors.DescriptorTables.from_decoders(atom_dec, bond_dec, "cpu")
    vtab = dict(atom_rows=atom_rows.tolist(), bond_rows=bond_rows.tolist())
    dtab = dict(bond_rows=tables.bond_rows.tolist(), atom_flags=tables.atom_flag_rows.tolist(),
                atom_class=tables.atom_class_rows.tolist(), env=ref.env_for(atom_dec))
    assert {int(k): int(v) for k, v in tables.env_rows} == dtab["env"]
    return strings, atoms, labels, atom_dec, bond_dec, vtab, dtab


def golden_rows():
    with open(os.path.join(ROOT, "tests", "golden", "chembl_like_descriptors.json")) as f:
        return json.load(f)


def test_fixture_molecules_have_their_hand_worked_rows():
    """tests/golden/chembl_like_descriptors.json: the eight molecules of chembl_like_validity.json, every row worked by hand in
    its comment; both scopes (the molecules are connected)."""
    strings, atoms, labels, _, _, vtab, dtab = fixture_tables()
    golden = golden_rows()
    assert [g["smiles"] for g in golden] == strings and all(g["comment"] for g in golden)
    assert dtab["bond_rows"] == vtab["bond_rows"] and dtab["atom_flags"] == [r[2] for r in vtab["atom_rows"]]
    for b, g in enumerate(golden):
        m = dref.decode_labels(atoms[b], labels[b])
        for scope in (ref.WHOLE, ref.LARGEST):
            kw = dict(scope=scope, component=m["component"], largest=m["largest"])
            valid = vref.validity(m["atoms"], m["bonds"], **vtab, **kw)
            got = ref.describe(m["atoms"], m["bonds"], valid, **dtab, **kw)
            assert {k: v for k, v in _fields(got).items() if not k.startswith("reserved")} == {k: g[k] for k in ref.DESC_FIELDS[:10]}, b
            assert (ref.veber_rules(got["desc"]), ref.lipinski_rules(valid["mol"], got["desc"])) == (g["veber"], g["lipinski"]), b
    assert [g["status"] for g in golden] == [0] * 7 + [5]


# ---- 3. invariance under atom order ---------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_atom_order():
    rng = np.random.default_rng(330)
    valid_seen = rot = tri = 0
    for k in range(40):
        atoms, labels = vref.aromatic_like(rng, int(rng.integers(2, 31)), k % 4 != 3)
        if k % 5 == 0 and len(atoms) >= 3:      # the first three atoms become a three-ring of their own (scope: whole)
            atoms[:3], labels[:3], labels[:, :3] = (1, 2, 3)[k % 3], 0, 0
            labels[1, 0] = labels[2, 0] = labels[2, 1] = 1
        m = dref.decode_labels(atoms, labels)
        base = ref.describe(m["atoms"], m["bonds"], vref.validity(m["atoms"], m["bonds"]))
        valid_seen += base["desc"][0] == 0
        rot += base["desc"][2] > 0
        tri += any(key != ref.NO_KEY and key >> 24 for key in base["keys"])
        for _ in range(10):
            a2, l2, perm = vref.renumbered(rng, atoms, labels)
            m2 = dref.decode_labels(a2, l2)
            got = ref.describe(m2["atoms"], m2["bonds"], vref.validity(m2["atoms"], m2["bonds"]))
            assert got["desc"] == base["desc"] and got["keys"] == [base["keys"][p] for p in perm], k
            assert sorted(got["classes"]) == sorted(base["classes"])
    assert valid_seen >= 10 and rot >= 5 and tri >= 2


# ---- 4. the fifth header against the fifth table -----------------------------------------------------------------------------------
def test_desc_header_matches_its_ctypes_table_parameter_by_parameter():
    from druggen_amd import _lib, build, descriptors
    named = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
             ctypes.c_double: "double", ctypes.c_char_p: "pointer", ctypes.c_void_p: "pointer"}
    path = os.path.join(ROOT, "include", "druggen_hip_desc.h")
    assert os.path.abspath(build.DESC_HEADER) == path and path not in [os.path.abspath(h) for h in build.HEADERS]
    header = open(path).read()
    assert re.search(r'^#include "druggen_hip_valid.h"', header, flags=re.M)
    macro = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"^#define\s+(DG_DESC_[A-Z_]+)\s+\(?(-?\w+)\)?", header, flags=re.M)}
    assert macro == {"DG_DESC_FIELDS": len(ref.DESC_FIELDS), "DG_DESC_MAX_ENV": ref.MAX_ENV, "DG_DESC_NO_KEY": ref.NO_KEY,
                     "DG_DESC_BOND": ref.BOND, "DG_DESC_RING_BOND": ref.RING_BOND, "DG_DESC_ROTATABLE": ref.ROTATABLE}
    assert (descriptors.DESC_FIELDS, descriptors.NO_KEY, descriptors.MAX_ENV) == (ref.DESC_FIELDS, ref.NO_KEY, ref.MAX_ENV)
    assert (descriptors.BOND, descriptors.RING_BOND, descriptors.ROTATABLE) == (1, 2, 4)
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    header = re.sub(r"^\s*#.*$", " ", header, flags=re.M)
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header)
    names = [name for _, name, _ in protos]
    assert names == list(_lib.DESC_SIGNATURES) == ["dg_mol_descriptors"]
    for table in (_lib.SIGNATURES, _lib.TEXT_SIGNATURES, _lib.FP_SIGNATURES, _lib.VALID_SIGNATURES):
        assert not set(names) & set(table)
    for other in ("druggen_hip.h", "druggen_hip_text.h", "druggen_hip_fp.h", "druggen_hip_valid.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(rf"\b{name}\s*\(", text) for name in names), other
    lib = _lib.load()
    for ret, name, params in protos:
        res, args = _lib.DESC_SIGNATURES[name]
        want = [_kind(ret)] + [_kind(p) for p in params.split(",")]
        assert want == [named[res]] + [named[a] for a in args], (name, want)
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, name
    assert lib.dg_version() == 232


# ---- 5. every refusal of the C entry ---------------------------------------------------------------------------------------
_buf = (ctypes.c_int64 * 8)()
P = ctypes.addressof(_buf)      # a non-null, 8-byte aligned pointer: no call below gets as far as reading it


def test_entry_argument_checks():
    """None of these calls launches, and B == 0 returns 0 without one."""
    from druggen_amd import _lib
    lib = _lib.load()
    names = ("atoms", "bonds", "n_bonds", "component", "largest", "flags", "mol", "hcount", "bond_table", "atom_flags",
             "atom_class", "env_table", "desc", "atom_key", "bond_class")

    def call(B=3, N=9, cap=36, scope=1, n_atom_labels=7, n_bond_labels=5, n_env=26, **ptrs):
        p = {n: P for n in names}
        p.update(ptrs)
        return lib.dg_mol_descriptors(p["atoms"], p["bonds"], p["n_bonds"], p["component"], p["largest"], p["flags"], p["mol"],
                                      p["hcount"], p["bond_table"], n_bond_labels, p["atom_flags"], p["atom_class"],
                                      n_atom_labels, p["env_table"], n_env, B, N, cap, scope, p["desc"], p["atom_key"],
                                      p["bond_class"], None)

    def err():
        return lib.dg_last_error_string()
    for kw in (dict(B=-1), dict(N=0), dict(N=257), dict(N=-4), dict(N=1 << 20), dict(cap=-1), dict(n_atom_labels=0),
               dict(n_atom_labels=256), dict(n_bond_labels=0), dict(n_bond_labels=257), dict(n_env=-1), dict(n_env=4097)):
        assert call(**kw) == SHAPE and b"dg_mol_descriptors: need B >= 0, 1 <= N <= 256" in err(), kw
    for scope in (-1, 2, 3, 256):
        assert call(scope=scope) == ARG and b"scope must be 0 (whole) or 1 (largest)" in err(), scope
    for name in ("atoms", "n_bonds", "mol", "hcount", "bond_table", "atom_flags", "atom_class", "desc", "atom_key", "bonds",
                 "bond_class", "component", "largest", "env_table"):
        assert call(**{name: None}) == ARG and b"dg_mol_descriptors: null pointer" in err(), name
    for name in ("bonds", "n_bonds", "largest", "flags", "mol", "bond_table", "atom_flags", "atom_class", "env_table", "desc",
                 "atom_key"):
        assert call(**{name: P + 2}) == ARG and b"aligned" in err(), name
    # the shape comes first, then the scope, then the pointers
    assert call(N=257, scope=5, atoms=None) == SHAPE and call(scope=5, atoms=None) == ARG and b"scope" in err()
    # an empty batch is no launch; the optional pointers may be null, B == 0 still checks the rest; every legal extreme passes
    assert call(B=0) == 0 and call(B=0, flags=None) == 0 and call(B=0, cap=0, bonds=None, bond_class=None) == 0
    assert call(B=0, scope=0, component=None, largest=None) == 0 and call(B=0, hcount=P + 1, atoms=P + 1, bond_class=P + 3) == 0
    assert call(B=0, n_env=0, env_table=None) == 0 and call(B=0, n_env=4096) == 0
    assert call(B=0, N=256, cap=32640, n_atom_labels=255, n_bond_labels=256) == 0
    assert call(B=0, N=1, cap=0, n_atom_labels=1, n_bond_labels=1, n_env=0) == 0
    assert call(B=0, scope=1, component=None) == ARG and call(B=0, desc=None) == ARG and call(B=0, scope=2) == ARG


# ---- 6. descriptors.py ---------------------------------------------------------------------------------------------------------------
def test_tables_from_decoders():
    from druggen_amd import descriptors, validity
    tables = descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    assert tables.atom_class_rows.tolist() == ref.ATOM_CLASS and tables.atom_flag_rows.tolist() == ref.ATOM_FLAGS
    assert tables.bond_rows.tolist() == ref.BOND_ROWS == validity.table_rows(fref.ATOM_DECODER, fref.BOND_DECODER)[1].tolist()
    # the issue's table, expanded over the labels of N and O and over r3: 11 + 5 patterns, of which 6 name their r3
    env = {int(k): int(v) for k, v in tables.env_rows}
    assert env == ref.ENV and len(env) == 2 * 16 - 6 == tables.n_env
    keys = tables.env_rows[:, 0]
    assert (keys[1:] > keys[:-1]).all() and tables.env_rows.dtype == np.uint32
    assert env[ref.key_of(2, 1, 2, 0, 0, 0, 0)] == 1203 and env[ref.key_of(2, 1, 2, 0, 0, 0, 1)] == 2194
    assert env[ref.key_of(3, 1, 1, 0, 0, 0, 0)] == env[ref.key_of(3, 1, 1, 0, 0, 0, 1)] == 2023
    assert (tables.n_atom_labels, tables.n_bond_labels) == (7, 5) and tables.env.shape == (26, 4) and tables.bonds.shape == (5,)
    assert tables.env[:, 2:].eq(0).all() and tables.env[:, 0].numpy().view(np.uint32).tolist() == keys.tolist()
    assert descriptors.env_key(2, 1, 2, 0, 0, 0, 1) == ref.key_of(2, 1, 2, 0, 0, 0, 1)
    # an element under two labels gets every row twice; an element no pattern names gets none
    twice = descriptors.DescriptorTables.from_decoders({0: 0, 1: 8, 2: 6, 3: 8}, fref.BOND_DECODER, "cpu")
    assert twice.n_env == 2 * (2 * 5 - 2) and {int(k) & 255 for k in twice.env_rows[:, 0]} == {1, 3}
    assert twice.atom_class_rows.tolist() == [0, 0, 1, 0] and twice.atom_flag_rows.tolist() == [0, 1, 0, 1]
    assert descriptors.DescriptorTables.from_decoders({0: 0, 1: 6}, fref.BOND_DECODER, "cpu").n_env == 0
    # tpsa=: the user's patterns replace the table
    own = descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu", tpsa=[(16, 0, 2, 0, 0, 0, None, 2530),
                                                                                                         (8, 1, 1, 0, 0, 0, 0, 5)])
    assert own.env_rows.tolist() == sorted([[ref.key_of(4, 0, 2, 0, 0, 0, 0), 2530], [ref.key_of(4, 0, 2, 0, 0, 0, 1), 2530],
                                            [ref.key_of(3, 1, 1, 0, 0, 0, 0), 5]])
    # ... and is refused when two rows reach one key, when a field leaves its range, and, as ready (key, value) rows, when
    # the keys are not strictly ascending
    for bad in ([(8, 1, 1, 0, 0, 0, None, 5), (8, 1, 1, 0, 0, 0, 1, 6)], [(7, 0, 0, 0, 1, 0, 0, 1)] * 2):
        with pytest.raises(ValueError, match="reached twice"):
            descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu", tpsa=bad)
    for bad in ((7, 9, 0, 0, 0, 0, 0, 1), (7, 0, 0, 5, 0, 0, 0, 1), (7, 0, 0, 0, 3, 0, 0, 1), (7, 0, 0, 0, 0, 8, 0, 1),
                (7, 0, 0, 0, 0, 0, 2, 1), (7, 0, 0, 0, 0, 0, 0, 1 << 23), (7, 0, 0, 0, 0, 0, 0, -1), (7, 0, 0)):
        with pytest.raises(ValueError, match="tpsa= row"):
            descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu", tpsa=[bad])
    ready = np.array([[5, 1], [9, 2], [700, 3]], dtype=np.uint32)
    assert descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu", tpsa=ready).env_rows.tolist() == ready.tolist()
    for bad in (ready[::-1], ready[[0, 2, 1]], ready[[0, 1, 1, 2]]):      # descending, unsorted, a key twice
        with pytest.raises(ValueError, match="strictly ascending"):
            descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu", tpsa=bad)
        with pytest.raises(ValueError, match="strictly ascending"):
            descriptors.DescriptorTables(ref.ATOM_CLASS, ref.ATOM_FLAGS, ref.BOND_ROWS, bad, "cpu")
    many = np.stack([np.arange(4097), np.ones(4097)], axis=1).astype(np.uint32)
    assert descriptors.DescriptorTables(ref.ATOM_CLASS, ref.ATOM_FLAGS, ref.BOND_ROWS, many[:4096], "cpu").n_env == 4096
    with pytest.raises(ValueError, match="at most 4096"):
        descriptors.DescriptorTables(ref.ATOM_CLASS, ref.ATOM_FLAGS, ref.BOND_ROWS, many, "cpu")
    with pytest.raises(ValueError, match="one word per atom label"):
        descriptors.DescriptorTables(ref.ATOM_CLASS, ref.ATOM_FLAGS[:3], ref.BOND_ROWS, ready, "cpu")
    # the decoders are checked like those of the other tables
    for bad in ({}, {1: 6}, {0: 0, 2: 6}):
        with pytest.raises(ValueError, match="labels 0..n-1"):
            descriptors.DescriptorTables.from_decoders(bad, fref.BOND_DECODER, "cpu")
    with pytest.raises(ValueError, match="bond type"):
        descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, {0: 0, 1: 4}, "cpu")


def test_python_refusals_and_the_record_without_a_gpu():
    """descriptors.py refuses host batches, other sources, other tables, a bad scope, a validity record that is not this batch's
    and out= -- all before any launch; the sampler refuses descriptors= without validity=; the record is one packed buffer
    whose columns are views, and the rule counts work on both sides."""
    import torch
    from druggen_amd import descriptors, validity
    from druggen_amd._packed import PackedRecord
    from druggen_amd.decode import MoleculeBatch, _layout
    from druggen_amd.sampling import MoleculeSampler
    tables = descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    vtables = validity.ValenceTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    host = MoleculeBatch(np.zeros(_layout(2, 3, 3, False)[1], dtype=np.uint8), 2, 3, 3, False)
    checked = validity.MoleculeValidity.empty(2, 3, 3, "cpu")
    assert host.descriptors is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        descriptors.describe_molecules(host, checked, tables)
    with pytest.raises(TypeError, match="MoleculeBatch"):
        descriptors.describe_molecules(np.zeros(4), checked, tables)

    class Device:      # stands in for a device buffer: the checks below come before anything touches it
        is_cuda, device = True, "cuda:0"
    host.is_host, host.buffer = False, Device()
    with pytest.raises(ValueError, match="scope must be"):
        descriptors.describe_molecules(host, checked, tables, scope="fragment")
    with pytest.raises(TypeError, match="DescriptorTables"):
        descriptors.describe_molecules(host, checked, vtables)
    with pytest.raises(ValueError, match="the tables live on cpu"):
        descriptors.describe_molecules(host, checked, tables)
    tables.device = "cuda:0"
    for bad in (None, np.zeros(3), checked, checked.cpu(), validity.MoleculeValidity.empty(3, 3, 3, "cpu")):
        with pytest.raises(ValueError, match="validity="):      # not a record; on another device; a host record; another B
            descriptors.describe_molecules(host, bad, tables)

    class Store:
        device, vertexes = "cuda:0", 3

        def __len__(self):
            return 2
    for bad in (0, -3):
        with pytest.raises(ValueError, match="chunk"):
            descriptors.descriptor_store(Store(), vtables, tables, chunk=bad)
    with pytest.raises(ValueError, match="scope must be"):
        descriptors.descriptor_store(Store(), vtables, tables, scope=1)
    with pytest.raises(TypeError, match="ValenceTables"):
        descriptors.descriptor_store(Store(), tables, tables)
    with pytest.raises(TypeError, match="DescriptorTables"):
        descriptors.descriptor_store(Store(), vtables, None)
    with pytest.raises(ValueError, match="valence tables live on"):
        descriptors.descriptor_store(Store(), vtables, tables)

    class Tensor:
        is_cuda = True
    with pytest.raises(TypeError, match="DescriptorTables"):
        MoleculeSampler(None, Tensor(), Tensor(), graph=False, validity=vtables, descriptors=vtables)
    with pytest.raises(ValueError, match="needs validity="):
        MoleculeSampler(None, Tensor(), Tensor(), graph=False, descriptors=tables)

    size = descriptors.MoleculeDescriptors.layout(3, 5, 2)[1]
    rec = descriptors.MoleculeDescriptors(torch.zeros(size, dtype=torch.uint8), 3, 5, 2)
    assert isinstance(rec, PackedRecord) and len(rec) == 3 and rec.desc.shape == (3, 12) and rec.desc.dtype == torch.int32
    assert rec.atom_key.shape == (3, 5) and rec.atom_key.dtype == torch.int32 and rec.bond_class.shape == (3, 2)
    assert rec.bond_class.dtype == torch.uint8 and descriptors.MoleculeDescriptors.layout(3, 5, 2)[0]["atom_key"][0] == 144
    rec.desc[:] = torch.tensor([[0, 13, 3, 6360, 0, 1, 6, 6, 9, 1, 0, 0], [0, 40, 11, 14001, 1, 0, 0, 0, 30, 30, 0, 0],
                                [5] + [0] * 11], dtype=torch.int32)
    val = validity.MoleculeValidity(torch.zeros(validity.MoleculeValidity.layout(3, 5, 2)[1], dtype=torch.uint8), 3, 5, 2)
    val.mol[:] = torch.tensor([[0, 13, 0, 0, 8, 1800420, 1, 4], [0, 40, 0, 0, 60, 5000000, 6, 11], [5, 5, 0, 1, 0, 0, 0, 0]],
                              dtype=torch.int32)
    host_rec, host_val = rec.cpu(), val.cpu()
    for r, v in ((rec, val), (host_rec, host_val)):
        assert [int(x) for x in r.status] == [0, 0, 5] and [int(x) for x in r.n_rot] == [3, 11, 0]
        assert [float(x) for x in r.tpsa_A2] == [63.6, 140.01, 0.0]
        assert [int(x) for x in r.veber_rules] == [2, 0, 0] and [int(x) for x in descriptors.veber_rules(r)] == [2, 0, 0]
        assert [int(x) for x in r.lipinski_rules(v)] == [4, 0, 0] and [int(x) for x in descriptors.lipinski_rules(v, r)] == [4, 0, 0]
        for k, name in enumerate(ref.DESC_FIELDS[:10]):
            assert [int(x) for x in getattr(r, name)] == [int(x) for x in r.desc[:, k]]
    assert isinstance(host_rec.desc, np.ndarray) and host_rec.tpsa_A2.dtype == np.float64 and rec.tpsa_A2.dtype == torch.float64
    with pytest.raises(ValueError, match="both on the device or"):
        descriptors.lipinski_rules(host_val, rec)
    text = descriptors.lipinski_rules.__doc__
    assert "logP" in text and "MISSING" in text and "N / O counts" in text


# ---- 7. csrc/mol_env.h on the host --------------------------------------------------------------------------------------------------
def test_the_key_packing_and_table_search_on_the_host(tmp_path):
    """csrc/mol_env.h is plain C++: tests/mol_env_harness.cpp runs the kernel's key packing and binary search on tables of 0, 1,
    2, 3, 26, 4095 and 4096 rows, asking for every key, for its neighbours on both sides, and for 0 and 0xFFFFFFFF."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "mol_env_harness")
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=",
                           os.path.join(ROOT, "tests", "mol_env_harness.cpp"), "-o", exe])
    rng = np.random.default_rng(9)
    cases, text = [], []
    for n in (0, 1, 2, 3, 26, 4095, 4096):
        keys = sorted(ref.ENV) if n == 26 else sorted(rng.choice(1 << 25, n, replace=False).tolist())
        if n >= 2:
            keys[0], keys[-1] = 0, 0xFFFFFFFF
            keys = sorted(set(keys))
            assert len(keys) == n
        asked = sorted({q for k in keys for q in (k - 1, k, k + 1) if 0 <= q <= 0xFFFFFFFF} | {0, 1, 0xFFFFFFFF, 1 << 24})
        cases.append((keys, asked))
        text.append(f"{len(keys)} {len(asked)}\n{' '.join(map(str, keys))}\n{' '.join(map(str, asked))}\n")
    packs = [(5, 3, 1, 0, 0, 0, 0), (254, 8, 0, 0, 0, 0, 0), (1, 0, 8, 0, 0, 0, 1), (2, 0, 0, 4, 0, 0, 1), (2, 0, 2, 0, 2, 0, 0),
             (3, 1, 0, 0, 0, 7, 1), (3, 0, 0, 0, 0, 8, 0), (3, 0, 0, 0, 0, 8, 1)]
    text.append(f"-1 {len(packs)}\n" + "".join(" ".join(map(str, p)) + "\n" for p in packs))
    out = subprocess.run([exe], input="".join(text), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases) + len(packs)
    for (keys, asked), line in zip(cases, out):
        got = list(map(int, line.split()))
        where = {k: i for i, k in enumerate(keys)}
        want = [x for q in asked for x in ((where[q], 7 * where[q] + 1) if q in where else (-1, 0))]
        assert got == want, len(keys)
    assert [int(l) for l in out[len(cases):]] == [ref.key_of(*p) for p in packs]
    assert int(out[-1]) == int(out[-2]) == 3 | 1 << 24
