"""Host side of the substructure matcher (csrc/mol_sub.hip, csrc/mol_sub.h, druggen_amd/substructure.py): the plain-Python
restatement (tests/mol_sub_ref.py) against results derived by hand, the parser of the pattern grammar construct by construct and
refusal by refusal, the record packing round-tripped, the sixth public header against its ctypes table, every argument refusal
of the C entry -- all of which return before a launch -- the host checks of substructure.py and its record, the fixture
molecules against their recorded rows, and the search of csrc/mol_sub.h run on the host against the restatement, exact step
counts and OVER verdicts included.  No GPU.  Every comparison is `==`."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_desc_ref as descref
import mol_fp_ref as fref
import mol_sub_ref as ref
import mol_valid_ref as vref
from test_mol_desc_host import fixture_tables
from test_mol_valid_host import _kind, from_smiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -1, -2      # DG_E_SHAPE, DG_E_ARG of include/druggen_hip.h
LATTICE_SIDE = 6         # the smallest lattice on which a 10-atom dead-end chain is OVER from the centre (5: 3713 steps)


def make_tables(typing=(), patterns=(), atom_decoder=fref.ATOM_DECODER, bond_decoder=fref.BOND_DECODER, device="cpu"):
    from druggen_amd import substructure
    return substructure.SubstructureTables.from_decoders(atom_decoder, bond_decoder, device, typing=typing, patterns=patterns)


def table_args(tables):
    """The restatement's keyword arguments of a SubstructureTables."""
    return dict(patterns=tables.pattern_rows, bond_rows=tables.bond_rows.tolist(), atom_sets=tables.atom_set_rows.tolist())


def match_smiles(smiles, tables, steps=None):
    atoms, rows = from_smiles(smiles)
    described = descref.describe(atoms, rows, vref.validity(atoms, rows))
    return ref.match(atoms, rows, described, steps_out=steps, **table_args(tables))


def hits_of(smiles, text):
    got = match_smiles(smiles, make_tables(patterns=[("p", text)]))
    assert got["mol"][7] == 0
    return got["hits"][0]


def dead_end_chain(n, end="[N]"):
    """n - 1 wildcards and an atom that the molecules in question do not have (no lattice carbon is an N, nothing is uranium),
    joined by any bond: a full enumeration that never succeeds."""
    return "~".join(["[*]"] * (n - 1) + [end])


# ---- 1. results derived by hand ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smiles,text,want", [
    ("CCO", "[O]", 1), ("CCO", "[C]", 2), ("CCO", "[*]", 3), ("CCO", "[!C]", 1), ("CCO", "[#6,#8]", 3), ("CCO", "[S]", 0),      # one atom
    ("CCO", "[C;H3]", 1), ("CCO", "[C;H2,3]", 2), ("CCO", "[*;D1]", 2), ("CCO", "[O;H1]-[C]", 1), ("CCO", "[O;H0]", 0),
    # injectivity: a carbon with three DIFFERENT carbon neighbours -- propane's middle carbon has only two, isobutane's has three
    ("CCC", "[C]([C])([C])[C]", 0), ("CC(C)C", "[C]([C])([C])[C]", 1), ("CCC", "[C]([C])[C]", 1),
    # ... and a four-ring walks back to its first atom over a closure: a triangle has no fourth atom
    ("C1CC1", "[C]1[C][C][C]1", 0), ("C1CCC1", "[C]1[C][C][C]1", 4), ("C1CC1", "[C]1[C][C]1", 3),
    # a six-ring closure: benzene at all six atoms (anchors, not the twelve matches), an open chain of six nowhere
    ("c1ccccc1", "[C]1:[C]:[C]:[C]:[C]:[C]:1", 6), ("C=CC=CC=C", "[C]1~[C]~[C]~[C]~[C]~[C]~1", 0),
    ("c1ccccc1", "[C]1~[C]~[C]~[C]~[C]~[C]~1", 6), ("C=CC=CC=C", "[C]~[C]~[C]~[C]~[C]~[C]", 2),      # the chain: from its two ends
    # ring and chain bonds: methylcyclopropane has three ring carbons on a ring bond, and one chain bond with two ends
    ("CC1CC1", "[C]-@[C]", 3), ("CC1CC1", "[C]-!@[C]", 2), ("CC1CC1", "[C]~@[C]", 3), ("CC1CC1", "[C;R]", 3), ("CC1CC1", "[C;!R]", 1),
    ("CC1CC1", "[C;r3]", 3), ("C1CCC1", "[C;r3]", 0), ("C1CCC1", "[C;!r3;R]", 4),
    # bond kinds: an omitted bond is single or aromatic, never double
    ("CC=O", "[C][O]", 0), ("CC=O", "[C]=[O]", 1), ("CC=O", "[C]-,=[*]", 2), ("CC#N", "[C]#[N]", 1), ("CC#N", "[C;T1]", 1),
    ("c1ccccc1O", "[C;a][O]", 1), ("c1ccccc1O", "[C;a]:[C;a]", 6), ("c1ccccc1O", "[C;A]", 0), ("C=CC", "[C;Y1]", 2),
    # the anchor is the first atom: the amide carbon, once, however many ways the rest can be laid
    ("CC(=O)N", "[C;Y1](=[O])-[N]", 1), ("CC(=O)Nc1ccc(O)cc1", "[C;Y1](=[O])-[N]", 1), ("CC(=O)Oc1ccccc1C(=O)O", "[C;Y1](=[O])-[O;H1]", 1),
    ("CC(=O)Oc1ccccc1C(=O)O", "[C;Y1](=[O])-[O;H0]-[C]", 1),
])
def test_hand_derived_anchor_counts(smiles, text, want):
    assert hits_of(smiles, text) == want


def test_typing_is_first_match_in_table_order_with_the_hydrogen_term():
    # ethanol C C O, h = 3, 2, 1.  Row a takes CH3, row b every other carbon; the oxygen has no row
    tables = make_tables(typing=[("a", "[C;H3]", 10, 1), ("b", "[C]", 100, 0, 7, 2)])
    got = match_smiles("CCO", tables)
    assert got["types"] == [0, 1, -1] and got["hits"] == [1, 2]
    #             status heavy typed untyped sum0: (10 + 3 x 1) + (100 + 2 x 0), sum1: 0 + (7 + 2 x 2), patterns hit, over
    assert got["mol"] == [0, 3, 2, 1, 113, 11, 2, 0]
    # the other order: every carbon is a `b`
    got = match_smiles("CCO", make_tables(typing=[("b", "[C]", 100, 0, 7, 2), ("a", "[C;H3]", 10, 1)]))
    assert got["types"] == [0, 0, -1] and got["mol"] == [0, 3, 2, 1, 200, 7 + 3 * 2 + 7 + 2 * 2, 2, 0]
    # counted rows never type; negative values wrap modulo 2^32
    got = match_smiles("CCO", make_tables(typing=[("o", "[O]", -5, -3)], patterns=[("c", "[C]")]))
    assert got["types"] == [-1, -1, 0] and got["hits"] == [1, 2] and got["mol"] == [0, 3, 1, 2, (-8) & 0xFFFFFFFF, 0, 2, 0]


def test_a_status_other_than_valid_gives_the_blank_row():
    tables = make_tables(typing=[("c", "[C]", 1, 1)], patterns=[("any", "[*]")])
    assert match_smiles("c1cccc1", tables) == dict(mol=[5] + [0] * 7, hits=[0, 0], types=[-1] * 5)
    assert match_smiles("C:C", tables)["mol"] == [4] + [0] * 7
    # outside the scope: no anchor, no type
    atoms, rows = [1, 0, 1, 0], [(2, 0, 1)]
    described = descref.describe(atoms, rows, vref.validity(atoms, rows))
    got = ref.match(atoms, rows, described, **table_args(tables))
    assert got == dict(mol=[0, 2, 2, 0, 2 + 6, 0, 2, 0], hits=[2, 2], types=[0, -1, 0, -1])


def test_builtin_tables_on_small_molecules_by_hand():
    """The built-in rows over the test decoders (C, N, O, S, Cl, Se): aspirin and paracetamol, each atom typed by hand."""
    from druggen_amd import substructure
    tables = make_tables(typing=None, patterns=None)
    assert tables.names[:tables.n_typing] == tuple(r[0] for r in substructure.LOGP) and tables.n_patterns == 29 + 12
    name = {k: n for n, k in tables.index.items()}
    # aspirin CC(=O)Oc1ccccc1C(=O)O: CH3 on carbon `C`; the ester C=O `C.dbl.hetero`; =O; the ester O `O`; c-O `C.ar.hetero`;
    # four aromatic CH; c-C(=O) `C.ar.subst`; the acid C `C.dbl.hetero`; =O; the acid OH `O.acid`
    got = match_smiles("CC(=O)Oc1ccccc1C(=O)O", tables)
    want = ["C", "C.dbl.hetero", "O.carbonyl", "O", "C.ar.hetero", "C.ar", "C.ar", "C.ar", "C.ar", "C.ar.subst", "C.dbl.hetero",
            "O.carbonyl", "O.acid"]
    assert [name[t] for t in got["types"]] == want
    logp = (1441 + 3 * 1230) + 2 * -2783 + 2 * -3339 + -684 + 1129 + 4 * (1581 + 1230) + 1360 + (-2893 + 2980)
    assert got["mol"] == [0, 13, 13, 0, logp, 0, got["mol"][6], 0] and logp == 6023
    groups = {n: got["hits"][tables.index[n]] for n, _ in substructure.GROUPS}
    assert groups == dict(amide=0, ester=1, carboxylic_acid=1, nitrile=0, primary_amine=0, secondary_amine=0, tertiary_amine=0,
                          aryl_halide=0, alcohol=0, ether=0, ketone=0, enone=0)
    # paracetamol CC(=O)Nc1ccc(O)cc1: the NH sits on an aromatic carbon `N.aryl`; the phenol OH `O.hydroxyl`
    got = match_smiles("CC(=O)Nc1ccc(O)cc1", tables)
    assert [name[t] for t in got["types"]] == ["C", "C.dbl.hetero", "O.carbonyl", "N.aryl", "C.ar.hetero", "C.ar", "C.ar",
                                               "C.ar.hetero", "O.hydroxyl", "C.ar", "C.ar"]
    assert got["mol"][4] == (1441 + 3690) - 2783 - 3339 + (-5188 + 2142) + 2 * 1129 + 4 * 2811 + (-2893 - 2677)
    assert {n: got["hits"][tables.index[n]] for n in ("amide", "alcohol", "secondary_amine")} == dict(amide=1, alcohol=0, secondary_amine=0)
    # one of each amine, an aryl chloride, an ether, a ketone and an enone
    for smiles, group in (("CCN", "primary_amine"), ("CNC", "secondary_amine"), ("CN(C)C", "tertiary_amine"), ("Clc1ccccc1", "aryl_halide"),
                          ("CCO", "alcohol"), ("COC", "ether"), ("CC(=O)C", "ketone"), ("CC(=O)C=C", "enone"), ("CC#N", "nitrile")):
        got = match_smiles(smiles, tables)
        assert got["hits"][tables.index[group]] == 1 and got["mol"][3] == 0, (smiles, group)
    assert match_smiles("CC(=O)NC", tables)["hits"][tables.index["secondary_amine"]] == 0      # an amide nitrogen is no amine
    assert match_smiles("C[Se]C", tables)["mol"][2:4] == [2, 1]                                 # no row for Se: untyped


# ---- 2. the parser -------------------------------------------------------------------------------------------------------------------
def test_parser_reads_every_construct():
    from druggen_amd.substructure import parse_pattern
    full = dict(h=0x1FF, deg=0x1FF, n2=0x1F, n3=7, arom=3, ring=3, r3=3)

    def atom(text):
        a = parse_pattern(text).atoms[0]
        return {k: v for k, v in a.items() if k in ("elements", "negate") or full.get(k) != v}
    assert atom("[*]") == dict(elements=None, negate=False)
    assert atom("[C]") == dict(elements=frozenset({6}), negate=False)
    assert atom("[C,N,#16,Cl]") == dict(elements=frozenset({6, 7, 16, 17}), negate=False)
    assert atom("[!C,#8]") == dict(elements=frozenset({6, 8}), negate=True)
    assert atom("[H0]") == dict(elements=None, negate=False, h=1) and atom("[C;H1,3]")["h"] == 0b1010
    assert atom("[D2,3]")["deg"] == 0b1100 and atom("[Y0]")["n2"] == 1 and atom("[Y1,4]")["n2"] == 0b10010 and atom("[T2]")["n3"] == 4
    assert atom("[a]")["arom"] == 2 and atom("[A]")["arom"] == 1 and atom("[R]")["ring"] == 2 and atom("[!R]")["ring"] == 1
    assert atom("[r3]")["r3"] == 2 and atom("[!r3]")["r3"] == 1 and atom("[H8;D8]") == dict(elements=None, negate=False, h=256, deg=256)
    assert atom("[N;H1,2;D1;A;!R;!r3;Y0;T0]") == dict(elements=frozenset({7}), negate=False, h=6, deg=2, arom=1, ring=1, r3=1, n2=1, n3=1)
    assert atom("[H1;H1,2;a;A]") == dict(elements=None, negate=False, h=2, arom=0)      # constraints are a conjunction

    def bonds(text):
        p = parse_pattern(text)
        return [(a["parent"], a["bond"]) for a in p.atoms[1:]], p.closures
    assert bonds("[C][C]") == ([(0, 0x99)], []) and bonds("[C]-[C]") == ([(0, 0x11)], []) and bonds("[C]=[C]") == ([(0, 0x22)], [])
    assert bonds("[C]#[C]") == ([(0, 0x44)], []) and bonds("[C]:[C]") == ([(0, 0x88)], []) and bonds("[C]~[C]") == ([(0, 0xFF)], [])
    assert bonds("[C]-,=[C]") == ([(0, 0x33)], []) and bonds("[C]-,=,#,:[C]") == ([(0, 0xFF)], [])
    assert bonds("[C]-@[C]") == ([(0, 0x10)], []) and bonds("[C]-!@[C]") == ([(0, 0x01)], []) and bonds("[C]=,:@[C]") == ([(0, 0xA0)], [])
    assert bonds("[C]~!@[C]") == ([(0, 0x0F)], [])
    # branches: the parent is the atom before the bracket; the writing order is the preorder
    assert bonds("[C]([N])([O])[S]")[0] == [(0, 0x99)] * 3 and bonds("[C]([N][O])[S]")[0] == [(0, 0x99), (1, 0x99), (0, 0x99)]
    assert bonds("[C](=[N](-[O])[F])[S]")[0] == [(0, 0x22), (1, 0x11), (1, 0x99), (0, 0x99)]
    # ring closures: the bond is the second digit's and belongs to the later atom; sorted by that atom
    assert bonds("[C]1[C][C]1") == ([(0, 0x99), (1, 0x99)], [(2, 0, 0x99)]) and bonds("[C]1[C][C]=1")[1] == [(2, 0, 0x22)]
    assert bonds("[C]12[C]1[C]2")[1] == [(1, 0, 0x99), (2, 0, 0x99)] and bonds("[C]1[C]2[C]1[C]~@2")[1] == [(2, 0, 0x99), (3, 1, 0xF0)]
    assert bonds("[C]1[C][C]1[C]1[C][C]1")[1] == [(2, 0, 0x99), (5, 3, 0x99)]      # a digit is free again once closed
    p = parse_pattern("[C]1:[C]:[C]:[C]:[C]:[C]:1")
    assert len(p.atoms) == 6 and p.closures == [(5, 0, 0x88)] and [a["parent"] for a in p.atoms[1:]] == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("text,what", [
    ("C", "bracket atom"), ("[C]C", "bracket atom"), ("[C+]", "charge"), ("[N-]", "charge"), ("[NH3+]", "charge"),
    ("[$([C])]", "recursive"), ("[13C]", "isotope"), ("[C@@H]", "chirality"), ("[C@]", "chirality"), ("[C:1]", "atom map"),
    ("[C&H1]", "& operator"), ("[C^2]", "hybridisation"), ("[C].[C]", "disconnected"), ("[C]%10[C]%10", "%nn"),
    ("[C]/[C]", "directional"), ("[CH2]", "constraint 'CH2'"), ("[X2]", "constraint 'X2'"), ("[C;v4]", "constraint 'v4'"),
    ("[R2]", "constraint 'R2'"), ("[r5]", "constraint 'r5'"), ("[H]", "constraint 'H'"), ("[C;N]", "two element constraints"),
    ("[*;C]", "two element constraints"), ("[H9]", "go up to 8"), ("[D9]", "go up to 8"), ("[Y5]", "go up to 4"), ("[T3]", "go up to 2"),
    ("[H1,]", "comma list"), ("[]", "empty bracket"), ("[C;]", "empty constraint"), ("[C", "unclosed bracket"), ("[C]1[C]", "open branch, ring"),
    ("[C]([C]", "open branch, ring"), ("[C])", "unmatched"), ("[C]-", "open branch, ring"), ("[C]--[C]", "two bonds"),
    ("[C]-,[C]", "bond list"), ("[C]@[C]", "ring suffix"), ("[C]!@[C]", "ring suffix"), ("-[C]", "before the first atom"),
    ("[C]-1[C][C]1", "opening digit"), ("[C]0[C]0", "ring-closure digit"), ("1[C]", "ring-closure digit"), ("[C]11", "with itself"),
    ("([C])", "branch without an atom"), ("[C]-([C])", "branch without an atom"), ("", "non-empty string"), ("[Xx]", "constraint 'Xx'"),
    ("[#0]", "constraint '#0'"),
])
def test_parser_refuses_by_name(text, what):
    from druggen_amd.substructure import parse_pattern
    with pytest.raises(ValueError, match="unsupported") as err:
        parse_pattern(text)
    assert what in str(err.value), str(err.value)


def test_parser_limits_16_atoms_and_8_closures():
    from druggen_amd.substructure import parse_pattern
    assert len(parse_pattern("[C]" * 16).atoms) == 16
    with pytest.raises(ValueError, match="more than 16 atoms"):
        parse_pattern("[C]" * 17)
    eight = "[C]12345678" + "".join(f"[C]{d}" for d in range(1, 9))
    assert parse_pattern(eight).closures == [(k, 0, 0x99) for k in range(1, 9)]
    with pytest.raises(ValueError, match="more than 8 ring closures"):
        parse_pattern("[C]123456789" + "".join(f"[C]{d}" for d in range(1, 10)))


# ---- 3. the record -------------------------------------------------------------------------------------------------------------------
def test_the_record_round_trips_and_has_the_headers_layout():
    from druggen_amd import substructure as sub
    bits = {6: 0, 7: 1, 8: 2, 17: 3}
    text = "[C;a;D3]1(:[!C;H0,1]):[N,O;R]~@[*;Y1;T0;r3]=,#!@1"
    pattern = sub.parse_pattern(text)
    rec = sub.pack_pattern(pattern, bits, sub.TYPING, (5, -7, 1 << 30, -(1 << 31)))
    assert rec.dtype == np.uint32 and rec.shape == (80,) and not rec[5:8].any() and not rec[8 + 4 * 4:72].any() and not rec[73:].any()
    assert rec[0] == 4 | 1 << 8 | 1 << 16 and rec[1:5].tolist() == [5, (-7) & 0xFFFFFFFF, 1 << 30, 1 << 31]
    back = sub.unpack_pattern(rec)
    assert (back["n"], back["flags"], back["values"], back["closures"]) == (4, 1, (5, -7, 1 << 30, -(1 << 31)), [(3, 0, 0x06)])
    sets = [1, 0b1110, 0b0110, 0b1111]      # C; everything but C; N or O; any
    for k, (a, b) in enumerate(zip(pattern.atoms, back["atoms"])):
        assert b["sets"] == sets[k] and all(b[f] == a[f] for f in ("h", "deg", "n2", "n3", "arom", "ring", "r3")), k
        assert (b["parent"], b["bond"]) == ((a["parent"], a["bond"]) if k else (0, 0))
    # word by word, as the header lays it out
    assert rec[8:12].tolist() == [1, 0x1FF | 8 << 16, 0x1F | 7 << 8 | 2 << 12 | 3 << 14 | 3 << 16, 0]
    assert rec[12:16].tolist() == [0b1110, 3 | 0x1FF << 16, 0x1F | 7 << 8 | 3 << 12 | 3 << 14 | 3 << 16, 0 | 0x88 << 8]
    assert rec[16:20].tolist() == [0b0110, 0x1FF | 0x1FF << 16, 0x1F | 7 << 8 | 3 << 12 | 2 << 14 | 3 << 16, 0 | 0x88 << 8]
    assert rec[20:24].tolist() == [0b1111, 0x1FF | 0x1FF << 16, 2 | 1 << 8 | 3 << 12 | 3 << 14 | 2 << 16, 2 | 0xF0 << 8]
    assert rec[72] == 3 | 0 << 8 | 0x06 << 16
    # the restatement decodes the same record
    n, flags, values, atoms, closures = ref.decode_record(rec)
    assert (n, flags, values, closures) == (4, 1, [5, -7, 1 << 30, -(1 << 31)], [(3, 0, 6)])
    assert atoms[3] == (0b1111, 0x1FF, 0x1FF, 2, 1, 3, 3, 2, 2, 0xF0)
    # an element without a bit gives no set; a counted row has no flag and no value
    assert sub.pack_pattern(sub.parse_pattern("[S]"), bits)[8] == 0 and sub.pack_pattern(sub.parse_pattern("[!S]"), bits)[8] == 15
    assert sub.pack_pattern(sub.parse_pattern("[S]"), bits)[:5].tolist() == [1, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="int32"):
        sub.pack_pattern(pattern, bits, 1, (1 << 31, 0, 0, 0))


# ---- 4. the sixth header against the sixth table --------------------------------------------------------------------------------------
def test_sub_header_matches_its_ctypes_table_parameter_by_parameter():
    from druggen_amd import _lib, build, substructure
    named = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
             ctypes.c_double: "double", ctypes.c_char_p: "pointer", ctypes.c_void_p: "pointer"}
    path = os.path.join(ROOT, "include", "druggen_hip_sub.h")
    assert os.path.abspath(build.SUB_HEADER) == path and path not in [os.path.abspath(h) for h in build.HEADERS + [build.DESC_HEADER]]
    header = open(path).read()
    assert re.search(r'^#include "druggen_hip_desc.h"', header, flags=re.M)
    macro = {k: int(v) for k, v in re.findall(r"^#define\s+(DG_SUB_[A-Z_]+)\s+\(?(-?\d+)\)?", header, flags=re.M)}
    assert macro == {"DG_SUB_MOL_FIELDS": len(ref.MOL_FIELDS), "DG_SUB_MAX_ATOMS": ref.MAX_ATOMS, "DG_SUB_MAX_CLOSURES": ref.MAX_CLOSURES,
                     "DG_SUB_MAX_PATTERNS": ref.MAX_PATTERNS, "DG_SUB_MAX_STEPS": ref.MAX_STEPS, "DG_SUB_MAX_NEIGHBOURS": ref.MAX_NEIGHBOURS,
                     "DG_SUB_PATTERN_WORDS": ref.PATTERN_WORDS, "DG_SUB_TYPING": ref.TYPING}
    assert (substructure.MOL_FIELDS, substructure.MAX_ATOMS, substructure.MAX_CLOSURES, substructure.MAX_PATTERNS, substructure.MAX_STEPS,
            substructure.PATTERN_WORDS, substructure.TYPING) == (ref.MOL_FIELDS, 16, 8, 1024, 4096, 80, 1)
    assert ref.PATTERN_WORDS == 8 + 16 * 4 + 8
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    header = re.sub(r"^\s*#.*$", " ", header, flags=re.M)
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header)
    names = [name for _, name, _ in protos]
    assert names == list(_lib.SUB_SIGNATURES) == ["dg_mol_substructure"]
    for table in (_lib.SIGNATURES, _lib.TEXT_SIGNATURES, _lib.FP_SIGNATURES, _lib.VALID_SIGNATURES, _lib.DESC_SIGNATURES):
        assert not set(names) & set(table)
    for other in ("druggen_hip.h", "druggen_hip_text.h", "druggen_hip_fp.h", "druggen_hip_valid.h", "druggen_hip_desc.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(re.search(rf"\b{name}\s*\(", text) for name in names), other
    lib = _lib.load()
    for ret, name, params in protos:
        res, args = _lib.SUB_SIGNATURES[name]
        want = [_kind(ret)] + [_kind(p) for p in params.split(",")]
        assert want == [named[res]] + [named[a] for a in args], (name, want)
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, name
    assert lib.dg_version() == 232


# ---- 5. every refusal of the C entry ----------------------------------------------------------------------------------------------
_buf = (ctypes.c_int64 * 8)()
P = ctypes.addressof(_buf)      # a non-null, 8-byte aligned pointer: no call below gets as far as reading it


def test_entry_argument_checks():
    """None of these calls launches, and B == 0 returns 0 without one."""
    from druggen_amd import _lib
    lib = _lib.load()
    names = ("atoms", "bonds", "n_bonds", "desc", "atom_key", "bond_class", "bond_table", "atom_sets", "patterns", "mol", "hits",
             "atom_type")

    def call(B=3, N=9, cap=36, n_atom_labels=7, n_bond_labels=5, n_patterns=41, **ptrs):
        p = {n: P for n in names}
        p.update(ptrs)
        return lib.dg_mol_substructure(p["atoms"], p["bonds"], p["n_bonds"], p["desc"], p["atom_key"], p["bond_class"],
                                       p["bond_table"], n_bond_labels, p["atom_sets"], n_atom_labels, p["patterns"], n_patterns,
                                       B, N, cap, p["mol"], p["hits"], p["atom_type"], None)

    def err():
        return lib.dg_last_error_string()
    for kw in (dict(B=-1), dict(N=0), dict(N=257), dict(N=-4), dict(N=1 << 20), dict(cap=-1), dict(n_atom_labels=0),
               dict(n_atom_labels=256), dict(n_bond_labels=0), dict(n_bond_labels=257), dict(n_patterns=-1), dict(n_patterns=1025)):
        assert call(**kw) == SHAPE and b"dg_mol_substructure: need B >= 0, 1 <= N <= 256" in err(), kw
    for name in names:
        assert call(**{name: None}) == ARG and b"dg_mol_substructure: null pointer" in err(), name
    for name in ("bonds", "n_bonds", "desc", "atom_key", "bond_table", "atom_sets", "patterns", "mol", "hits", "atom_type"):
        assert call(**{name: P + 2}) == ARG and b"aligned" in err(), name
    # the shape comes first, then the pointers
    assert call(N=257, atoms=None) == SHAPE and call(atoms=None, mol=P + 2) == ARG and b"null pointer" in err()
    # an empty batch is no launch; the optional pointers may be null, B == 0 still checks the rest; every legal extreme passes
    assert call(B=0) == 0 and call(B=0, cap=0, bonds=None, bond_class=None) == 0
    assert call(B=0, n_patterns=0, patterns=None, hits=None) == 0 and call(B=0, atoms=P + 1, bond_class=P + 3) == 0
    assert call(B=0, N=256, cap=32640, n_atom_labels=255, n_bond_labels=256, n_patterns=1024) == 0
    assert call(B=0, N=1, cap=0, n_atom_labels=1, n_bond_labels=1, n_patterns=0) == 0
    assert call(B=0, patterns=None) == ARG and call(B=0, hits=None) == ARG and call(B=0, mol=None) == ARG
    assert call(B=0, cap=1, bond_class=None) == ARG and call(B=0, n_patterns=1025) == SHAPE


# ---- 6. substructure.py ------------------------------------------------------------------------------------------------------------
def test_tables_from_decoders():
    from druggen_amd import substructure as sub
    from druggen_amd import validity
    tables = make_tables(typing=None, patterns=None)
    assert tables.element_bits == {6: 0, 7: 1, 8: 2, 16: 3, 17: 4, 34: 5} and tables.atom_set_rows.tolist() == [0, 1, 2, 4, 8, 16, 32]
    assert tables.bond_rows.tolist() == validity.table_rows(fref.ATOM_DECODER, fref.BOND_DECODER)[1].tolist() == descref.BOND_ROWS
    assert (tables.n_patterns, tables.n_typing, tables.n_atom_labels, tables.n_bond_labels) == (41, 29, 7, 5)
    assert tables.names == tuple(r[0] for r in sub.LOGP + sub.GROUPS) and tables.index["amide"] == 29
    assert tables.patterns.shape == (41, 80) and tables.atom_sets.shape == (7,) and tables.pattern_rows.dtype == np.uint32
    assert ((tables.pattern_rows[:, 0] >> 16) & 1).tolist() == [1] * 29 + [0] * 12
    # typing rows come first, in the given order; counted rows follow; an element under two labels shares its bit
    own = make_tables(typing=[("x", "[O]", 1, 2), ("y", "[*]", 3, 4, 5, 6)], patterns=[("z", "[C][C]")], atom_decoder={0: 0, 1: 8, 2: 6, 3: 8})
    assert own.names == ("x", "y", "z") and own.atom_set_rows.tolist() == [0, 2, 1, 2] and own.n_typing == 2
    assert own.pattern_rows[:, :5].tolist() == [[1 | 1 << 16, 1, 2, 0, 0], [1 | 1 << 16, 3, 4, 5, 6], [2, 0, 0, 0, 0]]
    assert own.pattern_rows[:, 8].tolist() == [2, 3, 1]
    assert make_tables().n_patterns == 0 and make_tables().patterns.shape == (0, 80)
    # every built-in row parses, stays within 16 atoms, and every element of LOGP ends in a catch-all
    last = {}
    for name, text, *_ in sub.LOGP:
        p = sub.parse_pattern(text)
        last[tuple(sorted(p.atoms[0]["elements"]))] = (len(p.atoms), {k: v for k, v in p.atoms[0].items() if k not in ("elements", "negate")})
    full = dict(h=0x1FF, deg=0x1FF, n2=0x1F, n3=7, arom=3, ring=3, r3=3)
    assert sorted(last) == [(6,), (7,), (8,), (9,), (15,), (16,), (17,), (35,), (53,)] and all(v == (1, full) for v in last.values())
    assert len(sub.GROUPS) == 12 and "FROM MEMORY" in sub.__doc__ and "not been measured" in sub.__doc__ and "PAINS" in sub.__doc__
    # refusals: a name twice, too many patterns, too many elements, malformed rows, whatever the parser refuses
    with pytest.raises(ValueError, match="twice"):
        make_tables(typing=[("a", "[C]", 0, 0)], patterns=[("a", "[N]")])
    assert make_tables(patterns=[(f"p{k}", "[C]") for k in range(1024)]).n_patterns == 1024
    with pytest.raises(ValueError, match="at most 1024"):
        make_tables(typing=[("t", "[C]", 0, 0)], patterns=[(f"p{k}", "[C]") for k in range(1024)])
    with pytest.raises(ValueError, match="at most 1024"):
        sub.SubstructureTables([str(k) for k in range(1025)], np.zeros((1025, 80), dtype=np.uint32), [0, 1], [0, 1], "cpu")
    assert make_tables(atom_decoder={0: 0, **{k: k + 1 for k in range(1, 33)}}).atom_set_rows[32] == 1 << 31
    with pytest.raises(ValueError, match="33 distinct elements"):
        make_tables(atom_decoder={0: 0, **{k: k + 1 for k in range(1, 34)}})
    for bad in ([("a", "[C]")], [("a", "[C]", 1)], [("a", "[C]", 1, 2, 3)]):
        with pytest.raises(ValueError, match="typing= row"):
            make_tables(typing=bad)
    with pytest.raises(ValueError, match="patterns= row"):
        make_tables(patterns=[("a", "[C]", 1, 2)])
    with pytest.raises(ValueError, match="unsupported: a charge"):
        make_tables(patterns=[("a", "[N+]")])
    with pytest.raises(ValueError, match="labels 0..n-1"):
        make_tables(atom_decoder={1: 6})


def test_python_refusals_and_the_record_without_a_gpu():
    import torch
    from druggen_amd import descriptors, validity
    from druggen_amd import substructure as sub
    from druggen_amd._packed import PackedRecord
    from druggen_amd.decode import MoleculeBatch, _layout
    from druggen_amd.sampling import MoleculeSampler
    tables = make_tables(typing=None, patterns=None)
    dtables = descriptors.DescriptorTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    vtables = validity.ValenceTables.from_decoders(fref.ATOM_DECODER, fref.BOND_DECODER, "cpu")
    host = MoleculeBatch(np.zeros(_layout(2, 3, 3, False)[1], dtype=np.uint8), 2, 3, 3, False)
    described = descriptors.MoleculeDescriptors.empty(2, 3, 3, "cpu")
    assert host.matches is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sub.match_molecules(host, described, tables)
    with pytest.raises(TypeError, match="MoleculeBatch"):
        sub.match_molecules(np.zeros(4), described, tables)

    class Device:      # stands in for a device buffer: the checks below come before anything touches it
        is_cuda, device = True, "cuda:0"
    host.is_host, host.buffer = False, Device()
    with pytest.raises(TypeError, match="SubstructureTables"):
        sub.match_molecules(host, described, dtables)
    with pytest.raises(ValueError, match="the tables live on cpu"):
        sub.match_molecules(host, described, tables)
    tables.device = "cuda:0"
    for bad in (None, np.zeros(3), described, described.cpu(), descriptors.MoleculeDescriptors.empty(3, 3, 3, "cpu")):
        with pytest.raises(ValueError, match="descriptors="):
            sub.match_molecules(host, bad, tables)

    class Store:
        device, vertexes = "cuda:0", 3

        def __len__(self):
            return 2
    for bad in (0, -3):
        with pytest.raises(ValueError, match="chunk"):
            sub.match_store(Store(), vtables, dtables, tables, chunk=bad)
    with pytest.raises(ValueError, match="scope must be"):
        sub.match_store(Store(), vtables, dtables, tables, scope=1)
    with pytest.raises(TypeError, match="ValenceTables"):
        sub.match_store(Store(), dtables, dtables, tables)
    with pytest.raises(TypeError, match="SubstructureTables"):
        sub.match_store(Store(), vtables, dtables, None)
    with pytest.raises(ValueError, match="ValenceTables live on"):
        sub.match_store(Store(), vtables, dtables, tables)

    class Tensor:
        is_cuda = True
    with pytest.raises(TypeError, match="SubstructureTables"):
        MoleculeSampler(None, Tensor(), Tensor(), graph=False, validity=vtables, descriptors=dtables, substructures=dtables)
    for kw in (dict(), dict(validity=vtables)):
        with pytest.raises(ValueError, match="needs validity= and descriptors="):
            MoleculeSampler(None, Tensor(), Tensor(), graph=False, substructures=tables, **kw)

    size = sub.MoleculeMatches.layout(3, 5, 2)[1]
    rec = sub.MoleculeMatches(torch.zeros(size, dtype=torch.uint8), 3, 5, 2, names=("a", "b"))
    assert isinstance(rec, PackedRecord) and len(rec) == 3 and rec.mol.shape == (3, 8) and rec.mol.dtype == torch.int32
    assert rec.hits.shape == (3, 2) and rec.atom_type.shape == (3, 5) and sub.MoleculeMatches.layout(3, 5, 2)[0]["hits"][0] == 96
    assert sub.MoleculeMatches.layout(3, 5, 0)[0]["hits"][1] == 0
    #                          status heavy typed untyped sum0 sum1 hit over
    rec.mol[:] = torch.tensor([[0, 13, 13, 0, 9045, 0, 9, 0], [0, 40, 39, 1, 61234, 5, 3, 0], [5] + [0] * 7], dtype=torch.int32)
    rec.hits[:] = torch.tensor([[1, 0], [2, 7], [0, 0]], dtype=torch.int32)
    dsc = descriptors.MoleculeDescriptors(torch.zeros(descriptors.MoleculeDescriptors.layout(3, 5, 2)[1], dtype=torch.uint8), 3, 5, 2)
    dsc.desc[:] = torch.tensor([[0, 13, 3, 6360, 0, 1, 6, 6, 9, 1, 0, 0], [0, 40, 11, 14001, 1, 0, 0, 0, 30, 30, 0, 0], [5] + [0] * 11],
                               dtype=torch.int32)
    val = validity.MoleculeValidity(torch.zeros(validity.MoleculeValidity.layout(3, 5, 2)[1], dtype=torch.uint8), 3, 5, 2)
    val.mol[:] = torch.tensor([[0, 13, 0, 0, 8, 1800420, 1, 4], [0, 40, 0, 0, 60, 5000000, 6, 11], [5, 5, 0, 1, 0, 0, 0, 0]],
                              dtype=torch.int32)
    host_rec = rec.cpu()
    assert host_rec.names == ("a", "b") and isinstance(host_rec.mol, np.ndarray)
    for r, d, v in ((rec, dsc, val), (host_rec, dsc.cpu(), val.cpu())):
        assert [int(x) for x in r.count("b")] == [0, 7, 0] and [float(x) for x in r.logp] == [0.9045, 6.1234, 0.0]
        assert [int(x) for x in sub.lipinski_rules5(v, d, r)] == [5, 0, 0]
        assert [int(x) for x in descriptors.lipinski_rules(v, d)] == [4, 0, 0]
        for k, name in enumerate(ref.MOL_FIELDS):
            assert [int(x) for x in getattr(r, name)] == [int(x) for x in r.mol[:, k]]
        with pytest.raises(KeyError, match="no pattern is called"):
            r.count("c")
    assert host_rec.logp.dtype == np.float64 and rec.logp.dtype == torch.float64
    with pytest.raises(ValueError, match="all on the device or"):
        sub.lipinski_rules5(val.cpu(), dsc, rec)
    text = sub.lipinski_rules5.__doc__
    assert "walrus" in text and "lower bound" in text and "n_untyped == 0" in text and "MISSING" in descriptors.lipinski_rules.__doc__


@pytest.mark.parametrize("mol,want", [
    # (sum0, n_untyped, n_over) at and around the logP bounds: -2 and 5 count, an incomplete typing never does
    ((-20000, 0, 0), 5), ((-20001, 0, 0), 4), ((50000, 0, 0), 5), ((50001, 0, 0), 4), ((0, 1, 0), 4), ((0, 0, 1), 4),
])
def test_the_logp_rule_at_its_bounds(mol, want):
    from druggen_amd import descriptors, validity
    from druggen_amd import substructure as sub
    rec = sub.MoleculeMatches(np.zeros(sub.MoleculeMatches.layout(1, 2, 0)[1], dtype=np.uint8), 1, 2, 0)
    dsc = descriptors.MoleculeDescriptors(np.zeros(descriptors.MoleculeDescriptors.layout(1, 2, 1)[1], dtype=np.uint8), 1, 2, 1)
    val = validity.MoleculeValidity(np.zeros(validity.MoleculeValidity.layout(1, 2, 1)[1], dtype=np.uint8), 1, 2, 1)
    rec.mol[0] = [0, 2, 2 - mol[1], mol[1], mol[0], 0, 0, mol[2]]
    assert sub.lipinski_rules5(val, dsc, rec).tolist() == [want] == [ref.lipinski_rules5(val.mol[0].tolist(), dsc.desc[0].tolist(),
                                                                                           [int(x) & 0xFFFFFFFF for x in rec.mol[0]])]


# ---- 7. the fixture molecules ------------------------------------------------------------------------------------------------------
def fixture_sub_tables():
    """The fixture molecules, the built-in tables under their decoders, and the restatements' keyword arguments."""
    strings, atoms, labels, atom_dec, bond_dec, vtab, dtab = fixture_tables()
    tables = make_tables(typing=None, patterns=None, atom_decoder=atom_dec, bond_decoder=bond_dec)
    return strings, atoms, labels, atom_dec, bond_dec, vtab, dtab, tables


def golden_sub_rows():
    with open(os.path.join(ROOT, "tests", "golden", "chembl_like_substructure.json")) as f:
        return json.load(f)


def fixture_wanted(scope):
    strings, atoms, labels, _, _, vtab, dtab, tables = fixture_sub_tables()
    out = []
    for b in range(len(strings)):
        m = dref.decode_labels(atoms[b], labels[b])
        kw = dict(scope=scope, component=m["component"], largest=m["largest"])
        valid = vref.validity(m["atoms"], m["bonds"], **vtab, **kw)
        described = descref.describe(m["atoms"], m["bonds"], valid, **dtab, **kw)
        out.append((valid, described, ref.match(m["atoms"], m["bonds"], described, **table_args(tables))))
    return out


def test_fixture_molecules_have_their_recorded_rows():
    """tests/golden/chembl_like_substructure.json: the eight molecules of chembl_like_smiles.csv under the built-in LOGP and GROUPS
    tables; each row's comment tallies the types and sums their values from the table's own rows.  Every atom is typed and no
    search runs over; both scopes (the molecules are connected)."""
    from druggen_amd import substructure as sub
    strings, _, _, _, _, _, _, tables = fixture_sub_tables()
    golden = golden_sub_rows()
    assert [g["smiles"] for g in golden] == strings and all(g["comment"] for g in golden)
    values = {row[0]: row[2:4] for row in sub.LOGP}
    for scope in (descref.WHOLE, descref.LARGEST):
        for b, ((valid, described, got), g) in enumerate(zip(fixture_wanted(scope), golden)):
            mol = dict(zip(ref.MOL_FIELDS, got["mol"]))
            assert mol["status"] == g["status"] and mol["n_over"] == 0 and mol["n_untyped"] == 0, b
            if g["status"] != 0:
                assert got == ref.blank(g["status"], len(got["types"]), tables.n_patterns)
                continue
            signed = mol["sum0"] - (1 << 32) if mol["sum0"] >> 31 else mol["sum0"]
            assert (mol["n_heavy"], mol["n_typed"], signed) == (g["n_heavy"], g["n_heavy"], g["logp_1e4"]), b
            assert {n: got["hits"][tables.index[n]] for n, _ in sub.GROUPS} == g["groups"], b
            # the comment's tally: {type: [atoms, hydrogens on them]} adds up to the sum with the table's own values
            tally = g["types"]
            assert sum(n for n, _ in tally.values()) == g["n_heavy"]
            assert sum(n * values[t][0] + h * values[t][1] for t, (n, h) in tally.items()) == g["logp_1e4"], b
            assert {t: got["hits"][tables.index[t]] >= n for t, (n, _) in tally.items()} == {t: True for t in tally}
            assert ref.lipinski_rules5(valid["mol"], described["desc"], got["mol"]) == g["lipinski5"], b
    assert [g["status"] for g in golden] == [0] * 7 + [5]


# ---- 8. csrc/mol_sub.h on the host ---------------------------------------------------------------------------------------------------
def _harness_case(atoms, rows, described, tables):
    """(input text, {(p, a): (verdict, steps)}) of one molecule for tests/mol_sub_harness.cpp."""
    args = table_args(tables)
    steps = {}
    got = ref.match(atoms, rows, described, steps_out=steps, **args)
    props, nbrs = ref.stage(atoms, [tuple(int(x) for x in r) for r in rows][:len(described["classes"])], described, args["bond_rows"],
                            args["atom_sets"])
    lines = [f"{len(atoms)} {tables.n_patterns}"]
    for a in range(len(atoms)):
        if a not in props:
            lines.append(f"{ref.NO_KEY} 0 0 0")
            continue
        entries = [v << 8 | nbrs[a][v] for v in sorted(nbrs[a])]
        lines.append(" ".join(map(str, [described["keys"][a], props[a]["sets"], props[a]["ring"], len(entries)] + entries)))
    lines += [" ".join(map(str, rec.tolist())) for rec in tables.pattern_rows]
    return "\n".join(lines) + "\n", steps, got


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("mol_sub") / "mol_sub_harness")
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=",
                           os.path.join(ROOT, "tests", "mol_sub_harness.cpp"), "-o", exe])

    def run(cases):
        import subprocess
        out = subprocess.run([exe], input="".join(c[0] for c in cases), capture_output=True, text=True, check=True).stdout
        blocks = out.split("end\n")[:-1]
        assert len(blocks) == len(cases)
        for (_, steps, _), block in zip(cases, blocks):
            got = {(p, a): (v, s) for p, a, v, s in (map(int, line.split()) for line in block.splitlines())}
            assert got == steps
    return run


def probe_patterns():
    """Patterns that walk: chains of wildcards (dead-ended and not), rings with closures, branches, the built-in rows."""
    from druggen_amd import substructure as sub
    rows = [("ring5", "[*]1~[*]~[*]~[*]~[*]~1"), ("ring6", "[C]1:[*]:[*]:[*]:[*]:[*]:1"), ("fused", "[*]1~[*]~[*]~[*]2~[*]~[*]~[*]~[*]~[*]~2~[*]~1"),
            ("chain16", "~".join(["[*]"] * 16)), ("dead16", dead_end_chain(16, "[#92]")), ("dead7", dead_end_chain(7, "[#92]")),
            ("branch", "[C]([*])([*])~[*]([*])~[*]"), ("hetero", "[!C]~[C]~[!C]"), ("ringbond", "[*;R]-,=!@[*]~@[*]")]
    return sub.LOGP, list(sub.GROUPS) + rows


def test_the_search_on_the_host_equals_the_restatement_step_for_step(harness):
    """csrc/mol_sub.h is plain C++: tests/mol_sub_harness.cpp runs the predicate and the bounded search on seeded molecule-like
    graphs of 1 .. 40 atoms under the built-in and the probe patterns; every verdict and every step count equals the
    restatement's, and nothing runs over."""
    typing, patterns = probe_patterns()
    tables = make_tables(typing=typing, patterns=patterns)
    rng = np.random.default_rng(332)
    cases, valid_seen, hit = [], 0, set()
    for k, n in enumerate([1, 2, 3, 5, 9, 14, 20, 27, 33, 40] * 2):
        atoms, labels = vref.aromatic_like(rng, n, True)
        m = dref.decode_labels(atoms, labels)
        described = descref.describe(m["atoms"], m["bonds"], vref.validity(m["atoms"], m["bonds"]))
        if described["desc"][0] != 0:
            continue
        valid_seen += 1
        case = _harness_case(m["atoms"], m["bonds"], described, tables)
        assert case[2]["mol"][7] == 0 and all(s < ref.MAX_STEPS for _, s in case[1].values())
        hit |= {tables.names[p] for p, h in enumerate(case[2]["hits"]) if h}
        cases.append(case)
    for smiles in ("c1ccc2ccccc2c1", "c1ccc2cccc2cc1", "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "CC(=O)Oc1ccccc1C(=O)O", "C1CC1C1CC1", "ClC(Cl)(Cl)C#N"):
        atoms, rows = from_smiles(smiles)
        described = descref.describe(atoms, rows, vref.validity(atoms, rows))
        case = _harness_case(atoms, rows, described, tables)
        assert described["desc"][0] == 0 and case[2]["mol"][7] == 0
        hit |= {tables.names[p] for p, h in enumerate(case[2]["hits"]) if h}
        cases.append(case)
    assert valid_seen >= 12 and {"ring5", "ring6", "fused", "chain16", "branch", "C.ar.fused", "ringbond"} <= hit and "dead7" not in hit
    assert max(s for c in cases for _, s in c[1].values()) > 300
    harness(cases)


def test_the_step_bound_on_the_lattice(harness):
    """A condition, not a measurement: from the centre of the 6 x 6 lattice (the smallest on which this happens: the 5 x 5 one
    completes in 3713 steps) a 10-atom dead-end chain of wildcards is OVER at exactly 4096 steps, a 4-atom one is a completed miss,
    and csrc/mol_sub.h gives the same verdicts and step counts everywhere on the lattice."""
    tables = make_tables(patterns=[("dead10", dead_end_chain(10)), ("dead4", dead_end_chain(4)), ("dead8", dead_end_chain(8)),
                                   ("square", "[C]1[C][C][C]1"), ("chain16", "~".join(["[*]"] * 16))])
    atoms, rows, described = ref.lattice_described(LATTICE_SIDE)
    case = _harness_case(atoms, rows, described, tables)
    steps, got = case[1], case[2]
    centre = (LATTICE_SIDE // 2) * LATTICE_SIDE + LATTICE_SIDE // 2
    assert steps[(0, centre)] == (-1, 4096) and steps[(1, centre)] == (0, 67) and steps[(1, centre)][1] < ref.MAX_STEPS
    assert got["mol"][7] == sum(v < 0 for v, _ in steps.values()) > 0 and got["hits"][:3] == [0, 0, 0] and got["hits"][3] == 36
    assert got["hits"][4] == 36 and all(v == 1 for (p, _), (v, _) in steps.items() if p == 4)
    small = ref.lattice_described(LATTICE_SIDE - 1)
    small_steps = _harness_case(*small, tables)[1]
    assert small_steps[(0, 2 * 5 + 2)] == (0, 3713)
    # the issue's figures for the unbounded search, from the centre of the 16 x 16 lattice: 4869 steps at 8 atoms, 37177 at 10
    big_atoms, big_rows, big = ref.lattice_described(16)
    props, nbrs = ref.stage(big_atoms, big_rows, big, descref.BOND_ROWS, tables.atom_set_rows.tolist())
    bound, ref.MAX_STEPS = ref.MAX_STEPS, 1 << 30
    try:
        assert [ref.search(tables.pattern_rows[p], props, nbrs, 8 * 16 + 8) for p in (2, 0)] == [(0, 4869), (0, 37177)]
    finally:
        ref.MAX_STEPS = bound
    harness([case, _harness_case(*small, tables)])


def test_the_bound_leaves_the_fixture_molecules_a_wide_margin():
    """A 16-atom dead-end chain of wildcards -- a full enumeration -- from every atom of the eight fixture molecules: at most 443
    steps, a factor of nine below the bound."""
    strings, atoms, labels, atom_dec, bond_dec, vtab, dtab = fixture_tables()
    tables = make_tables(patterns=[("dead16", dead_end_chain(16, "[#92]"))], atom_decoder=atom_dec, bond_decoder=bond_dec)
    worst = 0
    for b in range(len(strings)):
        m = dref.decode_labels(atoms[b], labels[b])
        described = descref.describe(m["atoms"], m["bonds"], vref.validity(m["atoms"], m["bonds"], **vtab), **dtab)
        steps = {}
        ref.match(m["atoms"], m["bonds"], described, steps_out=steps, **table_args(tables))
        worst = max([worst] + [s for _, s in steps.values()])
    assert worst == 443 and 9 * worst < ref.MAX_STEPS
