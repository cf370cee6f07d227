"""Host side of the SMILES writer (csrc/mol_smiles.hip, druggen_amd/smiles_out.py): the plain-Python restatement
(tests/mol_smiles_ref.py) read back by the project's own parser, the grammar's edge cases, the second public header against its
ctypes table, every argument refusal of the C entry -- all of which return before a launch -- and the host checks of
smiles_out.py.  No GPU."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_smiles_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -1, -2      # DG_E_SHAPE, DG_E_ARG of include/druggen_hip.h


def _write(atoms, labels, scope=ref.WHOLE, **kw):
    m = dref.decode_labels(atoms, labels)
    return ref.write(m["atoms"], m["bonds"], *ref.tables(), n_bonds=m["n_bonds"], component=m["component"],
                     largest=m["largest"], scope=scope, **kw)


def _string(result):
    assert result["length"] >= 0, result["length"]
    text = result["text"]
    assert not any(text[result["length"]:]) and 0 not in text[:result["length"]]
    return text[:result["length"]].decode("ascii")


# ---- 1. the restatement, read back by smiles.parse_smiles -------------------------------------------------------------------
def test_restatement_round_trips_through_the_parser():
    """Seeded molecule-like graphs with 0, 1, 2, 4 closures -- relabelled to six elements (C N O S Cl Se) and four bond types,
    aromatic included, no bonded pad -- cycles, a star, decalin and bicyclopentyl: none is left out, every string parses back
    to exactly the graph it was written from."""
    rng = np.random.default_rng(2025)
    graphs = [ref.relabelled(rng, *cref.molecule_like(rng, N, closures)) for N, closures, one in cref.MOLECULE_FAMILY if not one]
    graphs += [cref.molecule_like(rng, N, closures, True) for N, closures, one in cref.MOLECULE_FAMILY if one]
    graphs += [cref.cycle(n) for n in (3, 6, 12)] + [cref.cycle(6, label=4), cref.cycle(5, label=4, atom=2)]
    graphs += [(np.ones(9, dtype=np.int64), dref.star(9, 4)), cref.decalin(), cref.bicyclopentyl()]
    graphs += [ref.relabelled(rng, *g) for g in (cref.decalin(), cref.bicyclopentyl(), cref.cycle(7))]
    assert len(graphs) > 80
    seen = set()
    for atoms, labels in graphs:
        out = _write(atoms, labels)
        text = _string(out)
        assert out["n_written"] == len(atoms) and sorted(out["order"]) == list(range(len(atoms)))
        ref.parse_back(text, atoms, labels, out["order"])
        seen.update(text)
    assert set("CNOSclnos[]()=#:-12") <= seen, sorted(seen)      # the grammar was exercised: both cases, brackets, every bond symbol


# ---- 2. the fixture strings --------------------------------------------------------------------------------------------------
def _fixture_strings():
    with open(os.path.join(ROOT, "tests", "golden", "chembl_like_smiles.csv")) as f:
        rows = list(csv.DictReader(line for line in f if not line.startswith("#")))
    assert len(rows) == 8
    return [r["SMILES"] for r in rows]


def test_the_eight_fixture_strings_are_written_back():
    """Each string parsed to a labelled graph and written: the result parses back to the same graph; rows 2 to 4 -- written by
    RDKit, no brackets -- come back byte for byte, row 1 up to the order of two ring-closure digits."""
    from druggen_amd import smiles, smiles_out
    strings = _fixture_strings()
    atom_enc, atom_dec, bond_enc, bond_dec, kept, longest = smiles.build_encoders(strings, 64)
    assert kept == strings
    tables = smiles_out.table_rows(atom_dec, bond_dec)
    written = []
    for s in strings:
        z, _, bonds = smiles.parse_smiles(s)
        atoms = np.array([atom_enc[a] for a in z])
        labels = np.zeros((len(z), len(z)), dtype=np.int64)
        for i, j, t in bonds:
            labels[max(i, j), min(i, j)] = bond_enc[t]
        m = dref.decode_labels(atoms, labels)
        out = ref.write(m["atoms"], m["bonds"], *tables, scope=ref.WHOLE)
        text = _string(out)
        ref.parse_back(text, atoms, labels, out["order"], atom_dec, bond_dec)
        written.append(text)
    assert written[1:4] == strings[1:4]
    assert written[0] == strings[0][:-3] + "c12" and strings[0].endswith("c21")


# ---- 3. edge cases of the grammar --------------------------------------------------------------------------------------------
def test_twelve_nested_rings_take_two_digit_numbers():
    """A path of 24 atoms with bonds i to 23 - i: the innermost of the twelve is the path's own bond 11 - 12, eleven are open at
    atom 10."""
    atoms, labels = cref.from_edges(24, [(i, i + 1) for i in range(23)] + [(i, 23 - i) for i in range(11)])
    out = _write(atoms, labels)
    text = _string(out)
    assert "%10" in text and "%11" in text and "%12" not in text and text.startswith("C1C2C3")
    ref.parse_back(text, atoms, labels, out["order"])


def test_a_chain_of_separate_rings_reuses_digit_1():
    edges = []
    for r in range(4):      # four three-rings on a chain
        a = 3 * r
        edges += [(a, a + 1), (a + 1, a + 2), (a + 2, a)] + ([(a + 2, a + 3)] if r < 3 else [])
    atoms, labels = cref.from_edges(12, edges)
    out = _write(atoms, labels)
    text = _string(out)
    assert text == "C1CC1C1CC1C1CC1C1CC1" and "2" not in text
    ref.parse_back(text, atoms, labels, out["order"])


def test_a_number_closed_at_an_atom_is_not_reopened_there():
    """Atom 2 closes ring 1 and opens another: `C11` must not appear, the new ring takes 2."""
    atoms, labels = cref.from_edges(5, [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 2)])
    out = _write(atoms, labels)
    text = _string(out)
    assert text == "C1CC12CC2"
    ref.parse_back(text, atoms, labels, out["order"])


def test_bond_symbols_between_lower_and_upper_case_atoms():
    # biphenyl: two aromatic six-rings joined by a single bond
    atoms = np.ones(12, dtype=np.int64)
    labels = np.zeros((12, 12), dtype=np.int64)
    for ring in (0, 6):
        for k in range(6):
            i, j = ring + k, ring + (k + 1) % 6
            labels[max(i, j), min(i, j)] = 4
    labels[6, 5] = 1
    out = _write(atoms, labels)
    assert _string(out) == "c1ccccc1-c1ccccc1"
    ref.parse_back(_string(out), atoms, labels, out["order"])
    # an aromatic bond to an atom that is never lower-case (Cl), a double bond out of an aromatic ring, [se] in a ring
    atoms = np.array([1, 1, 1, 1, 6, 5, 3])
    labels = np.zeros((7, 7), dtype=np.int64)
    for i, j in ((1, 0), (2, 1), (3, 2), (4, 3), (4, 0)):
        labels[i, j] = 4
    labels[5, 0], labels[6, 2] = 4, 2
    out = _write(atoms, labels)
    assert _string(out) == "c1(cc(c[se]1)=O):Cl"
    ref.parse_back(_string(out), atoms, labels, out["order"])
    # without an aromatic bond nothing is lower-case and brackets stay
    out = _write(np.array([6, 1, 4]), dref.path(3))
    assert _string(out) == "[Se]CS"


def test_components_are_joined_by_a_dot_and_largest_takes_one():
    atoms = np.array([1, 2, 1, 3, 1, 2, 0, 0])
    labels = np.pad(dref.two_equal_components(6), ((0, 2), (0, 2)))
    whole, largest = _write(atoms, labels, ref.WHOLE), _write(atoms, labels, ref.LARGEST)
    assert _string(whole) == "CCC.NON" and whole["order"] == [0, 2, 4, 1, 3, 5]
    assert _string(largest) == "CCC" and largest["order"] == [0, 2, 4] and largest["n_written"] == 3
    ref.parse_back(_string(whole), atoms, labels, whole["order"])
    ref.parse_back(_string(largest), atoms, labels, largest["order"])
    # all pads: nothing under 'whole', the single pad of component 0 under 'largest'
    pads = np.zeros(4, dtype=np.int64), dref.empty_graph(4)
    assert (_write(*pads, ref.WHOLE)["length"], _write(*pads, ref.WHOLE)["n_written"]) == (0, 0)
    assert _string(_write(*pads, ref.LARGEST)) == "*"


def test_a_bonded_pad_is_written_as_a_star():
    out = _write(np.array([1, 0, 2]), dref.path(3))
    assert _string(out) == "C*N" and out["order"] == [0, 1, 2]


def test_labels_without_a_symbol_are_written_as_question_marks():
    atoms, bonds = np.array([1, 9, 1]), np.array([[1, 0, 1], [2, 1, 7]])
    out = ref.write(atoms, bonds, *ref.tables())
    assert _string(out) == "C??C"


def test_dense_graphs_run_out_of_ring_numbers():
    rng = np.random.default_rng(45)
    for E in (2, 5):
        atoms, labels = rng.integers(1, 4, 45), np.tril(rng.integers(0, E, (45, 45)), -1)
        out = _write(atoms, labels)
        assert out["length"] == ref.RINGS and out["text"] == bytes(360) and out["n_written"] == 45
        assert sorted(out["order"]) == list(range(45))
    # -3 outranks -4
    assert _write(atoms, labels, str_cap=3)["length"] == ref.RINGS
    # exactly 99 open at once still fit, 100 do not: atom 0 of a path bonded to every atom from 2 on
    hub = cref.from_edges(102, [(i, i + 1) for i in range(101)] + [(0, i) for i in range(2, 102)])
    assert _write(*hub, str_cap=2000)["length"] == ref.RINGS
    hub = cref.from_edges(101, [(i, i + 1) for i in range(100)] + [(0, i) for i in range(2, 101)])
    out = _write(*hub, str_cap=2000)
    assert "%99" in _string(out)
    ref.parse_back(_string(out), *hub, out["order"])


def test_a_string_cap_one_byte_short_and_a_truncated_list():
    rng = np.random.default_rng(9)
    atoms, labels = ref.relabelled(rng, *cref.molecule_like(rng, 17, 2))
    full = _write(atoms, labels)
    n = full["length"]
    exact, short = _write(atoms, labels, str_cap=n), _write(atoms, labels, str_cap=n - 1)
    assert exact["length"] == n and exact["text"] == full["text"][:n]
    assert short["length"] == ref.LONG and short["text"] == bytes(n - 1) and short["order"] == full["order"]
    m = dref.decode_labels(atoms, labels)
    cut = ref.write(m["atoms"], m["bonds"][:m["n_bonds"] - 1], *ref.tables(), n_bonds=m["n_bonds"], cap=m["n_bonds"] - 1)
    assert cut == dict(length=ref.NO_GRAPH, n_written=0, order=[], text=bytes(8 * 17))
    flagged = ref.write(m["atoms"], m["bonds"], *ref.tables(), flag=-2)
    assert flagged["length"] == ref.NO_GRAPH and flagged["n_written"] == 0


def test_forms_scope_skips_the_filler_atoms():
    out = ref.write([1, 2, 0xFF, 0xFF], [(1, 0, 2)], *ref.tables(), scope=ref.FORMS)
    assert _string(out) == "C=N" and out["order"] == [0, 1]


# ---- 4. the second header against the second table ---------------------------------------------------------------------------
def _kind(decl):
    decl = re.sub(r"\bconst\b", " ", decl).strip()
    if "*" in decl or re.match(r"dg_stream_t\b", decl):
        return "pointer"
    kind = decl.split()[0]
    assert kind in ("int", "int64_t", "size_t", "float", "double"), decl
    return kind


def test_text_header_matches_its_ctypes_table_parameter_by_parameter():
    from druggen_amd import _lib
    named = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
             ctypes.c_double: "double", ctypes.c_char_p: "pointer", ctypes.c_void_p: "pointer"}
    header = open(os.path.join(ROOT, "include", "druggen_hip_text.h")).read()
    assert re.search(r'^#include "druggen_hip.h"', header, flags=re.M)
    macro = {k: int(v) for k, v in re.findall(r"^#define\s+(DG_SMILES_[A-Z_]+)\s+\(?(-?\d+)\)?", header, flags=re.M)}
    assert (macro["DG_SMILES_FORMS"], macro["DG_SMILES_NO_GRAPH"], macro["DG_SMILES_RINGS"], macro["DG_SMILES_LONG"]) == \
        (ref.FORMS, ref.NO_GRAPH, ref.RINGS, ref.LONG)
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    header = re.sub(r"^\s*#.*$", " ", header, flags=re.M)
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header)
    names = [name for _, name, _ in protos]
    assert names == list(_lib.TEXT_SIGNATURES) == ["dg_mol_smiles"]
    assert not set(names) & set(_lib.SIGNATURES)
    first = open(os.path.join(ROOT, "include", "druggen_hip.h")).read()
    assert not any(re.search(rf"\b{name}\s*\(", first) for name in names)      # the first header's check reads comments too
    lib = _lib.load()
    for ret, name, params in protos:
        res, args = _lib.TEXT_SIGNATURES[name]
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
    names = ("atoms", "bonds", "n_bonds", "component", "largest", "flags", "atom_table", "bond_table", "length", "n_written",
             "order", "text")

    def call(B=3, N=9, cap=36, scope=1, str_cap=72, n_atom_labels=7, n_bond_labels=5, **ptrs):
        p = {n: P for n in names}
        p.update(ptrs)
        return lib.dg_mol_smiles(p["atoms"], p["bonds"], p["n_bonds"], p["component"], p["largest"], p["flags"], p["atom_table"],
                                 n_atom_labels, p["bond_table"], n_bond_labels, B, N, cap, scope, str_cap, p["length"],
                                 p["n_written"], p["order"], p["text"], None)

    def err():
        return lib.dg_last_error_string()
    for kw in (dict(B=-1), dict(N=0), dict(N=257), dict(N=-4), dict(N=1 << 20), dict(cap=-1), dict(str_cap=0), dict(str_cap=-8),
               dict(n_atom_labels=0), dict(n_atom_labels=256), dict(n_bond_labels=0), dict(n_bond_labels=257)):
        assert call(**kw) == SHAPE and b"dg_mol_smiles: need B >= 0, 1 <= N <= 256" in err(), kw
    # LDS: 49152 bytes hold the bit rows, the label triangle and the string
    for N, most in ((256, 49152 - 8192 - 32640), (45, 49152 - 45 * 2 * 4 - 992), (1, 49152 - 4)):
        assert call(B=0, N=N, str_cap=most) == 0, N
        assert call(B=0, N=N, str_cap=most + 1) == SHAPE and b"does not fit LDS" in err(), N
    assert call(B=0, N=256, str_cap=1 << 30) == SHAPE and call(B=0, N=256, str_cap=(1 << 31) - 1) == SHAPE
    for scope in (-1, 3, 4, 256):
        assert call(scope=scope) == ARG and b"scope must be 0 (whole), 1 (largest) or 2 (forms)" in err(), scope
    for name in ("atoms", "n_bonds", "atom_table", "bond_table", "length", "n_written", "order", "text", "bonds", "component",
                 "largest"):
        assert call(**{name: None}) == ARG and b"dg_mol_smiles: null pointer" in err(), name
    for name in ("bonds", "n_bonds", "largest", "flags", "length", "n_written"):
        assert call(**{name: P + 2}) == ARG and b"aligned" in err(), name
    # the shape comes first, then the scope, then the pointers
    assert call(N=257, scope=5, atoms=None) == SHAPE and call(scope=5, atoms=None) == ARG and b"scope" in err()
    # an empty batch is no launch; the optional pointers may be null, B == 0 still checks the rest
    assert call(B=0) == 0 and call(B=0, flags=None) == 0 and call(B=0, cap=0, bonds=None) == 0
    assert call(B=0, scope=0, component=None, largest=None) == 0 and call(B=0, scope=2, component=None, largest=None) == 0
    assert call(B=0, scope=1, component=None) == ARG and call(B=0, text=None) == ARG and call(B=0, scope=3) == ARG


# ---- 6. smiles_out.py ----------------------------------------------------------------------------------------------------------
def test_tables_from_decoders():
    from druggen_amd import smiles_out
    atom_rows, bond_rows = ref.tables()
    assert atom_rows.tolist() == [[ord("*"), 0, 0, 0], [ord("C"), 0, 2, 0], [ord("N"), 0, 2, 0], [ord("O"), 0, 2, 0],
                                  [ord("S"), 0, 2, 0], [ord("C"), ord("l"), 0, 0], [ord("S"), ord("e"), 3, 0]]
    assert bond_rows.tolist() == [[0, 0], [ord("-"), 0], [ord("="), 0], [ord("#"), 0], [ord(":"), 1]]
    rows, _ = smiles_out.table_rows({0: 0, 1: 14, 2: 9, 3: 35, 4: 33, 5: 53}, {0: 0})
    assert [bytes(r[:2]).rstrip(b"\0").decode() for r in rows] == ["*", "Si", "F", "Br", "As", "I"]
    assert rows[:, 2].tolist() == [0, 1, 0, 0, 3, 0]
    for bad in ({0: 0, 1: 1}, {0: 0, 1: 55}, {0: 0, 1: -6}, {0: 0, 1: 119}):
        with pytest.raises(ValueError, match="atomic number"):
            smiles_out.table_rows(bad, ref.BOND_DECODER)
    for bad in ({0: 0, 1: 4}, {0: 0, 1: 1, 2: 21}):
        with pytest.raises(ValueError, match="bond type"):
            smiles_out.table_rows(ref.ATOM_DECODER, bad)
    for bad in ({}, {1: 6}, {0: 0, 2: 6}):
        with pytest.raises(ValueError, match="labels 0..n-1"):
            smiles_out.table_rows(bad, ref.BOND_DECODER)
    with pytest.raises(ValueError, match="256 labels"):
        smiles_out.table_rows({l: 6 for l in range(256)}, ref.BOND_DECODER)
    assert len(smiles_out.table_rows({l: 6 for l in range(255)}, ref.BOND_DECODER)[0]) == 255
    with pytest.raises(ValueError, match="257 labels"):
        smiles_out.table_rows(ref.ATOM_DECODER, {l: 1 for l in range(257)})


def test_python_refusals_without_a_gpu():
    """smiles_out.py refuses host batches, host forms, other sources, other tables, another scope than the forms' own, a bad
    str_cap and a wrong out= -- all before any launch."""
    from druggen_amd import canon, smiles_out
    from druggen_amd.decode import MoleculeBatch, _layout
    tables = smiles_out.SmilesTables(*ref.tables(), "cpu")
    assert (tables.n_atom_labels, tables.n_bond_labels) == (7, 5) and tables.atoms.dtype.itemsize == 1
    host = MoleculeBatch(np.zeros(_layout(2, 3, 3, False)[1], dtype=np.uint8), 2, 3, 3, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        smiles_out.write_smiles(host, tables)
    forms = canon.CanonicalForms(np.zeros(canon._layout(2, 3, 3)[1], dtype=np.uint8), 2, 3, 3, "largest")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        smiles_out.write_smiles(forms, tables)
    with pytest.raises(TypeError, match="MoleculeBatch"):
        smiles_out.write_smiles(np.zeros(4), tables)
    with pytest.raises(TypeError, match="SmilesTables"):
        smiles_out.write_smiles(host, ref.tables())

    class Device:      # stands in for a device buffer: the checks below come before anything touches it
        is_cuda, device = True, "cuda:0"
    host.is_host, host.buffer = False, Device()
    forms.is_host, forms.buffer = False, Device()
    with pytest.raises(ValueError, match="scope must be"):
        smiles_out.write_smiles(host, tables, scope="fragment")
    with pytest.raises(ValueError, match="carries its scope"):
        smiles_out.write_smiles(forms, tables, scope="whole")
    with pytest.raises(ValueError, match="the tables live on cpu"):
        smiles_out.write_smiles(host, tables)
    tables.device = "cuda:0"
    for bad in (0, -1):
        with pytest.raises(ValueError, match="str_cap"):
            smiles_out.write_smiles(host, tables, str_cap=bad)
    for out in (np.zeros(3), smiles_out.SmilesBatch(np.zeros(smiles_out._layout(2, 3, 24)[1], dtype=np.uint8), 2, 3, 24)):
        with pytest.raises(ValueError, match="out="):      # not a SmilesBatch; a host one
            smiles_out.write_smiles(forms, tables, out=out)


def test_strings_read_the_host_copy():
    from druggen_amd import smiles_out
    table, total = smiles_out._layout(3, 4, 8)
    assert [table[k][0] % 16 for k in ("length", "n_written", "order", "text")] == [0] * 4 and total % 16 == 0
    s = smiles_out.SmilesBatch(np.zeros(total, dtype=np.uint8), 3, 4, 8)
    assert s.is_host and s.cpu() is s and s.length.dtype == np.int32 and s.text.shape == (3, 8) and s.order.shape == (3, 4)
    s.text[0, :3] = list(b"C=O")
    s.length[:] = [3, -3, 0]
    assert s.strings() == ["C=O", None, ""] and set(smiles_out.STATUS) == {-2, -3, -4}
