"""Plain-Python restatement of `dg_mol_descriptors` (include/druggen_hip_desc.h), written from the header's comment alone: Python
integers and sets, bridges by removing each bond and testing whether its ends stay connected (as tests/mol_fp_ref.py does -- no
spanning forest), triangles from neighbour sets (no bit rows), components by a flood fill, the table as a dict (no search).  Its
validity input is the result of tests/mol_valid_ref.py (`validity` / `analyse`) for the same molecule under the same scope: the
status and `hcount` are taken from there, as the kernel takes them from `dg_mol_validity`.  The molecules are the per-molecule
dicts of tests/decode_graph_ref.py (`decode_labels`)."""
import numpy as np

import mol_valid_ref as vref
from mol_fp_ref import _connected, scope_atoms, scope_bonds

WHOLE, LARGEST = 0, 1
DESC_FIELDS = ("status", "n_heavy", "n_rot", "tpsa", "n_untyped", "n_rings", "n_ring_atoms", "n_aromatic_atoms", "n_carbon",
               "n_sp3_carbon", "reserved0", "reserved1")
NO_KEY = 0xFFFFFFFF
MAX_ENV = 4096
BOND, RING_BOND, ROTATABLE = 1, 2, 4

# the tables of the tests over mol_fp_ref.ATOM_DECODER (pad, C, N, O, S, Cl, Se) and BOND_DECODER (none, single, double, triple,
# aromatic): the carbon bit, the polar bit of mol_valid_ref.ATOM_ROWS, and the issue's TPSA table expanded by hand over the
# labels 2 (N) and 3 (O)
ATOM_CLASS = [0, 1, 0, 0, 0, 0, 0]
ATOM_FLAGS = [row[2] for row in vref.ATOM_ROWS]
BOND_ROWS = vref.BOND_ROWS
# (label, h, n1, n2, n3, na, r3 or None for both, 1e-2 A^2)
TPSA_ROWS = [
    (2, 0, 3, 0, 0, 0, 0, 324), (2, 0, 3, 0, 0, 0, 1, 301), (2, 0, 1, 1, 0, 0, None, 1236), (2, 0, 0, 0, 1, 0, None, 2379),
    (2, 1, 2, 0, 0, 0, 0, 1203), (2, 1, 2, 0, 0, 0, 1, 2194), (2, 1, 0, 1, 0, 0, None, 2385), (2, 2, 1, 0, 0, 0, None, 2602),
    (2, 0, 0, 0, 0, 2, None, 1289), (2, 0, 0, 0, 0, 3, None, 441), (2, 0, 1, 0, 0, 2, None, 493),
    (3, 0, 2, 0, 0, 0, 0, 923), (3, 0, 2, 0, 0, 0, 1, 1253), (3, 0, 0, 1, 0, 0, None, 1707), (3, 1, 1, 0, 0, 0, None, 2023),
    (3, 0, 0, 0, 0, 2, None, 1314),
]


def key_of(label, h, n1, n2, n3, na, r3):
    return label | h << 8 | n1 << 12 | n2 << 16 | n3 << 19 | na << 21 | r3 << 24


def env_dict(rows=TPSA_ROWS):
    """{key: value} of rows (label, h, n1, n2, n3, na, r3 / None, value)."""
    out = {}
    for label, h, n1, n2, n3, na, r3, value in rows:
        for r in ((0, 1) if r3 is None else (r3,)):
            out[key_of(label, h, n1, n2, n3, na, r)] = value
    return out


ENV = env_dict()


def env_for(atom_decoder):
    """TPSA_ROWS over another atom decoder (label -> atomic number): the rows of label 2 go to every label of N, those of label
    3 to every label of O."""
    rows = [(l,) + row[1:] for row in TPSA_ROWS for l in sorted(atom_decoder) if atom_decoder[l] == {2: 7, 3: 8}[row[0]]]
    return env_dict(rows)


def blank(status, N, n_rows):
    return dict(desc=[status] + [0] * 11, keys=[NO_KEY] * N, classes=[0] * n_rows)


def describe(atoms, rows, valid, n_bonds=None, cap=None, flag=0, scope=WHOLE, component=None, largest=None, bond_rows=BOND_ROWS,
             atom_flags=ATOM_FLAGS, atom_class=ATOM_CLASS, env=ENV):
    """One molecule as the entry sees it -> dict(desc=[12 ints], keys=[N ints], classes=[min(n_bonds, cap) ints]).  `valid`:
    mol_valid_ref's result for it (only `mol[0]` and `hcount` are used)."""
    atoms = [int(a) for a in atoms]
    rows = [(int(i), int(j), int(l)) for i, j, l in rows]
    N = len(atoms)
    n_bonds = len(rows) if n_bonds is None else n_bonds
    read = max(min(n_bonds, len(rows) if cap is None else cap), 0)
    if (cap is not None and n_bonds > cap) or flag < 0:
        return blank(vref.NO_GRAPH, N, read)
    if valid["mol"][0] != vref.VALID:
        return blank(valid["mol"][0], N, read)
    rows = rows[:read]
    members = scope_atoms(atoms, rows, scope, component, largest)
    bonds = scope_bonds(atoms, rows, members)
    n = {a: [0, 0, 0, 0] for a in members}      # n1, n2, n3, na
    nbrs = {a: set() for a in members}
    at = {}
    for k, (i, j, l) in enumerate(bonds):
        order, aromatic = vref.bond_row(bond_rows[l])
        for a, other in ((i, j), (j, i)):
            n[a][3 if aromatic else order - 1] += 1
            nbrs[a].add(other)
            at.setdefault(a, []).append(k)
    deg = {a: sum(n[a]) for a in members}
    r3 = {a: int(any(v in nbrs[u] for u in nbrs[a] for v in nbrs[a] if u != v)) for a in members}
    h = {a: valid["hcount"][a] for a in members}
    key = {a: key_of(atoms[a], h[a], *n[a], r3[a]) for a in members}
    bridge = {b: not _connected(b[0], b[1], bonds, at, k) for k, b in enumerate(bonds)}
    rotatable = {b: bridge[b] and vref.bond_row(bond_rows[b[2]]) == (1, 0) and deg[b[0]] >= 2 and deg[b[1]] >= 2
                 and n[b[0]][2] == 0 and n[b[1]][2] == 0 for b in bonds}
    classes = []
    for row in rows:
        classes.append(BOND | (0 if bridge[row] else RING_BOND) | (ROTATABLE if rotatable[row] else 0) if row in bridge else 0)
    seen, components = set(), 0
    for a in sorted(members):
        if a in seen:
            continue
        components += 1
        stack = [a]
        seen.add(a)
        while stack:
            for y in nbrs[stack.pop()]:
                if y not in seen:
                    seen.add(y)
                    stack.append(y)
    ring_atoms = {a for b in bonds if not bridge[b] for a in b[:2]}
    carbons = [a for a in members if atom_class[atoms[a]] & 1]
    desc = [vref.VALID, len(members), sum(rotatable.values()), sum(env.get(key[a], 0) for a in members) & 0xFFFFFFFF,
            sum(1 for a in members if atom_flags[atoms[a]] & 1 and key[a] not in env),
            len(bonds) - len(members) + components, len(ring_atoms), sum(1 for a in members if n[a][3] > 0), len(carbons),
            sum(1 for a in carbons if n[a][1] == n[a][2] == n[a][3] == 0), 0, 0]
    return dict(desc=desc, keys=[key.get(a, NO_KEY) for a in range(N)], classes=classes)


def describe_batch(mols, valids, cap=None, scope=LARGEST, **kw):
    """`mols`: the dicts of `decode_graph_ref.decode_labels`; `valids`: `mol_valid_ref.validity_batch` of them under the same
    cap and scope -> one result per molecule."""
    return [describe(m["atoms"], m["bonds"], v, n_bonds=m["n_bonds"], cap=cap, scope=scope, component=m["component"],
                     largest=m["largest"], **kw) for m, v in zip(mols, valids)]


def veber_rules(desc):
    return (int(desc[2] <= 10) + int(desc[3] <= 14000)) * (desc[0] == 0)


def lipinski_rules(mol, desc):
    """`mol`: the validity row (status, n_atoms, n_over, deficiency, n_h, mass, n_donors, n_acceptors)."""
    return (int(mol[5] < 5000000) + int(mol[6] <= 5) + int(mol[7] <= 10) + int(desc[2] <= 10)) * (desc[0] == 0)


def assert_batch_equals(host, want):
    """Every `desc` field, every key and the written bond classes of a host `MoleculeDescriptors` against the restatement's
    list, with `==`."""
    assert host.B == len(want)
    for b, w in enumerate(want):
        got = host.desc[b].tolist()
        signed = [(v & 0xFFFFFFFF) - ((v & 0x80000000) << 1) for v in w["desc"]]      # (tpsa is a sum modulo 2^32)
        assert got == signed, (b, dict(zip(DESC_FIELDS, got)), w["desc"])
        assert host.atom_key[b].view(np.uint32).tolist() == w["keys"], b
        assert host.bond_class[b, :len(w["classes"])].tolist() == w["classes"], b
