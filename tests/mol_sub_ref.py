"""Plain-Python restatement of `dg_mol_substructure` (include/druggen_hip_sub.h), written from the header's comment alone: Python
integers, dicts and sets, the search as a RECURSIVE generator-free depth-first walk with a step counter that raises when it
reaches the bound (the kernel, csrc/mol_sub.h, walks iteratively over cursors in LDS -- the two sides cannot share a loop).  Its
inputs are the restatements' results: the descriptor record of tests/mol_desc_ref.py (`describe`: status, keys, classes) for the
same molecule, never the GPU's outputs.  The pattern table is the raw [n, 80] uint32 records; the record is decoded here."""
import numpy as np

import mol_valid_ref as vref

MOL_FIELDS = ("status", "n_heavy", "n_typed", "n_untyped", "sum0", "sum1", "n_patterns_hit", "n_over")
MAX_ATOMS, MAX_CLOSURES, MAX_PATTERNS, MAX_STEPS, MAX_NEIGHBOURS, PATTERN_WORDS, TYPING = 16, 8, 1024, 4096, 8, 80, 1
NO_KEY = 0xFFFFFFFF
BOND, RING_BOND = 1, 2


class Over(Exception):
    pass


def decode_record(rec):
    """(n, flags, values, atoms, closures) of one record; atoms: (sets, h, deg, n2, n3, arom, ring, r3, parent, bond)."""
    rec = [int(x) for x in rec]
    assert len(rec) == PATTERN_WORDS
    n, c = min(max(rec[0] & 255, 1), MAX_ATOMS), min((rec[0] >> 8) & 255, MAX_CLOSURES)
    signed = [v - (1 << 32) if v >> 31 else v for v in rec[1:5]]
    atoms = []
    for k in range(n):
        s, w1, w2, w3 = rec[8 + 4 * k:12 + 4 * k]
        atoms.append((s, w1 & 0x1FF, (w1 >> 16) & 0x1FF, w2 & 0x1F, (w2 >> 8) & 7, (w2 >> 12) & 3, (w2 >> 14) & 3, (w2 >> 16) & 3,
                      w3 & 15, (w3 >> 8) & 255))
    closures = [(w & 15, (w >> 8) & 15, (w >> 16) & 255) for w in rec[72:72 + c]]
    return n, rec[0] >> 16, signed, atoms, closures


def stage(atoms, rows, described, bond_rows, atom_sets):
    """The molecule as the definition sees it: {atom: properties} of the scope and {atom: {neighbour: kind}}."""
    keys, classes = described["keys"], described["classes"]
    N = len(atoms)
    props = {}
    for a in range(N):
        key = keys[a]
        if key == NO_KEY:
            continue
        n1, n2, n3, na = (key >> 12) & 15, (key >> 16) & 7, (key >> 19) & 3, (key >> 21) & 7
        label = int(atoms[a])
        props[a] = dict(h=(key >> 8) & 15, deg=n1 + n2 + n3 + na, n2=n2, n3=n3, arom=int(na > 0), r3=(key >> 24) & 1, ring=0,
                        sets=atom_sets[label] if label < len(atom_sets) else 0)
    nbrs = {a: {} for a in props}
    for (i, j, l), cls in zip(rows, classes):
        i, j, l = int(i), int(j), int(l)
        if not cls & BOND or i >= N or j >= N or i == j or i not in props or j not in props:
            continue
        kind = vref.bond_row(bond_rows[l]) if l < len(bond_rows) else None
        if kind is None:
            continue
        order, aromatic = kind
        ring = 1 if cls & RING_BOND else 0
        for x, y in ((i, j), (j, i)):
            assert y not in nbrs[x] and len(nbrs[x]) < MAX_NEIGHBOURS, "outside the definition: a pair twice or a ninth neighbour"
            nbrs[x][y] = (3 if aromatic else order - 1) + 4 * ring
            props[x]["ring"] |= ring
    return props, nbrs


def atom_ok(pa, x):
    sets, h, deg, n2, n3, arom, ring, r3 = pa[:8]

    def bit(mask, width, v):
        return v < width and (mask >> v) & 1
    return bool(x["sets"] & sets and bit(h, 9, x["h"]) and bit(deg, 9, x["deg"]) and bit(n2, 5, x["n2"]) and bit(n3, 3, x["n3"])
                and bit(arom, 2, x["arom"]) and bit(ring, 2, x["ring"]) and bit(r3, 2, x["r3"]))


def search(record, props, nbrs, a):
    """(verdict, steps): verdict 1 a match, 0 none, -1 OVER.  `record`: the 80 words, or `decode_record` of them."""
    n, _, _, patoms, closures = record if isinstance(record, tuple) else decode_record(record)
    steps = [1]
    if not atom_ok(patoms[0], props[a]):
        return 0, 1
    if n == 1:
        return 1, 1

    def extend(k, image):
        pa = patoms[k]
        origin = image[pa[8]]
        for v in sorted(nbrs[origin]):
            steps[0] += 1
            if steps[0] >= MAX_STEPS:
                raise Over
            kind = nbrs[origin][v]
            if v in image or not (pa[9] >> kind) & 1 or not atom_ok(pa, props[v]):
                continue
            if not all(image[j] in nbrs[v] and (mask >> nbrs[v][image[j]]) & 1 for ck, j, mask in closures if ck == k):
                continue
            if k == n - 1 or extend(k + 1, image + [v]):
                return True
        return False
    try:
        return int(extend(1, [a])), steps[0]
    except Over:
        return -1, steps[0]


def blank(status, N, n_patterns):
    return dict(mol=[status] + [0] * 7, hits=[0] * n_patterns, types=[-1] * N)


def match(atoms, rows, described, patterns, bond_rows, atom_sets, steps_out=None):
    """One molecule -> dict(mol=[8 ints], hits=[n_patterns], types=[N]).  `described`: mol_desc_ref's result for it (its status
    row 0, keys and classes are used); `rows`: the bond rows the classes belong to.  `steps_out`: a dict that receives
    {(p, a): (verdict, steps)}."""
    N = len(atoms)
    status = described["desc"][0]
    if status != 0:
        return blank(status, N, len(patterns))
    rows = [tuple(int(x) for x in r) for r in rows][:len(described["classes"])]
    props, nbrs = stage(atoms, rows, described, bond_rows, atom_sets)
    hits, types, over = [0] * len(patterns), [-1] * N, 0
    decoded = [decode_record(record) for record in patterns]
    for p, record in enumerate(decoded):
        typing = record[1] & TYPING
        for a in sorted(props):
            verdict, steps = search(record, props, nbrs, a)
            if steps_out is not None:
                steps_out[(p, a)] = (verdict, steps)
            over += verdict < 0
            if verdict == 1:
                hits[p] += 1
                if typing and types[a] < 0:
                    types[a] = p
    sums = [0, 0]
    for a, t in enumerate(types):
        if t >= 0:
            values = decoded[t][2]
            for c in range(2):
                sums[c] += values[2 * c] + props[a]["h"] * values[2 * c + 1]
    typed = sum(t >= 0 for t in types)
    mol = [0, len(props), typed, len(props) - typed, sums[0] & 0xFFFFFFFF, sums[1] & 0xFFFFFFFF, sum(h > 0 for h in hits), over]
    return dict(mol=mol, hits=hits, types=types)


def match_batch(mols, descs, patterns, bond_rows, atom_sets):
    """`mols`: the dicts of `decode_graph_ref.decode_labels`; `descs`: `mol_desc_ref.describe_batch` of them."""
    return [match(m["atoms"], m["bonds"], d, patterns, bond_rows, atom_sets) for m, d in zip(mols, descs)]


def lipinski_rules5(vmol, desc, mol):
    """`vmol`: the validity row, `desc`: the descriptor row, `mol`: the row of this module."""
    s0 = mol[4] - (1 << 32) if mol[4] >> 31 else mol[4]
    logp = -20000 <= s0 <= 50000 and mol[3] == 0 and mol[7] == 0
    return (int(vmol[5] < 5000000) + int(vmol[6] <= 5) + int(vmol[7] <= 10) + int(desc[2] <= 10) + int(logp)) * (desc[0] == 0)


def assert_batch_equals(host, want):
    """Every `mol` field, every hit count and every atom type of a host `MoleculeMatches` against the restatement's list, with
    `==`."""
    assert host.B == len(want)
    for b, w in enumerate(want):
        got = host.mol[b].tolist()
        signed = [(v & 0xFFFFFFFF) - ((v & 0x80000000) << 1) for v in w["mol"]]      # (the sums are modulo 2^32)
        assert got == signed, (b, dict(zip(MOL_FIELDS, got)), w["mol"])
        assert host.hits[b].tolist() == w["hits"], b
        assert host.atom_type[b].tolist() == w["types"], b


# ---- the lattice of the step bound -----------------------------------------------------------------------------------------------
def lattice(side):
    """A side x side square lattice of single-bonded atoms of label 1 (degree 4 inside): (atoms, rows (hi, lo, 1)), rows in the
    decode's order (ascending hi, then lo)."""
    at = lambda r, c: r * side + c
    rows = []
    for r in range(side):
        for c in range(side):
            if c:
                rows.append((at(r, c), at(r, c - 1), 1))
            if r:
                rows.append((at(r, c), at(r - 1, c), 1))
    return [1] * (side * side), sorted(rows)


def lattice_described(side):
    """The descriptor record a valid lattice would have -- written down directly, since the lattice's interior carbons have
    four bonds and no hydrogen: key = label 1, h = 4 - deg, n1 = deg; every bond a ring bond but none when side == 1."""
    atoms, rows = lattice(side)
    deg = [0] * len(atoms)
    for i, j, _ in rows:
        deg[i] += 1
        deg[j] += 1
    keys = [1 | (4 - d) << 8 | d << 12 for d in deg]
    return atoms, rows, dict(desc=[0, len(atoms)] + [0] * 10, keys=keys, classes=[BOND | RING_BOND] * len(rows))
