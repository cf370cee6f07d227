"""Plain-Python restatement of `dg_mol_scaffold` (include/druggen_hip_scaf.h), written from the header's comment alone: Python
integers, sets and dicts; the core by removing ONE atom of degree <= 1 at a time until none is left (the kernel drops all of
them per round over bit rows); bridges by removing each bond and asking whether its ends stay connected, held against the ring
bit of the class the descriptors gave it; the ring size of a ring bond by a breadth-first search over dicts of neighbours
without the bond; ring systems by a flood fill.  Its inputs are the restatements' results: the descriptor record of
tests/mol_desc_ref.py (`describe`: status, keys, classes) for the same molecule, never the GPU's outputs.  The derived batch is
tests/decode_graph_ref.py's `decode_labels` of the scaffold graph."""
from collections import Counter

import numpy as np

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_valid_ref as vref

MOL_FIELDS = ("status", "n_heavy", "n_scaffold_atoms", "n_scaffold_bonds", "n_exo", "n_linker_atoms", "n_ring_atoms", "n_ring_bonds",
              "n_rings", "n_ring_systems", "largest_system_atoms", "min_ring", "max_ring")
N_MOL, HIST_BINS, MAX_RING, NO_SYSTEM = 16, 8, 255, 255
NONE, SIDE, EXO, LINKER, RING = 0, 1, 2, 3, 4
NO_KEY = 0xFFFFFFFF
BOND, RING_BOND = 1, 2


def hist_bin(size):
    return size - 3 if size <= 8 else 6 if size <= 12 else 7


def _reaches(u, v, nbrs, skip):
    """The number of bonds of the shortest path from u to v that does not use the bond `skip` = {u, v}; None if there is none."""
    seen, front, steps = {u}, [u], 0
    while front:
        steps += 1
        nxt = []
        for x in front:
            for y in nbrs[x]:
                if {x, y} == skip or y in seen:
                    continue
                if y == v:
                    return steps
                seen.add(y)
                nxt.append(y)
        front = nxt
    return None


def empty(status, N, n_rows):
    return dict(mol=[status] + [0] * (N_MOL - 1), hist=[0] * HIST_BINS, role=[NONE] * N, system=[NO_SYSTEM] * N, sizes=[0] * n_rows,
                s_atoms=[0] * N, s_rows=[], derived=dref.decode_labels([0] * N, np.zeros((N, N), dtype=np.int64)))


def scaffold(atoms, rows, described, bond_rows=vref.BOND_ROWS, inside=True):
    """One molecule -> dict(mol=[16], hist=[8], role=[N], system=[N], sizes=[rows read], s_atoms=[N], s_rows=[(hi, lo, label)],
    derived=decode_labels of the scaffold graph).  `described`: mol_desc_ref's result for it (status, keys, classes); `rows`: the
    bond rows the classes belong to.  `inside`: the input is inside the definition -- the ring bits are then held against
    bridges found by removal."""
    atoms = [int(a) for a in atoms]
    N = len(atoms)
    keys, classes = described["keys"], described["classes"]
    status = described["desc"][0]
    if status != 0:
        return empty(status, N, len(classes))
    rows = [tuple(int(x) for x in r[:3]) for r in rows][:len(classes)]
    scope = {a for a in range(N) if keys[a] != NO_KEY}
    bonds = {}      # row index -> (i, j, label, order, aromatic, ring)
    for k, ((i, j, l), cls) in enumerate(zip(rows, classes)):
        if not cls & BOND or i >= N or j >= N or i == j or i not in scope or j not in scope:
            continue
        kind = vref.bond_row(bond_rows[l]) if l < len(bond_rows) else None
        if kind is None:
            continue
        bonds[k] = (i, j, l, kind[0], kind[1], bool(cls & RING_BOND))
    nbrs = {a: set() for a in scope}
    for i, j, *_ in bonds.values():
        assert j not in nbrs[i], "outside the definition: a pair twice"
        nbrs[i].add(j)
        nbrs[j].add(i)
    if inside:
        for i, j, _, _, _, ring in bonds.values():
            assert ring == (_reaches(i, j, nbrs, {i, j}) is not None), (i, j)

    # the core: one removal at a time
    core = set(scope)
    while True:
        loose = [a for a in sorted(core) if len(nbrs[a] & core) <= 1]
        if not loose:
            break
        core.remove(loose[0])
    exo = set()
    for i, j, _, order, aromatic, _ in bonds.values():
        if order == 2 and not aromatic:
            if i in core and j in scope - core:
                exo.add(j)
            if j in core and i in scope - core:
                exo.add(i)
    members = core | exo
    s_rows = [(i, j, l) for i, j, l, *_ in bonds.values() if i in members and j in members]

    ring_nbrs = {a: set() for a in scope}
    sizes = [0] * len(rows)
    hist = [0] * HIST_BINS
    for k, (i, j, _, _, _, ring) in bonds.items():
        if ring:
            ring_nbrs[i].add(j)
            ring_nbrs[j].add(i)
            steps = _reaches(i, j, nbrs, {i, j})
            sizes[k] = MAX_RING if steps is None else min(1 + steps, MAX_RING)
            hist[hist_bin(sizes[k])] += 1
    ringed = {a for a in scope if ring_nbrs[a]}
    system = [NO_SYSTEM] * N
    system_sizes = []
    for a in sorted(ringed):      # flood fill from the smallest atom not seen yet
        if system[a] != NO_SYSTEM:
            continue
        stack, seen = [a], {a}
        while stack:
            for y in ring_nbrs[stack.pop()]:
                if y not in seen:
                    seen.add(y)
                    stack.append(y)
        for y in seen:
            system[y] = a
        system_sizes.append(len(seen))
    role = [NONE if a not in scope else RING if a in ringed else LINKER if a in core else EXO if a in exo else SIDE for a in range(N)]
    ring_sizes = [s for s in sizes if s]
    mol = [0, len(scope), len(members), len(s_rows), len(exo), len(core - ringed), len(ringed), len(ring_sizes),
           len(ring_sizes) - len(ringed) + len(system_sizes), len(system_sizes), max(system_sizes, default=0),
           min(ring_sizes, default=0), max(ring_sizes, default=0), 0, 0, 0]
    s_atoms = [atoms[a] if a in members else 0 for a in range(N)]
    labels = np.zeros((N, N), dtype=np.int64)
    for i, j, l in s_rows:
        labels[max(i, j), min(i, j)] = l
    return dict(mol=mol, hist=hist, role=role, system=system, sizes=sizes, s_atoms=s_atoms, s_rows=s_rows,
                derived=dref.decode_labels(s_atoms, labels), core=core, exo=exo)


def scaffold_batch(mols, descs, bond_rows=vref.BOND_ROWS):
    """`mols`: the dicts of `decode_graph_ref.decode_labels`; `descs`: `mol_desc_ref.describe_batch` of them."""
    return [scaffold(m["atoms"], m["bonds"], d, bond_rows) for m, d in zip(mols, descs)]


def kept_forms(wants, min_rings=2):
    """Counter over the forms (mol_canon_ref.form_of, scope WHOLE of the derived graph) of the scaffolds that count: status 0,
    n_rings >= min_rings, not empty -- the reference's `compute_scaffolds`."""
    forms = Counter()
    for w in wants:
        if w["mol"][0] == 0 and w["mol"][8] >= min_rings and w["mol"][2] > 0:
            d = w["derived"]
            forms[cref.form_of(cref.canon(d["atoms"], d["bonds"], scope=cref.WHOLE))] += 1
    return forms


def similarity_counts(gen, stock, min_rings=2):
    """(dot, g2, r2) of two lists of restatement results: the sums `cos_similarity` is made of."""
    g, r = kept_forms(gen, min_rings), kept_forms(stock, min_rings)
    return sum(n * r.get(k, 0) for k, n in g.items()), sum(n * n for n in g.values()), sum(n * n for n in r.values())


def similarity(dot, g2, r2):
    """One product, one square root, one division in float64; nan when a side keeps nothing."""
    return float("nan") if g2 == 0 or r2 == 0 else dot / float(np.sqrt(np.float64(g2) * np.float64(r2)))


def assert_batch_equals(host, want, sentinel=None):
    """Every field of a host `MoleculeScaffolds` and of its derived host `MoleculeBatch` against the restatement's list, with
    `==`.  `sentinel`: the byte the buffers were pre-filled with -- the rows past both bond counts must still hold it."""
    assert host.B == len(want)
    for b, w in enumerate(want):
        got = host.mol[b].tolist()
        assert got == w["mol"], (b, dict(zip(MOL_FIELDS, got)), w["mol"])
        assert host.ring_hist[b].tolist() == w["hist"], b
        assert host.atom_role[b].tolist() == w["role"], b
        assert host.atom_system[b].tolist() == w["system"], b
        assert host.bond_ring_size[b, :len(w["sizes"])].tolist() == w["sizes"], b
        if sentinel is not None:
            assert (host.bond_ring_size[b, len(w["sizes"]):] == sentinel).all(), b
        # the scaffold's rows keep the order of the list they were cut from, which is the decode's order
        assert [tuple(r) for r in w["derived"]["bonds"].tolist()] == [(max(i, j), min(i, j), l) for i, j, l in w["s_rows"]], b
    dref.assert_batch_equals(host.batch, [w["derived"] for w in want], sentinel=sentinel)
