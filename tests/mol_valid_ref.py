"""Plain-Python restatement of `dg_mol_validity` (include/druggen_hip_valid.h), written from the header's comment alone: Python
integers, bridges by removing each bond and testing whether its ends stay connected (as tests/mol_fp_ref.py does), and the
maximum matching of the aromatic graph by exhaustive branching with a memo per connected component -- no augmenting paths, no
blossoms, no spanning tree: the kernel (csrc/mol_valid.hip, csrc/mol_match.h) uses all three, so the two sides cannot share a
mistake.  Components of more than 24 vertices are refused.  The molecules are the per-molecule dicts of
tests/decode_graph_ref.py (`decode_labels`)."""
from functools import lru_cache

import numpy as np

from mol_fp_ref import _connected, scope_atoms, scope_bonds

WHOLE, LARGEST = 0, 1
VALID, NO_GRAPH, EMPTY, UNKNOWN_LABEL, OVER_VALENT, AROMATIC_NOT_IN_RING, NOT_KEKULISABLE = 0, -2, 1, 2, 3, 4, 5
MOL_FIELDS = ("status", "n_atoms", "n_over", "deficiency", "n_h", "mass", "n_donors", "n_acceptors")
H_MASS = 10078
MAX_COMPONENT = 24

# the tables of the tests: labels 0..6 are pad, C, N, O, S, Cl, Se (mol_fp_ref.ATOM_DECODER); bond labels 0..4 none, single,
# double, triple, aromatic (mol_fp_ref.BOND_DECODER)
S_VALENCES = 2 | 4 << 8 | 6 << 16
ATOM_ROWS = [(0, 0, 0, 0), (4, 120000, 0, 0), (3, 140031, 1, 0), (2, 159949, 1, 0), (S_VALENCES, 319721, 0, 0),
             (1, 349689, 0, 0), (S_VALENCES, 799165, 0, 0)]
BOND_ROWS = [0, 1, 2, 3, 1 | 1 << 8]


def allowed_valences(word):
    """The allowed valences of an atom row's first word, or None for an UNKNOWN row."""
    b = [(word >> (8 * k)) & 255 for k in range(4)]
    if b[0] == 0 or any(v > 8 for v in b):
        return None
    return b[:b.index(0)] if 0 in b else b


def bond_row(word):
    """(order, aromatic) of a bond row, or None for an UNKNOWN row."""
    order, aromatic = word & 255, (word >> 8) & 1
    if order == 0 or order > 3 or word >> 9 or (aromatic and order != 1):
        return None
    return order, aromatic


def _components(vertices, edges):
    nbrs = {v: set() for v in vertices}
    for i, j in edges:
        nbrs[i].add(j)
        nbrs[j].add(i)
    seen, out = set(), []
    for v in sorted(vertices):
        if v in seen:
            continue
        comp, stack = [], [v]
        seen.add(v)
        while stack:
            x = stack.pop()
            comp.append(x)
            for y in nbrs[x]:
                if y not in seen:
                    seen.add(y)
                    stack.append(y)
        out.append(sorted(comp))
    return out, nbrs


def max_matching_size(vertices, edges):
    """The number of edges of a maximum matching: per connected component, the first vertex left is either left free or
    matched with one of its neighbours still there -- every possibility, memoised on the set of vertices left."""
    total = 0
    comps, nbrs = _components(vertices, edges)
    for comp in comps:
        if len(comp) > MAX_COMPONENT:
            raise ValueError(f"an aromatic component of {len(comp)} vertices: the restatement stops at {MAX_COMPONENT}")
        at = {v: k for k, v in enumerate(comp)}
        masks = [sum(1 << at[y] for y in nbrs[v]) for v in comp]

        @lru_cache(maxsize=None)
        def best(left):
            if left == 0:
                return 0
            v = (left & -left).bit_length() - 1
            rest = left & ~(1 << v)
            options = masks[v] & rest
            if not options:
                return best(rest)
            found = best(rest)
            while options:
                u = (options & -options).bit_length() - 1
                options &= options - 1
                found = max(found, 1 + best(rest & ~(1 << u)))
            return found
        total += best((1 << len(comp)) - 1)
    return total


def analyse(atoms, rows, atom_rows=ATOM_ROWS, bond_rows=BOND_ROWS, scope=WHOLE, component=None, largest=None, h_mass=H_MASS,
            deficiency=None):
    """One molecule with a graph -> dict(mol=[8 ints], hcount=[N ints], and, past status 2, w0 / sigma / candidates / bonds).
    `deficiency`: the deficiency of the aromatic graph where it is known by construction (the families below at sizes the
    exhaustive matching refuses); everything else is still worked out here."""
    atoms = [int(a) for a in atoms]
    rows = [(int(i), int(j), int(l)) for i, j, l in rows]
    N = len(atoms)
    members = scope_atoms(atoms, rows, scope, component, largest)
    bonds = scope_bonds(atoms, rows, members)
    blank = [0xFF] * N

    def result(status, n_over=0, deficiency=-1, **more):
        return dict(mol=[status, len(members), n_over, deficiency, 0, 0, 0, 0], hcount=blank, members=members, bonds=bonds, **more)
    if not members:
        return result(EMPTY)
    valences = {a: allowed_valences(atom_rows[atoms[a]][0]) if atoms[a] < len(atom_rows) else None for a in members}
    kinds = [bond_row(bond_rows[l]) if l < len(bond_rows) else None for _, _, l in bonds]
    if any(v is None for v in valences.values()) or any(k is None for k in kinds):
        return result(UNKNOWN_LABEL)
    sigma, arom = {a: 0 for a in members}, {a: 0 for a in members}
    for (i, j, _), (order, aromatic) in zip(bonds, kinds):
        for a in (i, j):
            sigma[a] += order
            arom[a] += aromatic
    w0 = {a: min((v for v in valences[a] if v >= sigma[a]), default=None) for a in members}
    n_over = sum(1 for a in members if w0[a] is None)
    if n_over:
        return result(OVER_VALENT, n_over)
    at = {}
    for k, (i, j, _) in enumerate(bonds):
        at.setdefault(i, []).append(k)
        at.setdefault(j, []).append(k)
    if any(aromatic and not _connected(i, j, bonds, at, k) for k, ((i, j, _), (_, aromatic)) in enumerate(zip(bonds, kinds))):
        return result(AROMATIC_NOT_IN_RING)
    candidates = {a for a in members if arom[a] > 0 and w0[a] > sigma[a]}
    edges = [(i, j) for (i, j, _), (_, aromatic) in zip(bonds, kinds) if aromatic and i in candidates and j in candidates]
    if deficiency is None:
        deficiency = len(candidates) - 2 * max_matching_size(candidates, edges)
    more = dict(w0=w0, sigma=sigma, candidates=candidates, kinds=kinds)
    if deficiency:
        return result(NOT_KEKULISABLE, 0, deficiency, **more)
    h = {a: w0[a] - sigma[a] - (a in candidates) for a in members}
    n_h = sum(h.values())
    mass = (sum(atom_rows[atoms[a]][1] for a in members) + n_h * h_mass) & 0xFFFFFFFF
    polar = [a for a in members if atom_rows[atoms[a]][2] & 1]
    mol = [VALID, len(members), 0, 0, n_h, mass - (1 << 32) if mass >> 31 else mass, sum(1 for a in polar if h[a] >= 1), len(polar)]
    return dict(mol=mol, hcount=[h.get(a, 0xFF) for a in range(N)], members=members, bonds=bonds, **more)


def validity(atoms, rows, n_bonds=None, cap=None, flag=0, **kw):
    """One molecule as the entry sees it: status NO_GRAPH when the list is truncated (n_bonds > cap) or flag < 0."""
    rows = list(rows)
    n_bonds = len(rows) if n_bonds is None else n_bonds
    if (cap is not None and n_bonds > cap) or flag < 0:
        return dict(mol=[NO_GRAPH, 0, 0, -1, 0, 0, 0, 0], hcount=[0xFF] * len(atoms), members=set(), bonds=[])
    return analyse(atoms, rows[:max(n_bonds, 0)], **kw)


def validity_batch(mols, cap=None, scope=LARGEST, **kw):
    """`mols`: the dicts of `decode_graph_ref.decode_labels` -> one result per molecule."""
    return [validity(m["atoms"], m["bonds"], n_bonds=m["n_bonds"], cap=cap, scope=scope, component=m["component"],
                     largest=m["largest"], **kw) for m in mols]


def check_certificate(want, rows_in, kekule):
    """`kekule`: the [rows, 4] output rows of one molecule; `rows_in` its input rows (hi, lo, label); `want` the restatement's
    result.  The bytes (hi, lo, label) are the input's; the orders are all 0 unless the status is 0, and then: 0 exactly for
    the rows that are no BONDS, the table's order for a bond that is not aromatic, 1 or 2 for an aromatic one; every candidate
    has exactly one aromatic bond of order 2 and no other atom has one; the orders at `a` plus hcount[a] give w0[a]."""
    kekule = np.asarray(kekule).reshape(-1, 4).tolist()
    rows_in = [tuple(int(x) for x in r) for r in np.asarray(rows_in).reshape(-1, 3).tolist()]
    assert [tuple(r[:3]) for r in kekule] == rows_in[:len(kekule)] and len(kekule) <= len(rows_in)
    if want["mol"][0] != VALID:
        assert not any(r[3] for r in kekule)
        return
    assert len(kekule) == len(rows_in)
    kinds = {b: k for b, k in zip(want["bonds"], want["kinds"])}
    total = {a: 0 for a in want["members"]}
    doubles = {a: 0 for a in want["members"]}
    for hi, lo, label, order in kekule:
        kind = kinds.get((hi, lo, label))
        if kind is None:
            assert order == 0, (hi, lo, label, order)
            continue
        assert order in (1, 2) if kind[1] else order == kind[0], (hi, lo, label, order)
        for a in (hi, lo):
            total[a] += order
            doubles[a] += kind[1] and order == 2
    for a in want["members"]:
        assert doubles[a] == (a in want["candidates"]), a
        assert total[a] + want["hcount"][a] == want["w0"][a], a


def assert_batch_equals(host, want, mols=None):
    """Every `mol` field and `hcount` of a host `MoleculeValidity` against the restatement's list, with `==`; with `mols` (the
    input dicts) also the Kekule certificate of every molecule."""
    assert host.B == len(want)
    for b, w in enumerate(want):
        got = host.mol[b].tolist()
        assert got == w["mol"], (b, dict(zip(MOL_FIELDS, got)), dict(zip(MOL_FIELDS, w["mol"])))
        assert host.hcount[b].tolist() == w["hcount"], b
        if mols is not None:
            m = mols[b]
            check_certificate(w, m["bonds"], host.kekule[b, :max(min(m["n_bonds"], host.cap), 0)])


# ---- graph families: (atoms [N], labels [N,N] lower triangle) over the tables above -----------------------------------------
def _bond(labels, i, j, label):
    labels[max(i, j), min(i, j)] = label


def _grow_ring(labels, x, y, first, size, label):
    """Close a ring of `size` atoms over the bond (or the future bond) x-y with the new atoms first .. first + size - 3."""
    path = [x] + list(range(first, first + size - 2)) + [y]
    for u, v in zip(path, path[1:]):
        _bond(labels, u, v, label)
    return path[1:-1]


def fused_chain(sizes, N, first=0, out=None):
    """Rings of the given sizes, all aromatic carbon, each fused to the one before over a bond between two of that ring's own new
    atoms: no atom lies on two fusion bonds, so every atom is on the perimeter, which is a Hamiltonian cycle.  Hence the
    aromatic graph (every atom is a candidate: sigma 2 or 3 < 4) has a perfect matching when the atom count is even -- every
    second perimeter bond -- and a maximum matching that leaves exactly one atom when it is odd (the perimeter without that
    atom is a path with an even number of vertices; one atom must stay free by parity).  Returns (atoms, labels, atoms used)."""
    atoms, labels = out if out is not None else (np.zeros(N, dtype=np.int64), np.zeros((N, N), dtype=np.int64))
    new = list(range(first, first + sizes[0]))
    for u, v in zip(new, new[1:] + new[:1]):
        _bond(labels, u, v, 4)
    used = first + sizes[0]
    for size in sizes[1:]:
        k = len(new) // 2 - 1
        new = _grow_ring(labels, new[k], new[k + 1], used, size, 4)
        used += size - 2
    assert used <= N
    atoms[first:used] = 1
    return atoms, labels, used


def chain_atoms(sizes):
    return sizes[0] + sum(s - 2 for s in sizes[1:])


def disjoint(systems, N):
    """Several fused chains side by side in one molecule of N positions (the rest stays pads): [(sizes), ...]."""
    out = np.zeros(N, dtype=np.int64), np.zeros((N, N), dtype=np.int64)
    used = 0
    for sizes in systems:
        _, _, used = fused_chain(sizes, N, used, out)
    return out[0], out[1], used


def rotated(atoms, labels, shift):
    """The same labelled graph with atom i at position (i + shift) mod N."""
    N = len(atoms)
    perm = (np.arange(N) - shift) % N                    # new position p holds old atom perm[p]
    full = labels + labels.T
    return np.asarray(atoms)[perm], np.tril(full[np.ix_(perm, perm)], -1)


def renumbered(rng, atoms, labels):
    """The same labelled graph with its atoms in a random order, and the order: new position p holds old atom perm[p]."""
    N = len(atoms)
    perm = rng.permutation(N)
    full = labels + labels.T
    return np.asarray(atoms)[perm], np.tril(full[np.ix_(perm, perm)], -1), perm


def aromatic_like(rng, N, clean=False):
    """A molecule-like graph: chain atoms and rings of 5, 6 or 7 atoms -- most of them aromatic -- hung on a random tree or fused
    to the ring before them (at most three in a row: no aromatic component above 7 + 5 + 5 atoms), hetero atoms in the rings,
    double bonds in the chains; a substituent goes where a valence is free.  `clean`: five-rings carry an O, S or Se, seven-rings
    are not aromatic, an aromatic ring is fused to aromatic rings only and nothing else is done -- most such molecules are valid.  Otherwise odd carbon rings occur, and now and
    then a defect: an aromatic bond on a chain, a bonded pad, one more bond.  Valid, not kekulisable, over-valent,
    aromatic-outside-a-ring and unknown-label molecules all occur."""
    atoms, labels = np.zeros(N, dtype=np.int64), np.zeros((N, N), dtype=np.int64)
    free = np.zeros(N, dtype=np.int64)
    room_of = {1: 4, 2: 3, 3: 2, 4: 2, 5: 1, 6: 2}

    def anchor_for(n, need):
        near = [a for a in range(max(0, n - 6), n) if free[a] >= need]
        far = near or [a for a in range(n) if free[a] >= need]
        return int(rng.choice(far)) if far else None

    n, last_new, last_label, run = 0, None, 0, 0
    while n < N:
        room = N - n
        if room < 5 or rng.random() < 0.35:                       # a chain atom
            atoms[n] = rng.choice([1, 1, 1, 2, 3, 5])
            free[n] = room_of[int(atoms[n])]
            order = 2 if atoms[n] in (1, 3) and rng.random() < 0.15 else 1
            anchor = anchor_for(n, order)
            if anchor is not None:
                _bond(labels, n, anchor, order)
                free[n] -= order
                free[anchor] -= order
            n, last_new, run = n + 1, None, 0
            continue
        size = int(rng.choice([s for s in (5, 6, 6, 7) if s <= room]))
        label = 4 if rng.random() < 0.75 and not (clean and size == 7) else 1
        if last_new is not None and run < 3 and rng.random() < 0.5 and not (clean and label != last_label):      # fused over a bond between two new atoms of the last ring
            k = len(last_new) // 2 - 1
            new = _grow_ring(labels, last_new[k], last_new[k + 1], n, size, label)
            free[[last_new[k], last_new[k + 1]]] = 0
            n, run = n + size - 2, run + 1
        else:
            new = list(range(n, n + size))
            for u, v in zip(new, new[1:] + new[:1]):
                _bond(labels, u, v, label)
            anchor = anchor_for(n, 1)
            n, run = n + size, 1
        atoms[new] = 1
        free[new] = 1 if label == 4 else 2
        if label == 4:
            if size == 5 and (clean or rng.random() < 0.6):
                hetero = new[len(new) // 2 + 1]                   # not on the bond the next ring fuses over
                atoms[hetero] = rng.choice([3, 4, 6])
                free[hetero] = 0
            for a in new:
                if atoms[a] == 1 and rng.random() < 0.12:
                    atoms[a], free[a] = 2, 0
        if run == 1 and anchor is not None and free[new[0]] >= 1:
            _bond(labels, new[0], anchor, 1)
            free[new[0]] -= 1
            free[anchor] -= 1
        last_new, last_label = new, label
    if not clean and N >= 2:
        dice = rng.random()
        pairs = np.argwhere(labels == 1)
        if dice < 0.15 and len(pairs):
            i, j = pairs[rng.integers(len(pairs))]
            labels[i, j] = 4
        elif dice < 0.25:
            atoms[rng.integers(N)] = 0
        elif dice < 0.4:
            i, j = sorted(rng.integers(0, N, 2).tolist(), reverse=True)
            if i != j and labels[i, j] == 0:
                labels[i, j] = rng.choice([1, 2])
    return atoms, labels
