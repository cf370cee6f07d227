"""Plain-Python restatement of `dg_mol_fingerprint` (include/druggen_hip_fp.h), written from the header's comment alone: Python
integers masked to 64 bits, environments as explicit `frozenset`s of bonds, distances by breadth-first search, the ring flag
by removing each bond and testing whether its ends stay connected.  Deliberately no atom-set stand-in for an environment and no
spanning tree: the kernel (csrc/mol_fp.hip) uses both, so the two sides cannot share a mistake.  The molecules are the
per-molecule dicts of tests/decode_graph_ref.py (`decode_labels`)."""
import numpy as np

M64 = (1 << 64) - 1
WHOLE, LARGEST = 0, 1
NO_GRAPH = -2
MAX_RADIUS = 4
NO_ROW = 0xFFFFFFFF

# the tables of the tests: labels 0..6 are pad, C, N, O, S, Cl, Se; bond labels 0..4 none, single, double, triple, aromatic
ATOM_DECODER = {0: 0, 1: 6, 2: 7, 3: 8, 4: 16, 5: 17, 6: 34}
BOND_DECODER = {0: 0, 1: 1, 2: 2, 3: 3, 4: 12}
ATOM_WORDS = [0, 6, 7, 8, 16, 17, 34]
BOND_ROWS = [(0, 0), (1, 2), (2, 4), (3, 6), (12, 3)]


def mix64(z):
    """splitmix64's finaliser."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def scope_atoms(atoms, rows, scope, component=None, largest=None):
    N = len(atoms)
    if scope == LARGEST:
        return {i for i in range(N) if int(component[i]) == int(largest)}
    bonded = {e for i, j, _ in rows if i < N and j < N and i != j for e in (i, j)}
    return {i for i in range(N) if int(atoms[i]) != 0 or i in bonded}


def scope_bonds(atoms, rows, members):
    N = len(atoms)
    return [(i, j, l) for i, j, l in rows if i < N and j < N and i != j and i in members and j in members]


def _connected(u, v, bonds, at, skip):
    """Is there a walk from u to v that does not use bond `skip`?"""
    seen, stack = {u}, [u]
    while stack:
        x = stack.pop()
        for k in at[x]:
            if k == skip:
                continue
            i, j, _ = bonds[k]
            y = j if x == i else i
            if y == v:
                return True
            if y not in seen:
                seen.add(y)
                stack.append(y)
    return False


def ring_flags(N, bonds):
    """ring[a]: one of a's bonds is not a bridge -- its ends stay connected without it."""
    at = {}
    for k, (i, j, _) in enumerate(bonds):
        at.setdefault(i, []).append(k)
        at.setdefault(j, []).append(k)
    ring = [0] * N
    for k, (i, j, _) in enumerate(bonds):
        if _connected(i, j, bonds, at, k):
            ring[i] = ring[j] = 1
    return ring


def _distances(a, neighbours, limit):
    dist, layer = {a: 0}, [a]
    for d in range(1, limit + 1):
        nxt = []
        for x in layer:
            for y in neighbours[x]:
                if y not in dist:
                    dist[y] = d
                    nxt.append(y)
        layer = nxt
    return dist


def features(atoms, rows, radius, atom_words=ATOM_WORDS, bond_rows=BOND_ROWS, scope=WHOLE, component=None, largest=None,
             detail=False):
    """The feature set F of one molecule as a Python set of 64-bit integers (`detail`: also ids per layer, ring, members)."""
    atoms = [int(a) for a in atoms]
    rows = [(int(i), int(j), int(l)) for i, j, l in rows]
    N = len(atoms)
    members = scope_atoms(atoms, rows, scope, component, largest)
    bonds = scope_bonds(atoms, rows, members)
    aw = lambda l: atom_words[l] if l < len(atom_words) else NO_ROW
    bw = lambda l: bond_rows[l][0] if l < len(bond_rows) else NO_ROW
    o2 = lambda l: bond_rows[l][1] if l < len(bond_rows) else 0
    of = {a: [] for a in members}      # the bonds of a, as indices into `bonds`
    for k, (i, j, _) in enumerate(bonds):
        of[i].append(k)
        of[j].append(k)
    neighbours = {a: [bonds[k][1] if bonds[k][0] == a else bonds[k][0] for k in of[a]] for a in members}
    ring = ring_flags(N, bonds)
    ids = [{}]
    for a in members:
        t = mix64(aw(atoms[a]))
        t = mix64((t + len(of[a])) & M64)
        t = mix64((t + (sum(o2(bonds[k][2]) for k in of[a]) & 0xFFFFFFFF)) & M64)
        ids[0][a] = mix64((t + ring[a]) & M64)
    F = set(ids[0].values())
    seen = set()
    for r in range(1, radius + 1):
        prev, now = ids[-1], {}
        for a in members:
            s = 0
            for k in of[a]:
                i, j, l = bonds[k]
                x = j if i == a else i
                s = (s + mix64((prev[x] + mix64(bw(l))) & M64)) & M64
            now[a] = mix64((mix64((prev[a] + r) & M64) + s) & M64)
        ids.append(now)
        fresh = {}
        for a in members:
            if not of[a]:
                continue
            near = _distances(a, neighbours, r - 1)
            env = frozenset(k for k, (i, j, _) in enumerate(bonds) if i in near or j in near)
            if env and env not in seen:
                fresh[env] = min(fresh.get(env, M64), now[a])
        seen.update(fresh)
        F.update(fresh.values())
    if detail:
        return F, ids, ring, members
    return F


def folded(F, nbits):
    """A feature set (None: no graph) -> dict(words: nbits / 32 unsigned ints, count, n_features)."""
    words = [0] * (nbits // 32)
    if F is None:
        return dict(words=words, count=0, n_features=NO_GRAPH)
    for v in F:
        k = v % nbits
        words[k // 32] |= 1 << (k % 32)
    return dict(words=words, count=sum(bin(w).count("1") for w in words), n_features=len(F))


def feature_set(atoms, rows, radius=2, n_bonds=None, cap=None, flag=0, **kw):
    """F of one molecule as the entry sees it: None when the list is truncated (n_bonds > cap) or flag < 0."""
    rows = list(rows)
    n_bonds = len(rows) if n_bonds is None else n_bonds
    if (cap is not None and n_bonds > cap) or flag < 0:
        return None
    return features(atoms, rows[:max(n_bonds, 0)], radius, **kw)


def fingerprint(atoms, rows, radius=2, nbits=1024, **kw):
    """One molecule -> dict(words, count, n_features)."""
    return folded(feature_set(atoms, rows, radius, **kw), nbits)


def feature_sets(mols, radius=2, cap=None, scope=LARGEST, **kw):
    """`mols`: the dicts of `decode_graph_ref.decode_labels` -> one F (or None) per molecule."""
    return [feature_set(m["atoms"], m["bonds"], radius, n_bonds=m["n_bonds"], cap=cap, scope=scope, component=m["component"],
                        largest=m["largest"], **kw) for m in mols]


def fingerprint_batch(mols, radius=2, nbits=1024, cap=None, scope=LARGEST, **kw):
    return [folded(F, nbits) for F in feature_sets(mols, radius, cap, scope, **kw)]


def bit_set(result):
    return {32 * w + k for w, word in enumerate(result["words"]) for k in range(32) if (word >> k) & 1}


def assert_batch_equals(words, counts, n_features, want):
    """Device outputs as numpy arrays (words int32) against the restatement's list, with `==`."""
    assert len(want) == len(counts) == len(n_features) == len(words)
    got = np.asarray(words).view(np.uint32)
    for b, w in enumerate(want):
        assert int(n_features[b]) == w["n_features"], (b, int(n_features[b]), w["n_features"])
        assert int(counts[b]) == w["count"], (b, int(counts[b]), w["count"])
        assert got[b].tolist() == w["words"], b


def tanimoto(a, b):
    """The reference's quotient on two bit sets as float32 (0 / 0 taken as 1)."""
    c = len(a & b)
    union = len(a) + len(b) - c
    return np.float32(1.0) if union == 0 else np.float32(c) / np.float32(union)
