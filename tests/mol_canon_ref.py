"""Plain-Python restatement of `dg_mol_canon` and `dg_mol_canon_match` (include/druggen_hip.h), written from their
specification: loops, `sorted()` and Python integers modulo 2^64.  No keys in the matching: forms are compared as tuples in a
double loop.  The molecules are the per-molecule dicts of tests/decode_graph_ref.py (`decode_labels`).  Also the graph families
the host and GPU tests share."""
from bisect import bisect_left
from collections import Counter

import numpy as np

M64 = (1 << 64) - 1
WHOLE, LARGEST = 0, 1


def mix64(z):
    """splitmix64's finaliser."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix(pos, value):
    return mix64(((pos + 1) << 32) | value)


def _ranks(keys):
    """c[i] = number of keys strictly smaller than keys[i]."""
    ordered = sorted(keys)
    return [bisect_left(ordered, k) for k in keys]


def canon(atoms, bonds, component=None, largest=None, scope=LARGEST):
    """One molecule: atoms [N], bonds [(i, j, label)], and for scope LARGEST the decode's component [N] and largest.  Returns a
    dict: n_atoms, n_bonds, n_splits, n_rounds, order [n], canon_atoms [n], canon_bonds [(hi, lo, label)], key (signed)."""
    atoms = [int(a) for a in atoms]
    bonds = [(int(i), int(j), int(l)) for i, j, l in np.asarray(bonds).reshape(-1, 3).tolist()]
    N = len(atoms)
    if scope == LARGEST:
        S = [i for i in range(N) if int(component[i]) == int(largest)]
    else:
        bonded = {i for i, _, _ in bonds} | {j for _, j, _ in bonds}
        S = [i for i in range(N) if atoms[i] != 0 or i in bonded]
    n = len(S)
    at = {p: m for m, p in enumerate(S)}                 # position -> index into S
    inside = [(at[i], at[j], l) for i, j, l in bonds if i in at and j in at]
    nbrs = [[] for _ in range(n)]
    for i, j, l in inside:
        nbrs[i].append((j, l))
        nbrs[j].append((i, l))

    c = _ranks([atoms[p] for p in S])
    splits = rounds = 0
    for _ in range(n):
        settled = False
        for _ in range(n):
            sig = [sum(mix64((l << 16) | c[j]) for j, l in nbrs[i]) & M64 for i in range(n)]
            new = _ranks(list(zip(c, sig)))
            rounds += 1
            if new == c:
                settled = True
                break
            c = new
        assert settled
        count = Counter(c)
        shared = sorted(v for v in count if count[v] > 1)
        if not shared:
            break
        cell = [i for i in range(n) if c[i] == shared[0]]
        for i in cell[1:]:                               # S is ascending in position: cell[0] has the smallest
            c[i] += 1
        splits += 1
    assert sorted(c) == list(range(n))

    order, canon_atoms = [0] * n, [0] * n
    for i in range(n):
        order[c[i]] = S[i]
        canon_atoms[c[i]] = atoms[S[i]]
    canon_bonds = sorted((max(c[i], c[j]), min(c[i], c[j]), l) for i, j, l in inside)
    key = (mix(256, n) + mix(257, len(canon_bonds))) & M64
    for r, a in enumerate(canon_atoms):
        key = (key + mix(r, a)) & M64
    for k, (hi, lo, l) in enumerate(canon_bonds):
        key = (key + mix(258 + k, hi | lo << 8 | l << 16)) & M64
    return dict(n_atoms=n, n_bonds=len(canon_bonds), n_splits=splits, n_rounds=rounds, order=order, canon_atoms=canon_atoms,
                canon_bonds=canon_bonds, key=key - (1 << 64) if key >> 63 else key)


TRUNCATED = dict(n_atoms=0, n_bonds=0, n_splits=-2, n_rounds=0, order=[], canon_atoms=[], canon_bonds=[], key=0)


def canon_batch(mols, cap=None, scope=LARGEST):
    """The forms of the molecule dicts `mols` (list); `cap`: rows of the bond list (None: nothing is truncated)."""
    return [dict(TRUNCATED) if cap is not None and m["n_bonds"] > cap else
            canon(m["atoms"], m["bonds"], m["component"], m["largest"], scope) for m in mols]


def form_of(f):
    """What two forms are compared by; None: truncated."""
    if f["n_splits"] < 0:
        return None
    return f["n_atoms"], f["n_bonds"], tuple(f["canon_atoms"]), tuple(map(tuple, f["canon_bonds"]))


def match(forms, stock=None):
    """(match [B,2] int32, tot [8] int64) of a list of forms against itself and a list of stock forms (None or empty: none)."""
    B = len(forms)
    mine = [form_of(f) for f in forms]
    theirs = [form_of(f) for f in stock] if stock else []
    out = np.zeros((B, 2), dtype=np.int32)
    for b in range(B):
        if mine[b] is None:
            out[b] = -2
            continue
        out[b, 0] = next((j for j in range(b) if mine[j] == mine[b]), -1)
        out[b, 1] = next((k for k in range(len(theirs)) if theirs[k] == mine[b]), -1) if theirs else -3
    tot = np.zeros(8, dtype=np.int64)
    tot[0] = B
    tot[1] = int((out[:, 0] == -1).sum())
    tot[2] = int((out[:, 1] >= 0).sum())
    tot[3] = int((out[:, 1] == -1).sum())
    tot[4] = sum(1 for f in forms if f["n_splits"] < 0)
    tot[5] = sum(1 for f in forms if f["n_splits"] == 0)
    return out, tot


def assert_forms_equal(host, want):
    """Every field of a host `CanonicalForms` against the restatement's list, with `==`, fillers included."""
    assert host.B == len(want)
    for b, w in enumerate(want):
        where = f"molecule {b}"
        got = (int(host.n_atoms[b]), int(host.n_bonds[b]), int(host.n_splits[b]), int(host.n_rounds[b]), int(host.key[b]))
        assert got == (w["n_atoms"], w["n_bonds"], w["n_splits"], w["n_rounds"], w["key"]), (where, got, w)
        n, nb = w["n_atoms"], w["n_bonds"]
        assert host.order[b, :n].tolist() == w["order"] and (host.order[b, n:] == 0xFF).all(), where
        assert host.canon_atoms[b, :n].tolist() == w["canon_atoms"] and (host.canon_atoms[b, n:] == 0xFF).all(), where
        assert [tuple(r) for r in host.canon_bonds[b, :nb, :3].tolist()] == w["canon_bonds"], where
        assert not host.canon_bonds[b, :nb, 3].any() and not host.canon_bonds[b, nb:].any(), where


def check_order(atoms, labels, order, canon_atoms, canon_bonds):
    """Soundness without the restatement: `order` is a list of distinct positions, and reading the INPUT (atoms [N], dense
    labels [N,N], lower triangle) through it gives exactly `canon_atoms` and `canon_bonds` -- the form is the input relabelled."""
    n = len(order)
    assert len(set(order)) == n
    assert [int(atoms[p]) for p in order] == list(canon_atoms)
    rows = []
    for hi in range(n):
        for lo in range(hi):
            p, q = order[hi], order[lo]
            l = int(labels[max(p, q)][min(p, q)])
            if l:
                rows.append((hi, lo, l))
    assert rows == [tuple(r) for r in canon_bonds]


# ---- graph families: (atoms [N], labels [N,N] lower triangle) ---------------------------------------------------------------
def molecule_like(rng, N, closures, one_label=False):
    """A random tree -- atom i bonds to one of the (up to) 4 atoms before it -- with atom labels from {1,1,1,1,2,3} and bond
    labels from {1,1,1,2}, then `closures` ring closures labelled 1 or 4.  `one_label`: label 1 everywhere."""
    atoms = np.ones(N, dtype=np.int64) if one_label else rng.choice([1, 1, 1, 1, 2, 3], N)
    labels = np.zeros((N, N), dtype=np.int64)
    for i in range(1, N):
        labels[i, rng.integers(max(0, i - 4), i)] = 1 if one_label else rng.choice([1, 1, 1, 2])
    for _ in range(closures if N >= 3 else 0):
        for _ in range(8):
            i, j = sorted(rng.integers(0, N, 2).tolist(), reverse=True)
            if i != j and labels[i, j] == 0:
                labels[i, j] = 1 if one_label else rng.choice([1, 4])
                break
    return atoms, labels


def renumbered(rng, atoms, labels):
    """The same labelled graph with its atoms in a random order."""
    N = len(atoms)
    perm = rng.permutation(N)                            # new position p holds old atom perm[p]
    full = labels + labels.T
    return np.asarray(atoms)[perm], np.tril(full[np.ix_(perm, perm)], -1)


def from_edges(N, edges, label=1, atom=1):
    atoms = np.full(N, atom, dtype=np.int64)
    labels = np.zeros((N, N), dtype=np.int64)
    for i, j in edges:
        labels[max(i, j), min(i, j)] = label
    return atoms, labels


def cycle(N, label=1, atom=1):
    return from_edges(N, [(i, (i + 1) % N) for i in range(N)] if N >= 3 else [], label, atom)


def decalin():
    """Two six-rings sharing a bond: 10 atoms, 11 bonds."""
    return from_edges(10, [(i, i + 1) for i in range(9)] + [(9, 0), (4, 9)])


def bicyclopentyl():
    """Two five-rings joined by a bond: 10 atoms, 11 bonds, the same degrees and the same refinement colours as decalin."""
    return from_edges(10, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (5, 6), (6, 7), (7, 8), (8, 9), (9, 5), (4, 9)])


# (N, ring closures, one label everywhere) of the fixed-seed molecule-like family: a lone atom, a pair, odd sizes, the wave
# boundary at 64 / 65
MOLECULE_FAMILY = [(N, closures, one_label) for one_label in (False, True) for N in (1, 2, 5, 9, 17, 33, 45, 64, 65)
                   for closures in (0, 1, 2, 4)]
