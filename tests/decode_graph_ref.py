"""CPU restatement of `dg_decode_graph` (include/druggen_hip.h), written from its specification: numpy argmax (first
maximum, NaN maximal), a plain walk over the lower triangle in row-major order, a plain union-find.  Also the small
structured graphs the host and GPU tests share, and a pure-Python copy of the bond walk of the reference's decoder
(`np.nonzero` over the dense matrix, keep `start > end`)."""
import numpy as np


def argmax_first(x):
    """Index of the first maximum over the last axis; NaN counts as maximal (numpy's rule, and torch.max's)."""
    return np.argmax(np.asarray(x), axis=-1)


class _UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, i):
        while self.parent[i] != i:
            self.parent[i] = self.parent[self.parent[i]]
            i = self.parent[i]
        return i

    def union(self, i, j):
        ri, rj = self.find(i), self.find(j)
        if ri != rj:
            self.parent[max(ri, rj)] = min(ri, rj)      # the root is always the smallest index of its set


def decode_labels(atoms, labels, order2=None):
    """One molecule from its labels: atoms [N], labels [N,N] (only i > j is read)."""
    N = len(atoms)
    rows = np.asarray(labels).tolist()      # plain lists: the walk below is a Python loop over N (N - 1) / 2 entries
    bonds = [(i, j, rows[i][j]) for i in range(N) for j in range(i) if rows[i][j] != 0]
    uf = _UnionFind(N)
    for i, j, _ in bonds:
        uf.union(i, j)
    component = np.array([uf.find(i) for i in range(N)], dtype=np.uint8)
    roots = sorted(set(component.tolist()))
    sizes = {r: int((component == r).sum()) for r in roots}
    largest = min(roots, key=lambda r: (-sizes[r], r))
    out = dict(atoms=np.asarray(atoms, dtype=np.uint8), bonds=np.array(bonds, dtype=np.uint8).reshape(-1, 3),
               n_bonds=len(bonds), component=component, n_components=len(roots), largest=largest,
               largest_size=sizes[largest], valence2=None)
    if order2 is not None:
        v = np.zeros(N, dtype=np.int64)
        for i, j, l in bonds:
            v[i] += int(order2[l])
            v[j] += int(order2[l])
        out["valence2"] = v.astype(np.uint16)
    return out


def decode_graph(node_logits, edge_logits, order2=None):
    """List of per-molecule dicts from float logits [B,N,M], [B,N,N,E]."""
    atoms, labels = argmax_first(node_logits), argmax_first(edge_logits)
    return [decode_labels(atoms[b], labels[b], order2) for b in range(atoms.shape[0])]


def assert_batch_equals(host, want, cap=None, sentinel=None):
    """Every field of a host `MoleculeBatch` against the restatement's list, with `==`.  `cap`: rows of the bond list (None =
    nothing truncated); `sentinel`: the byte the buffer was pre-filled with -- rows past the prefix must still hold it."""
    assert host.B == len(want)
    for b, w in enumerate(want):
        where = f"molecule {b}"
        assert np.array_equal(host.atoms[b], w["atoms"]), where
        assert int(host.n_bonds[b]) == w["n_bonds"], where
        kept = w["n_bonds"] if cap is None else min(cap, w["n_bonds"])
        assert np.array_equal(host.edge_list(b), w["bonds"][:kept]), where
        assert not host.bonds[b, :kept, 3].any(), where
        assert bool(host.truncated[b]) == (w["n_bonds"] > host.cap), where
        if sentinel is not None:
            assert (host.bonds[b, kept:] == sentinel).all(), where
        assert np.array_equal(host.component[b], w["component"]), where
        assert (int(host.n_components[b]), int(host.largest[b]), int(host.largest_size[b])) == \
            (w["n_components"], w["largest"], w["largest_size"]), where
        if w["valence2"] is not None:
            assert host.valence2 is not None and host.valence2.dtype == np.uint16
            assert np.array_equal(host.valence2[b], w["valence2"]), where


def reference_bond_walk(dense_labels):
    """The decoder's walk, copied in plain Python: `zip(*np.nonzero(labels))`, keep `start > end`."""
    return [(int(s), int(e), int(dense_labels[s, e])) for s, e in zip(*np.nonzero(dense_labels)) if s > e]


# ---- structured graphs: label matrices [N,N] (int), lower triangle unless said otherwise ----
def empty_graph(N):
    return np.zeros((N, N), dtype=np.int64)


def chain(order, label=1):
    """Path visiting the atoms in `order`; each bond is stored at (larger, smaller)."""
    N = len(order)
    l = np.zeros((N, N), dtype=np.int64)
    for a, b in zip(order[:-1], order[1:]):
        l[max(a, b), min(a, b)] = label
    return l


def path(N):
    return chain(list(range(N)))


def far_end_path(N):
    """1 - 2 - ... - (N-1) - 0: the smallest label enters at the far end and has to cross the whole chain, while label 1
    floods it from the other side first."""
    return chain(list(range(1, N)) + [0])


def zigzag_path(N):
    """0 - (N-1) - 1 - (N-2) - ...: neighbours along the chain are far apart in index."""
    lo, hi, order = 0, N - 1, []
    while lo <= hi:
        order.append(lo)
        if lo != hi:
            order.append(hi)
        lo, hi = lo + 1, hi - 1
    return chain(order)


def star(N, centre):
    l = np.zeros((N, N), dtype=np.int64)
    for k in range(N):
        if k != centre:
            l[max(k, centre), min(k, centre)] = 1 + (k % 3)
    return l


def complete(N, E):
    l = np.zeros((N, N), dtype=np.int64)
    for i in range(N):
        for j in range(i):
            l[i, j] = 1 + (i + j) % (E - 1)
    return l


def two_equal_components(N):
    """Even atoms chained together, odd atoms chained together: two components of N / 2 atoms (N even), roots 0 and 1."""
    l = np.zeros((N, N), dtype=np.int64)
    for i in range(2, N):
        l[i, i - 2] = 1
    return l


def upper_only(N):
    """Entries in the upper triangle (and on the diagonal) only: the decoder reads none of them."""
    l = np.zeros((N, N), dtype=np.int64)
    for i in range(N):
        l[i, i:] = 1
    return l


def one_hot_logits(atoms, labels, M, E):
    """Label arrays [..] -> float32 one-hot 'logits' [.., M] / [.., E]."""
    return np.eye(M, dtype=np.float32)[np.asarray(atoms)], np.eye(E, dtype=np.float32)[np.asarray(labels)]
