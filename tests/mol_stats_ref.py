"""numpy restatement of `dg_mol_stats` (include/druggen_hip.h), written from its specification: every column of
`mol` and every entry of `tot`, in plain loops over dense label matrices.  No keys: duplicates are a double loop that compares
the label matrices.  The molecules are the per-molecule dicts of tests/decode_graph_ref.py (`decode_labels`)."""
import numpy as np

COLUMNS = ("atom_types", "largest_size", "n_components", "n_bonds", "over_valent", "changed_atoms", "changed_bonds",
           "duplicate_of")


def dense_labels(bonds, N):
    """[N,N] label matrix (lower triangle) of a bond list [(i, j, label)]."""
    dense = np.zeros((N, N), dtype=np.int64)
    for i, j, l in np.asarray(bonds).reshape(-1, 3).tolist():
        dense[i, j] = l
    return dense


def molecules_of(host):
    """The restatement's molecule dicts from a host `MoleculeBatch`."""
    out = []
    for b in range(host.B):
        out.append(dict(atoms=host.atoms[b].copy(), bonds=host.edge_list(b).copy(), n_bonds=int(host.n_bonds[b]),
                        n_components=int(host.n_components[b]), largest_size=int(host.largest_size[b]),
                        valence2=None if host.valence2 is None else host.valence2[b].copy()))
    return out


def atom_types(row):
    """The reference's count (src/util/utils.py:122-127, `Metrics.mean_atom_type`: `len(i.unique().tolist())` per molecule of
    the argmax'd node tensor): the pad label counts as a type."""
    return len(np.unique(np.asarray(row)))


def mol_stats(mols, cap=None, in_atoms=None, in_labels=None, max_valence2=None):
    """(mol [B,8] int32, tot [16] int64) of the molecule dicts `mols`; `cap`: rows of the bond list (None: nothing truncated;
    a truncated molecule's dict may hold the full list or its prefix, it is not looked at)."""
    B = len(mols)
    mol = np.full((B, 8), -1, dtype=np.int32)
    dense = []
    for b, m in enumerate(mols):
        N = len(m["atoms"])
        truncated = cap is not None and m["n_bonds"] > cap
        dense.append(None if truncated else dense_labels(m["bonds"], N))
        mol[b, 0] = atom_types(m["atoms"])
        mol[b, 1], mol[b, 2], mol[b, 3] = m["largest_size"], m["n_components"], m["n_bonds"]
        if m["valence2"] is not None and max_valence2 is not None:
            over = 0
            for i in range(N):
                a = int(m["atoms"][i])
                if a < len(max_valence2) and int(m["valence2"][i]) > int(max_valence2[a]):
                    over += 1
            mol[b, 4] = over
        if in_atoms is not None:
            mol[b, 5] = sum(int(m["atoms"][i]) != int(in_atoms[b][i]) for i in range(N))
        if in_labels is not None and not truncated:
            mol[b, 6] = sum(int(dense[b][i, j]) != int(in_labels[b][i][j]) for i in range(N) for j in range(i))
        if truncated:
            mol[b, 7] = -2
            continue
        for j in range(b):
            if dense[j] is not None and mols[j]["n_bonds"] == m["n_bonds"] and \
                    np.array_equal(mols[j]["atoms"], m["atoms"]) and np.array_equal(dense[j], dense[b]):
                mol[b, 7] = j
                break
    tot = np.zeros(16, dtype=np.int64)
    tot[0] = B
    for c in range(7):
        tot[1 + c] = sum(int(v) for v in mol[:, c] if v >= 0)
    tot[8] = int((mol[:, 4] > 0).sum())
    tot[9] = int(((mol[:, 5] == 0) & (mol[:, 6] == 0)).sum())
    tot[10] = int((mol[:, 7] == -1).sum())
    tot[11] = sum(1 for m in mols if cap is not None and m["n_bonds"] > cap)
    tot[12] = int((mol[:, 2] == 1).sum())
    return mol, tot
