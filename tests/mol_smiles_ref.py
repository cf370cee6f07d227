"""Plain-Python restatement of `dg_mol_smiles` (include/druggen_hip_text.h), written from its specification:
recursion, lists, sets and `sorted()`.  It takes what the kernel takes -- atom labels, bond rows, the decode's components, the
two symbol tables as arrays -- and returns what it stores.  Also the tables, graph helpers and the parse-back check the host and
GPU tests share."""
import numpy as np

WHOLE, LARGEST, FORMS = 0, 1, 2
NO_GRAPH, RINGS, LONG = -2, -3, -4


class _RingsOut(Exception):
    pass


def write(atoms, bonds, atom_table, bond_table, *, n_bonds=None, cap=None, component=None, largest=None, flag=0, scope=WHOLE,
          str_cap=None):
    """One molecule: atoms [N] labels, bonds rows (hi, lo, label) -- the first min(n_bonds, cap) count -- tables [n,4] / [n,2]
    uint8.  Returns dict(length, n_written, order [n_written], text bytes of str_cap (None: 8 N) bytes)."""
    atoms = [int(a) for a in atoms]
    rows = [(int(r[0]), int(r[1]), int(r[2])) for r in np.asarray(bonds).tolist()]
    N = len(atoms)
    n_bonds = len(rows) if n_bonds is None else int(n_bonds)
    cap = max(n_bonds, len(rows)) if cap is None else int(cap)
    str_cap = 8 * N if str_cap is None else int(str_cap)
    blank = bytes(str_cap)
    if n_bonds > cap or flag < 0:
        return dict(length=NO_GRAPH, n_written=0, order=[], text=blank)
    rows = [r for r in rows[:n_bonds] if r[0] < N and r[1] < N and r[0] != r[1]]

    if scope == LARGEST:
        S = {i for i in range(N) if int(component[i]) == int(largest)}
    elif scope == WHOLE:
        S = {i for i in range(N) if atoms[i] != 0} | {i for i, _, _ in rows} | {j for _, j, _ in rows}
    else:
        S = {i for i in range(N) if atoms[i] != 0xFF}

    def atom_row(l):
        known = l < len(atom_table) and atom_table[l][0] != 0
        return (chr(atom_table[l][0]), chr(atom_table[l][1]) if atom_table[l][1] else "", int(atom_table[l][2])) if known else ("?", "", 0)

    def bond_row(l):
        known = l < len(bond_table) and bond_table[l][0] != 0
        return (chr(bond_table[l][0]), bool(bond_table[l][1])) if known else ("?", False)

    label, nbrs = {}, {i: set() for i in S}
    for i, j, l in rows:
        if i in S and j in S:
            label[frozenset((i, j))] = l
            nbrs[i].add(j)
            nbrs[j].add(i)
    lower = {i: bool(atom_row(atoms[i])[2] & 2) and any(bond_row(label[frozenset((i, j))])[1] for j in nbrs[i]) for i in S}

    # ---- the traversal ----
    order, pre, parent, children = [], {}, {}, {}

    def visit(v, p):
        pre[v], parent[v], children[v] = len(order), p, []
        order.append(v)
        for u in sorted(nbrs[v]):
            if u not in pre:
                children[v].append(u)
                visit(u, v)
    for root in sorted(S):
        if root not in pre:
            visit(root, None)

    # ---- the string ----
    def bond_symbol(a, b):
        sym, aromatic = bond_row(label[frozenset((a, b))])
        if lower[a] and lower[b]:
            return "" if aromatic else sym
        return "" if sym == "-" else sym

    def number(n):
        return str(n) if n < 10 else "%%%02d" % n

    out, in_use, closed_here, number_of = [], set(), set(), {}

    def emit(v):
        p = parent[v]
        if p is not None:
            out.append(bond_symbol(p, v))
        first, second, fl = atom_row(atoms[v])
        if lower[v]:
            first = first.lower()
        out.append(("[%s%s]" if fl & 1 else "%s%s") % (first, second))
        in_use.difference_update(closed_here)
        closed_here.clear()
        for u in sorted((u for u in nbrs[v] if u != p and u not in children[v]), key=pre.get):
            if pre[u] < pre[v]:
                n = number_of.pop((u, v))
                out.append(bond_symbol(u, v) + number(n))
                closed_here.add(n)
            else:
                free = [n for n in range(1, 100) if n not in in_use]
                if not free:
                    raise _RingsOut
                in_use.add(free[0])
                number_of[(v, u)] = free[0]
                out.append(number(free[0]))
        for c in children[v][:-1]:
            out.append("(")
            emit(c)
            out.append(")")
        if children[v]:
            emit(children[v][-1])

    result = dict(n_written=len(order), order=order)
    try:
        for root in (v for v in order if parent[v] is None):
            if out:
                out.append(".")
            emit(root)
    except _RingsOut:
        return dict(result, length=RINGS, text=blank)
    text = "".join(out).encode("ascii")
    if len(text) > str_cap:
        return dict(result, length=LONG, text=blank)
    return dict(result, length=len(text), text=text + bytes(str_cap - len(text)))


def write_batch(mols, atom_table, bond_table, cap=None, scope=LARGEST, str_cap=None):
    """The molecule dicts of tests/decode_graph_ref.py (`decode_labels`) -> list of `write` results; `cap`: rows of the bond list."""
    return [write(m["atoms"], m["bonds"][:cap], atom_table, bond_table, n_bonds=m["n_bonds"], cap=cap,
                  component=m["component"], largest=m["largest"], scope=scope, str_cap=str_cap) for m in mols]


def assert_batch_equals(host, want):
    """Every field of a host `SmilesBatch` against the restatement's list, with `==`, fillers included."""
    assert host.B == len(want)
    for b, w in enumerate(want):
        where = f"molecule {b}"
        assert (int(host.length[b]), int(host.n_written[b])) == (w["length"], w["n_written"]), (where, host.length[b], w["length"])
        n = w["n_written"]
        assert host.order[b, :n].tolist() == w["order"] and (host.order[b, n:] == 0xFF).all(), where
        assert host.text[b].tobytes() == w["text"], (where, host.text[b].tobytes(), w["text"])


# ---- tables --------------------------------------------------------------------------------------------------------------
# atom labels 0..6: pad, C, N, O, S, Cl, Se; bond labels 0..4: none, single, double, triple, aromatic (RDKit's values)
ATOM_DECODER = {0: 0, 1: 6, 2: 7, 3: 8, 4: 16, 5: 17, 6: 34}
BOND_DECODER = {0: 0, 1: 1, 2: 2, 3: 3, 4: 12}


def tables(atom_decoder=ATOM_DECODER, bond_decoder=BOND_DECODER):
    """Host arrays ([n,4], [n,2] uint8) of `SmilesTables.from_decoders`'s rows."""
    from druggen_amd import smiles_out
    return smiles_out.table_rows(atom_decoder, bond_decoder)


def relabelled(rng, atoms, labels):
    """The same bonds with every atom one of C N O S Cl Se (labels 1..6, no pad) and every bond one of the four types."""
    labels = np.array(labels)
    labels[labels != 0] = rng.choice([1, 1, 1, 2, 3, 4, 4], int(np.count_nonzero(labels)))
    return rng.integers(1, 7, len(atoms)), labels


# ---- reading a string back --------------------------------------------------------------------------------------------------
def parse_back(text, atoms, labels, order, atom_decoder=ATOM_DECODER, bond_decoder=BOND_DECODER):
    """`smiles.parse_smiles(text)` is the input graph (atoms [N] labels, labels [N,N] lower triangle) read through `order`:
    atomic numbers of atoms[order[k]], and exactly the bonds among the atoms of `order`, with their types.  The parser takes
    one fragment at a time: the parts between `.` are parsed one by one and numbered on."""
    from druggen_amd.smiles import parse_smiles
    z, bonds = [], []
    for part in text.split("."):
        part_z, _, part_bonds = parse_smiles(part)
        bonds += [(i + len(z), j + len(z), t) for i, j, t in part_bonds]
        z += part_z
    assert z == [atom_decoder[int(atoms[p])] for p in order], text
    got = sorted((max(order[i], order[j]), min(order[i], order[j]), t) for i, j, t in bonds)
    assert len(set(g[:2] for g in got)) == len(got), text
    inside = set(order)
    want = sorted((i, j, bond_decoder[int(labels[i][j])]) for i in inside for j in inside if j < i and labels[i][j])
    assert got == want, (text, got, want)
