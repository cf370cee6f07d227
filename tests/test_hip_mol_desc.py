"""GPU tests of the descriptors (`dg_mol_descriptors` through `druggen_amd.descriptors`) against the plain-Python restatement of
tests/mol_desc_ref.py, whose validity input is the restatement of tests/mol_valid_ref.py -- never the GPU's own verdicts.
Batches are built from label tensors as in tests/test_hip_mol_valid.py (logits = 4 x one-hot, the reference molecules from
tests/decode_graph_ref.py, not from the GPU decode).  Every output is an integer and a pinned value: every `desc` field, every
key and every written bond class is compared with `==`.  There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_desc_ref as ref
import mol_fp_ref as fref
import mol_valid_ref as vref
from test_hip_mol_canon import _finish, _mols, _stack, _store_graphs
from test_hip_mol_smiles import _decode
from test_mol_desc_host import fixture_tables, golden_rows

pytestmark = pytest.mark.gpu

E = 5      # bond labels of the test tables: none, single, double, triple, aromatic
FILL = 0xA5
C, N_, O = 1, 2, 3      # atom labels of mol_fp_ref.ATOM_DECODER


def _tables(atom_decoder=fref.ATOM_DECODER, bond_decoder=fref.BOND_DECODER, tpsa=None):
    from druggen_amd import descriptors, validity
    return (validity.ValenceTables.from_decoders(atom_decoder, bond_decoder, "cuda"),
            descriptors.DescriptorTables.from_decoders(atom_decoder, bond_decoder, "cuda", tpsa=tpsa))


def _env(tables):
    return {int(k): int(v) for k, v in tables.env_rows}


def _check(atoms, labels, tables, cap=None, scopes=("largest",), batch=None, known=None, vtab=None, dtab=None):
    """Kernel outputs of the batch against the restatement under every scope.  `known`: per molecule the deficiency of the
    aromatic graph where the validity restatement's matching refuses the size.  Returns the last scope's (host record, host
    validity record, wanted descriptors, wanted validity)."""
    from druggen_amd import canon, descriptors, validity
    vtables, dtables = tables
    batch = batch if batch is not None else _decode(atoms, labels, E, cap)
    mols = _mols(atoms, labels)
    vtab = vtab or {}
    dtab = dtab if dtab is not None else {}      # the restatement's own tables over mol_fp_ref's decoders
    out = None
    for scope in scopes:
        checked = validity.check_molecules(batch, vtables, scope)
        host, hval = _finish(descriptors.describe_molecules(batch, checked, dtables, scope), checked)
        code = canon.SCOPES[scope]
        if known is None:
            valids = vref.validity_batch(mols, cap, code, **vtab)
        else:
            valids = [vref.validity(m["atoms"], m["bonds"], n_bonds=m["n_bonds"], cap=cap, scope=code, component=m["component"],
                                    largest=m["largest"], deficiency=d, **vtab) for m, d in zip(mols, known)]
        want = ref.describe_batch(mols, valids, cap, code, **dtab)
        assert hval.status.tolist() == [v["mol"][0] for v in valids]
        ref.assert_batch_equals(host, want)
        out = host, hval, want, valids
    return out


def _graph(N, atoms, bonds):
    """(atom labels [N], labels [N,N]) of `atoms` (a list, padded with 0) and bonds (i, j, label)."""
    a = np.zeros(N, dtype=np.int64)
    a[:len(atoms)] = atoms
    labels = np.zeros((N, N), dtype=np.int64)
    for i, j, l in bonds:
        labels[max(i, j), min(i, j)] = l
    return a, labels


def _chain(n, N=None, label=C, bonds=()):
    """n atoms in a row with single bonds, except the bonds {first atom: label} named."""
    bonds = dict(bonds)
    return _graph(N or n, [label] * n, [(i, i + 1, bonds.get(i, 1)) for i in range(n - 1)])


# ---- 1. the fixture molecules ---------------------------------------------------------------------------------------------------
def test_fixture_molecules_equal_the_restatement_and_their_hand_worked_rows():
    from druggen_amd import decode
    strings, atoms, labels, atom_dec, bond_dec, vtab, dtab = fixture_tables()
    tables = _tables(atom_dec, bond_dec)
    node, edge = dref.one_hot_logits(atoms, labels, len(atom_dec), len(bond_dec))
    batch = decode.decode_molecule_graphs(torch.from_numpy(4.0 * node).cuda(), torch.from_numpy(4.0 * edge).cuda())
    host, hval, want, valids = _check(atoms, labels, tables, scopes=("largest", "whole"), batch=batch, vtab=vtab, dtab=dtab)
    golden = golden_rows()
    for name in ref.DESC_FIELDS[:10]:
        assert getattr(host, name).tolist() == [g[name] for g in golden], name
    assert host.veber_rules.tolist() == [g["veber"] for g in golden]
    assert host.lipinski_rules(hval).tolist() == [g["lipinski"] for g in golden]
    assert host.tpsa_A2.tolist() == [g["tpsa"] / 100 for g in golden]


# ---- 2. seeded molecule-like graphs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 9, 33, 64, 65, 96, 97, 255, 256])
def test_molecule_like_graphs_equal_the_restatement(N):
    """Rings and chains with aromatic labels (mol_valid_ref.aromatic_like, most of them clean so that most are valid) at a single
    atom, a single bond, the smallest triangle, every size at which a bit row gains a word (32 k, 32 k + 1), the wave boundaries
    and the maximum; both scopes; and a bond list one row short of the largest molecule (no graph)."""
    rng = np.random.default_rng([N, 330])
    tables = _tables()
    B = 8 if N <= 97 else 6
    graphs = [vref.aromatic_like(rng, N, b % 4 != 3) for b in range(B)]
    if N == 3:
        graphs[0] = _graph(3, [C, N_, O], [(0, 1, 1), (1, 2, 1), (0, 2, 1)])      # the smallest triangle
        graphs[1] = _graph(3, [C, C, O], [(0, 1, 2), (1, 2, 1)])
    atoms, labels = _stack(graphs)
    host, _, want, _ = _check(atoms, labels, tables, scopes=("largest", "whole"))
    assert 0 in host.status
    if N >= 33:
        assert (host.status != 0).any() and host.n_rot.max() > 0 and host.n_rings.max() > 0 and host.tpsa.max() > 0
    if N == 3:
        assert host.atom_key[0].view(np.uint32).tolist() == [C | 2 << 8 | 2 << 12 | 1 << 24, N_ | 1 << 8 | 2 << 12 | 1 << 24,
                                                             O | 2 << 12 | 1 << 24]
        assert host.desc[0].tolist() == [0, 3, 0, 2194 + 1253, 0, 1, 3, 0, 1, 1, 0, 0] and host.bond_class[0].tolist() == [3, 3, 3]
    most = max(int(np.count_nonzero(l)) for l in labels)
    host, _, _, _ = _check(atoms, labels, tables, cap=max(most - 1, 0))
    if most > 0:
        cut = host.status == vref.NO_GRAPH
        assert cut.any() and not host.bond_class[cut].any() and (host.atom_key[cut] == -1).all() and not host.desc[cut][:, 1:].any()


# ---- 3. triangles ---------------------------------------------------------------------------------------------------------------------
def _fused_triangles(n, N):
    """A strip of n atoms: i - i + 1 and i - i + 2, single bonds, atoms 0 and n - 1 carbon (valence 2 + 2 hydrogens), 1 and n - 2
    carbon (3 bonds), the inner ones carbon with 4 bonds: n - 2 fused triangles, every atom in one."""
    return _graph(N, [C] * n, [(i, i + 1, 1) for i in range(n - 1)] + [(i, i + 2, 1) for i in range(n - 2)])


def test_triangles():
    tables = _tables()
    N = 9
    k3 = _graph(N, [C, N_, O], [(0, 1, 1), (1, 2, 1), (0, 2, 1)])
    k4 = _graph(N, [C] * 4, [(i, j, 1) for i in range(4) for j in range(i)])                      # tetrahedrane: six bonds, three rings
    edge = _graph(N, [C] * 4, [(0, 1, 1), (1, 2, 1), (0, 2, 1), (1, 3, 1), (2, 3, 1)])            # two triangles sharing an edge
    vertex = _graph(N, [C] * 5, [(0, 1, 1), (1, 2, 1), (0, 2, 1), (2, 3, 1), (3, 4, 1), (2, 4, 1)])      # ... sharing a vertex
    square = _graph(N, [C, N_, C, O], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 3, 1)])               # a four-ring: no triangle
    tail = _graph(N, [N_, C, C, C, O], [(0, 1, 1), (1, 2, 1), (0, 2, 1), (2, 3, 1), (3, 4, 1)])   # a triangle with a chain: the chain is outside
    # two components, the triangle in the smaller one: under `largest` it is outside the scope (a triangle that the scope cuts
    # through needs a component array the decode never writes: the next test)
    apart = _graph(N, [C] * 7, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (4, 5, 1), (5, 6, 1), (4, 6, 1)])
    atoms, labels = _stack([k3, k4, edge, vertex, square, tail, apart])
    host, _, _, _ = _check(atoms, labels, tables, scopes=("whole", "largest"))      # (the last scope: largest)
    r3 = (host.atom_key.view(np.uint32) >> 24) & (host.atom_key != -1)
    assert r3.tolist() == [[1, 1, 1] + [0] * 6, [1] * 4 + [0] * 5, [1] * 4 + [0] * 5, [1] * 5 + [0] * 4, [0] * 9,
                           [1, 1, 1] + [0] * 6, [0] * 9]
    assert host.n_rings.tolist() == [1, 3, 2, 2, 1, 1, 0] and host.n_heavy.tolist() == [3, 4, 4, 5, 4, 5, 4]
    assert host.tpsa.tolist() == [2194 + 1253, 0, 0, 0, 1203 + 923, 2194 + 2023, 0]


def test_a_triangle_whose_third_atom_is_outside_the_scope_sets_no_r3():
    """The entry itself, with a component array that puts atom 2 of the triangle 0 - 1 - 2 into another component than 0 and 1
    (the decode never writes such an array; the scope rule is defined on what the arrays hold): the rows 0 - 2 and 1 - 2 are no
    BONDS, 0 - 1 is a bridge between two atoms of degree 1, and nobody is in a triangle."""
    from druggen_amd import _lib, descriptors, validity
    vtables, dtables = _tables()
    N = 9
    atoms, labels = _stack([_graph(N, [N_, C, C, O], [(0, 1, 1), (1, 2, 1), (0, 2, 1), (2, 3, 1)])] * 2)
    batch = _decode(atoms, labels, E)
    # molecule 0: the four atoms are component 0; molecule 1: atoms 0 and 1 | atoms 2 and 3; every pad is a component of its own
    component = torch.tensor([[0, 0, 0, 0, 1, 2, 3, 4, 5], [0, 0, 1, 1, 2, 3, 4, 5, 6]], dtype=torch.uint8, device="cuda")
    largest = torch.zeros(2, dtype=torch.int32, device="cuda")
    checked = validity.MoleculeValidity.empty(2, N, batch.cap, "cuda")
    out = descriptors.MoleculeDescriptors.empty(2, N, batch.cap, "cuda")
    out.buffer.fill_(FILL)
    _lib.launch("dg_mol_validity", batch.buffer, batch.atoms.data_ptr(), batch.bonds.data_ptr(), batch.n_bonds.data_ptr(),
                component.data_ptr(), largest.data_ptr(), None, vtables.atoms.data_ptr(), vtables.n_atom_labels,
                vtables.bonds.data_ptr(), vtables.n_bond_labels, 2, N, batch.cap, 1, vref.H_MASS, checked.mol.data_ptr(),
                checked.hcount.data_ptr(), checked.kekule.data_ptr())
    _lib.launch("dg_mol_descriptors", batch.buffer, batch.atoms.data_ptr(), batch.bonds.data_ptr(), batch.n_bonds.data_ptr(),
                component.data_ptr(), largest.data_ptr(), None, checked.mol.data_ptr(), checked.hcount.data_ptr(),
                dtables.bonds.data_ptr(), dtables.n_bond_labels, dtables.atom_flags.data_ptr(), dtables.atom_class.data_ptr(),
                dtables.n_atom_labels, dtables.env.data_ptr(), dtables.n_env, 2, N, batch.cap, 1, out.desc.data_ptr(),
                out.atom_key.data_ptr(), out.bond_class.data_ptr())
    host, = _finish(out)
    mols = _mols(atoms, labels)
    want = []
    for m, comp in zip(mols, component.cpu().numpy()):
        kw = dict(scope=ref.LARGEST, component=comp, largest=0)
        valid = vref.validity(m["atoms"], m["bonds"], **kw)
        want.append(ref.describe(m["atoms"], m["bonds"], valid, **kw))
    ref.assert_batch_equals(host, want)
    # molecule 0: the whole graph, [NH] in the three-ring 2194 + OH 2023; molecule 1: N-C alone -- NH2 2602, no r3, one bridge
    assert host.desc[0].tolist() == [0, 4, 0, 2194 + 2023, 0, 1, 3, 0, 2, 2, 0, 0]
    assert host.desc[1].tolist() == [0, 2, 0, 2602, 0, 0, 0, 0, 1, 1, 0, 0]
    assert host.atom_key[1].view(np.uint32).tolist() == [N_ | 2 << 8 | 1 << 12, C | 3 << 8 | 1 << 12] + [ref.NO_KEY] * 7
    assert sorted(host.bond_class[1, :4].tolist()) == [0, 0, 0, 1] and sorted(host.bond_class[0, :4].tolist()) == [1, 3, 3, 3]


def test_fused_three_rings_of_253_atoms():
    """A strip of 251 fused triangles over 253 atoms at N = 256 (three pads), at two atom orders: every atom is in a triangle,
    every bond is a ring bond, n_rings = 503 - 253 + 1."""
    tables = _tables()
    strip = _fused_triangles(253, 256)
    graphs = [strip, vref.rotated(*strip, 100), _fused_triangles(256, 256)]
    host, _, _, _ = _check(*_stack(graphs), tables, scopes=("whole",), known=[0, 0, 0])
    assert host.desc[0].tolist() == [0, 253, 0, 0, 0, 251, 253, 0, 253, 253, 0, 0] == host.desc[1].tolist()
    assert host.desc[2].tolist() == [0, 256, 0, 0, 0, 254, 256, 0, 256, 256, 0, 0]
    keys = host.atom_key.view(np.uint32)
    assert ((keys[0, :253] >> 24) == 1).all() and (keys[0, 253:] == ref.NO_KEY).all() and ((keys[2] >> 24) == 1).all()
    assert (host.bond_class[0, :503] == 3).all() and sorted(keys[0].tolist()) == sorted(keys[1].tolist())


# ---- 4. rotatable bonds -----------------------------------------------------------------------------------------------------------
def test_rotatable_bond_edge_cases():
    tables = _tables()
    N = 256
    biphenyl_like = _graph(N, [C] * 6, [(0, 1, 1), (1, 2, 1), (0, 2, 1), (2, 3, 1), (3, 4, 1), (4, 5, 1), (3, 5, 1)])      # a bridge between two rings
    graphs = [_chain(256),                                         # 255 bonds, the two at the ends touch an atom of degree 1: 253
              _chain(256, bonds={100: 3}),                         # one triple bond: it and its two neighbours drop out: 250
              _chain(256, bonds={0: 3}),                           # ... at the end: the end bond was none, its neighbour drops: 252
              _chain(256, bonds={100: 2}),                         # a double bond is not rotatable, its neighbours are: 252
              biphenyl_like,
              cref.cycle(256, label=1),                            # ring single bonds: none
              _chain(2, N), _chain(3, N), _chain(4, N),            # 0, 0, 1
              _graph(N, [C, C, C, C], [(0, 1, 4), (1, 2, 1), (2, 3, 1)])]      # an aromatic bridge: status 4, a row of zeros
    host, hval, _, _ = _check(*_stack(graphs), tables, scopes=("whole",), known=[0] * len(graphs))
    assert host.n_rot.tolist() == [253, 250, 252, 252, 1, 0, 0, 0, 1, 0]
    assert host.status.tolist() == [0] * 9 + [vref.AROMATIC_NOT_IN_RING] and not host.desc[9, 1:].any()
    assert not host.bond_class[9, :3].any() and (host.atom_key[9] == -1).all()
    assert host.n_rings.tolist() == [0, 0, 0, 0, 2, 1, 0, 0, 0, 0] and host.n_ring_atoms.tolist() == [0, 0, 0, 0, 6, 256, 0, 0, 0, 0]
    assert host.n_sp3_carbon.tolist() == [256, 254, 254, 254, 6, 256, 2, 3, 4, 0]
    assert np.count_nonzero(host.bond_class[0, :255] == 5) == 253 and np.count_nonzero(host.bond_class[0, :255] == 1) == 2
    assert sorted(host.bond_class[4, :7].tolist()) == [3] * 6 + [5] and (host.bond_class[5, :256] == 3).all()


# ---- 5. cap = 0, truncated lists, flags, every status --------------------------------------------------------------------------------
def test_truncated_lists_flags_and_an_empty_bond_list():
    from druggen_amd import _lib, descriptors, validity
    rng = np.random.default_rng(5)
    tables = vtables, dtables = _tables()
    B, N = 6, 17
    atoms, labels = _stack([vref.aromatic_like(rng, N, True) for _ in range(B)])
    labels[2] = 0                                                  # a molecule without bonds: it has a graph at every cap
    counts = np.array([int(np.count_nonzero(l)) for l in labels])
    for cap in (0, 1, int(sorted(counts)[3]), int(max(counts))):
        for scope in ("largest", "whole"):
            host, _, _, _ = _check(atoms, labels, tables, cap=cap, scopes=(scope,))
            assert ((host.status == vref.NO_GRAPH) == (counts > cap)).all() and host.status[2] == 0
    # flags: a negative value means no graph, whatever the list and the validity record hold (the Python layer passes none)
    batch = _decode(atoms, labels, E)
    checked = validity.check_molecules(batch, vtables)
    flags = torch.tensor([0, -2, 5, -1, 0, -2], dtype=torch.int32, device="cuda")
    out = descriptors.MoleculeDescriptors.empty(B, N, batch.cap, "cuda")
    out.buffer.fill_(FILL)
    _lib.launch("dg_mol_descriptors", batch.buffer, batch.atoms.data_ptr(), batch.bonds.data_ptr(), batch.n_bonds.data_ptr(),
                batch.component.data_ptr(), batch.largest.data_ptr(), flags.data_ptr(), checked.mol.data_ptr(),
                checked.hcount.data_ptr(), dtables.bonds.data_ptr(), dtables.n_bond_labels, dtables.atom_flags.data_ptr(),
                dtables.atom_class.data_ptr(), dtables.n_atom_labels, dtables.env.data_ptr(), dtables.n_env, B, N, batch.cap, 1,
                out.desc.data_ptr(), out.atom_key.data_ptr(), out.bond_class.data_ptr())
    mols = _mols(atoms, labels)
    valids = vref.validity_batch(mols)
    want = [ref.describe(m["atoms"], m["bonds"], v, flag=f, scope=ref.LARGEST, component=m["component"], largest=m["largest"])
            for m, v, f in zip(mols, valids, flags.tolist())]
    host, = _finish(out)
    ref.assert_batch_equals(host, want)
    assert host.status.tolist()[1::2] == [-2, -2, -2] and (host.status[0::2] != -2).all()
    # an empty batch launches nothing
    empty = _decode(atoms[:0], labels[:0], E)
    got = descriptors.describe_molecules(empty, validity.check_molecules(empty, vtables), dtables)
    assert len(got) == 0 and got.desc.shape == (0, 12)


def test_every_status_but_valid_gives_the_zero_row():
    """One molecule per validity status 1 .. 5 and -2, and a valid one: the status is copied, everything else is zero, every key
    0xFFFFFFFF, every class 0."""
    tables = _tables()
    N = 9
    graphs = [_graph(N, [], []),                                                   # 1: no atom (scope whole)
              _graph(N, [C, 0], [(0, 1, 1)]),                                      # 2: a bonded pad has no table row
              _graph(N, [C] * 6, [(0, k, 1) for k in range(1, 6)]),                # 3: five bonds at a carbon
              _graph(N, [C, C], [(0, 1, 4)]),                                      # 4: an aromatic bridge
              cref.cycle(5, label=4), ]                                            # 5: an odd aromatic carbon ring
    graphs[4] = (np.pad(graphs[4][0], (0, N - 5)), np.pad(graphs[4][1], ((0, N - 5), (0, N - 5))))
    graphs.append(_graph(N, [C, C, O], [(0, 1, 1), (1, 2, 1)]))                     # 0: ethanol
    host, _, _, _ = _check(*_stack(graphs), tables, scopes=("whole",))
    assert host.status.tolist() == [1, 2, 3, 4, 5, 0]
    assert not host.desc[:5, 1:].any() and (host.atom_key[:5] == -1).all()
    assert not any(host.bond_class[b, :np.count_nonzero(graphs[b][1])].any() for b in range(5))
    assert host.desc[5].tolist() == [0, 3, 0, 2023, 0, 0, 0, 0, 2, 2, 0, 0]
    host, _, _, _ = _check(*_stack(graphs), tables, scopes=("whole",), cap=1)      # -2: ethanol's list is cut
    assert host.status.tolist() == [1, 2, -2, 4, -2, -2] and not host.desc[:, 1:].any()


# ---- 6. the table search ---------------------------------------------------------------------------------------------------------------
def test_environment_tables_of_no_row_one_row_and_4096_rows():
    """The same molecules under tables of 0, 1, 2, 26 + fillers up to 4095 and 4096 rows: with no row every polar atom is untyped;
    with one row -- the first, the last or a middle key of the full table -- exactly the atoms of that key are typed; filler keys
    around and between the real ones (every real key - 1 and + 1 among them) change nothing."""
    from druggen_amd import descriptors, validity
    rng = np.random.default_rng(6)
    vtables, full = _tables()
    N = 33
    named = [_graph(N, [N_, C, C, O], [(0, 1, 1), (1, 2, 1), (2, 3, 1)]),          # NH2 and OH
             _graph(N, [C, N_, O], [(0, 1, 1), (1, 2, 1), (0, 2, 1)]),              # [NH] and O in a three-ring
             _graph(N, [C, C, N_], [(0, 1, 1), (1, 2, 3)]),                         # N#
             _graph(N, [N_], [])]                                                   # ammonia: never typed by the built-in rows
    atoms, labels = _stack(named + [vref.aromatic_like(rng, N, True) for _ in range(12)])
    batch = _decode(atoms, labels, E)
    mols = _mols(atoms, labels)
    valids = vref.validity_batch(mols)
    checked = validity.check_molecules(batch, vtables)
    real = full.env_rows
    fillers = sorted((set(rng.choice(1 << 25, 5000, replace=False).tolist()) | {int(k) + d for k in real[:, 0] for d in (-1, 1)})
                     - set(real[:, 0].tolist()))
    assert len(fillers) >= 4096

    def table(rows):
        rows = np.array(sorted(rows), dtype=np.uint32).reshape(-1, 2)
        return descriptors.DescriptorTables(full.atom_class_rows, full.atom_flag_rows, full.bond_rows, rows, "cuda")
    cases = [[], [real[0].tolist()], [real[-1].tolist()], [real[12].tolist()], [real[3].tolist(), real[20].tolist()], real.tolist()]
    for n in (27, 64, 4095, 4096):
        pick = rng.choice(len(fillers), n - len(real), replace=False)
        cases.append(real.tolist() + [[fillers[k], 1 + k % 5000] for k in pick])
    polar = sum(len([a for a in v["members"] if ref.ATOM_FLAGS[m["atoms"][a]]]) for m, v in zip(mols, valids) if v["mol"][0] == 0)
    untyped = []
    for rows in cases:
        tables = table(rows)
        assert tables.n_env == len(rows)
        host, = _finish(descriptors.describe_molecules(batch, checked, tables))
        want = ref.describe_batch(mols, valids, env={int(k): int(v) for k, v in rows})
        ref.assert_batch_equals(host, want)
        untyped.append(int(host.n_untyped.sum()))
    assert untyped[0] == polar > untyped[1] and all(polar >= u >= untyped[5] for u in untyped[1:5]) and untyped[5:] == [untyped[5]] * 5
    assert untyped[5] >= 1 and host.tpsa[:4].tolist() == [2602 + 2023, 2194 + 1253, 2379, 0] and host.n_untyped[:4].tolist() == [0, 0, 0, 1]


# ---- 7. the same bytes on every run; every element is written, nothing outside ----------------------------------------------------
def test_two_runs_give_identical_bytes_between_untouched_guards():
    """The record is a view into a buffer filled with 0xA5 bytes, a guard of 256 bytes on both sides: after the call every `desc`
    and `atom_key` element equals the restatement (molecules without a graph included), the bond classes past min(n_bonds, cap),
    the padding between the fields and the guards still hold the fill, and a second run into a second buffer gives the same
    bytes everywhere."""
    from druggen_amd import descriptors, validity
    rng = np.random.default_rng(4)
    vtables, dtables = _tables()
    B, N, G = 9, 33, 256
    atoms, labels = _stack([vref.aromatic_like(rng, N, b % 3 != 2) for b in range(B)])
    counts = [int(np.count_nonzero(l)) for l in labels]
    cap = max(counts) - 1
    batch = _decode(atoms, labels, E, cap)
    checked = validity.check_molecules(batch, vtables, "whole")
    table, size = descriptors.MoleculeDescriptors.layout(B, N, cap)
    runs = []
    for _ in range(2):
        buf = torch.full((G + size + G,), FILL, dtype=torch.uint8, device="cuda")
        out = descriptors.MoleculeDescriptors(buf[G:G + size], B, N, cap)
        assert descriptors.describe_molecules(batch, checked, dtables, "whole", out=out) is out
        host, = _finish(out)
        runs.append(buf.cpu().numpy())
    mols = _mols(atoms, labels)
    valids = vref.validity_batch(mols, cap, ref.WHOLE)
    want = ref.describe_batch(mols, valids, cap, ref.WHOLE)
    ref.assert_batch_equals(host, want)
    assert any(w["desc"][0] == vref.NO_GRAPH for w in want) and sum(w["desc"][0] == 0 for w in want) >= 2
    assert np.array_equal(runs[0], runs[1])
    written = np.zeros(G + size + G, dtype=bool)
    for name in ("desc", "atom_key"):
        off, nbytes = table[name][:2]
        written[G + off:G + off + nbytes] = True
    off = G + table["bond_class"][0]
    for b, n in enumerate(counts):
        written[off + cap * b:off + cap * b + min(n, cap)] = True
    assert (runs[0][~written] == FILL).all() and (~written).sum() >= 2 * G + (cap - min(counts))
    with pytest.raises(ValueError, match="out="):
        descriptors.describe_molecules(batch, checked, dtables, out=descriptors.MoleculeDescriptors.empty(B + 1, N, cap, "cuda"))


# ---- 8. atom order ----------------------------------------------------------------------------------------------------------------
def test_a_permuted_batch_gives_identical_rows_and_permuted_keys():
    rng = np.random.default_rng(7)
    tables = _tables()
    N, copies = 33, 4
    base = [vref.aromatic_like(rng, N, k % 4 != 3) for k in range(8)]
    base[0] = _fused_triangles(20, N)
    graphs, perms = [], []
    for g in base:
        graphs.append(g)
        perms.append(np.arange(N))
        for _ in range(copies - 1):
            a, l, perm = vref.renumbered(rng, *g)
            graphs.append((a, l))
            perms.append(perm)
    host, _, _, _ = _check(*_stack(graphs), tables, scopes=("whole",))
    for k in range(len(base)):
        first = copies * k
        for c in range(copies):
            assert host.desc[first + c].tolist() == host.desc[first].tolist()
            assert host.atom_key[first + c].tolist() == host.atom_key[first][perms[first + c]].tolist()
            rows = np.count_nonzero(graphs[first][1])
            assert sorted(host.bond_class[first + c, :rows].tolist()) == sorted(host.bond_class[first, :rows].tolist())
    assert (host.status == 0).sum() >= 8 and (host.n_rot > 0).any()


# ---- 9. stores, the sampler, a captured graph -------------------------------------------------------------------------------------
def test_descriptors_of_a_resident_store_in_uneven_chunks():
    """`descriptor_store` equals `check_molecules` + `describe_molecules` on the whole set and the restatement, whatever the
    chunk (1, 7, n)."""
    from druggen_amd import descriptors, validity
    from druggen_amd.resident import ResidentMolecules
    n, N = 11, 9
    graphs, atoms, labels = _store_graphs(n, N, E, 1)
    store = ResidentMolecules.from_graphs(graphs, device="cuda", m_dim=4, b_dim=E)
    vtables, dtables = _tables()
    mols = _mols(atoms, labels)
    batch = _decode(atoms, labels, E)
    whole_valid = validity.check_molecules(batch, vtables)
    whole, = _finish(descriptors.describe_molecules(batch, whole_valid, dtables))
    for scope, code in (("largest", ref.LARGEST), ("whole", ref.WHOLE)):
        valids = vref.validity_batch(mols, scope=code)
        want = ref.describe_batch(mols, valids, scope=code)
        for chunk in (1, 7, n) if scope == "largest" else (5,):
            checked, out = descriptors.descriptor_store(store, vtables, dtables, chunk=chunk, scope=scope)
            host, hval = _finish(out, checked)
            assert len(host) == n == len(hval)
            ref.assert_batch_equals(host, want)
            vref.assert_batch_equals(hval, valids, mols)
            if scope == "largest":
                assert np.array_equal(host.desc, whole.desc) and np.array_equal(host.atom_key, whole.atom_key)


@pytest.mark.parametrize("graph", [False, True])
def test_sampler_describes_its_batch(graph):
    """`MoleculeSampler(..., validity=, descriptors=)`: the record on the returned batch equals `describe_molecules` on that batch
    field for field (graphed: a replay against the eager call) and the restatement, and a sampler without tables carries none."""
    from druggen_amd import descriptors, synth
    from druggen_amd.model import Generator
    from druggen_amd.sampling import MoleculeSampler
    N, Mn, B = 9, 13, 4
    net = Generator("relu", N, E, Mn, 0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
    params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=11)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net = net.cuda()
    decoder = {0: 0, 1: 6, 2: 7, 3: 8, 4: 9, 5: 15, 6: 16, 7: 17, 8: 35, 9: 53, 10: 34, 11: 14, 12: 5}
    vtables, dtables = _tables(decoder)
    vtab = dict(atom_rows=vtables.atom_rows.tolist(), bond_rows=vtables.bond_rows.tolist())
    dtab = dict(bond_rows=dtables.bond_rows.tolist(), atom_flags=dtables.atom_flag_rows.tolist(),
                atom_class=dtables.atom_class_rows.tolist(), env=ref.env_for(decoder))
    assert _env(dtables) == dtab["env"]
    rng = np.random.default_rng(4)
    inputs = []
    for _ in range(2):
        atoms, labels = _stack([cref.molecule_like(rng, N, b % 3) for b in range(B)])
        node, edge = dref.one_hot_logits(atoms, labels + labels.transpose(0, 2, 1), Mn, E)
        inputs.append((torch.from_numpy(edge).cuda(), torch.from_numpy(node).cuda()))
    with pytest.raises(TypeError, match="DescriptorTables"):
        MoleculeSampler(net, *inputs[0], graph=False, validity=vtables, descriptors=vtables)
    with pytest.raises(ValueError, match="needs validity="):
        MoleculeSampler(net, *inputs[0], graph=False, descriptors=dtables)
    plain = MoleculeSampler(net, *inputs[0], graph=graph, validity=vtables)
    describing = MoleculeSampler(net, *inputs[0], graph=graph, validity=vtables, descriptors=dtables)
    assert plain.descriptors is None
    for edge, node in inputs[::-1]:
        bare = plain.sample(edge, node)
        assert bare.descriptors is None and plain.descriptors is None
        before, = _finish(bare)
        batch = describing.sample(edge, node)
        assert batch.descriptors is describing.descriptors and isinstance(batch.descriptors, descriptors.MoleculeDescriptors)
        got, gval, host = _finish(batch.descriptors, batch.validity, batch)
        for name in ("atoms", "n_bonds", "component", "n_components", "largest", "largest_size"):
            assert np.array_equal(getattr(host, name), getattr(before, name)), name
        eager, = _finish(descriptors.describe_molecules(batch, batch.validity, dtables))
        rows = [min(int(n), host.cap) for n in host.n_bonds]
        assert np.array_equal(got.desc, eager.desc) and np.array_equal(got.atom_key, eager.atom_key)
        assert all(np.array_equal(got.bond_class[b, :rows[b]], eager.bond_class[b, :rows[b]]) for b in range(B))
        mols = [dict(atoms=host.atoms[b], bonds=host.edge_list(b), n_bonds=int(host.n_bonds[b]), component=host.component[b],
                     largest=int(host.largest[b])) for b in range(B)]
        valids = vref.validity_batch(mols, **vtab)
        vref.assert_batch_equals(gval, valids, mols)
        ref.assert_batch_equals(got, ref.describe_batch(mols, valids, **dtab))


def test_a_captured_graph_follows_its_static_inputs():
    """Decode, check and describe captured into one hipGraph with `out=`: the capture allocates nothing, and replays on new
    logits give the eager results and the restatement's."""
    from druggen_amd import decode, descriptors, validity
    rng = np.random.default_rng(8)
    B, N, M = 5, 9, 7
    vtables, dtables = _tables()
    sets = [_stack([vref.aromatic_like(rng, N, b % 4 != 3) for b in range(B)]) for _ in range(3)]
    node, edge = (torch.from_numpy(4.0 * t).cuda() for t in dref.one_hot_logits(*sets[0], M, E))
    cap = N * (N - 1) // 2
    decoded = decode.MoleculeBatch.empty(B, N, cap, False, "cuda")
    checked = validity.MoleculeValidity.empty(B, N, cap, "cuda")
    out = descriptors.MoleculeDescriptors.empty(B, N, cap, "cuda")

    def chain():
        decode.decode_molecule_graphs(node, edge, out=decoded)
        validity.check_molecules(decoded, vtables, "whole", out=checked)
        descriptors.describe_molecules(decoded, checked, dtables, "whole", out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        chain()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    seen = []
    for atoms, labels in sets[1:] + sets[:1]:
        n, e = dref.one_hot_logits(atoms, labels, M, E)
        node.copy_(torch.from_numpy(4.0 * n))
        edge.copy_(torch.from_numpy(4.0 * e))
        out.buffer.fill_(FILL)
        graph.replay()
        got, = _finish(out)
        batch = _decode(atoms, labels, E)
        eager, = _finish(descriptors.describe_molecules(batch, validity.check_molecules(batch, vtables, "whole"), dtables, "whole"))
        mols = _mols(atoms, labels)
        assert np.array_equal(got.desc, eager.desc) and np.array_equal(got.atom_key, eager.atom_key)
        assert all(np.array_equal(got.bond_class[b, :m["n_bonds"]], eager.bond_class[b, :m["n_bonds"]]) for b, m in enumerate(mols))
        ref.assert_batch_equals(got, ref.describe_batch(mols, vref.validity_batch(mols, scope=ref.WHOLE), scope=ref.WHOLE))
        seen.append(got.desc.tobytes())
    assert len(set(seen)) == 3


# ---- 10. the rule counts --------------------------------------------------------------------------------------------------------------
def test_rule_counts_on_the_device_and_at_their_thresholds():
    """`veber_rules` / `lipinski_rules` on the device record against the restatement, at the thresholds: chains of 13 and 14
    carbons have 10 and 11 rotatable bonds; a chain of 35 carbons weighs 492.6 Da and the same chain with a Cl for its last C 512.5,
    with a Se for an inner C 558.5 -- under and over 500 by element choice; six OH are six donors; eleven O are eleven acceptors; and a
    chain of 15 hydroxylated carbons carries 15 x 20.23 = 303.45 A^2."""
    from druggen_amd import descriptors, validity
    N = 40
    polyol = _graph(N, [C] * 15 + [O] * 15, [(i, i + 1, 1) for i in range(14)] + [(i, 15 + i, 1) for i in range(15)])
    hexol = _graph(N, [C] * 6 + [O] * 6, [(i, i + 1, 1) for i in range(5)] + [(i, 6 + i, 1) for i in range(6)])
    pentol = _graph(N, [C] * 6 + [O] * 5, [(i, i + 1, 1) for i in range(5)] + [(i, 6 + i, 1) for i in range(5)])
    ethers = _chain(23, N)
    ethers[0][1:23:2] = O                                          # C O C O ... C: eleven O, no donor
    ethers10 = _chain(21, N)
    ethers10[0][1:21:2] = O
    heavy_cl, heavy_se = _chain(35, N), _chain(35, N)
    heavy_cl[0][34], heavy_se[0][17] = 5, 6                        # Cl at the end (valence 1), Se inside (valence 2)
    graphs = [_chain(13, N), _chain(14, N), _chain(35, N), heavy_cl, heavy_se, hexol, pentol, ethers, ethers10, polyol,
              _graph(N, [C, C], [(0, 1, 4)])]
    vtables, dtables = _tables()
    atoms, labels = _stack(graphs)
    batch = _decode(atoms, labels, E)
    checked = validity.check_molecules(batch, vtables)
    desc = descriptors.describe_molecules(batch, checked, dtables)
    veber, lipinski = desc.veber_rules, desc.lipinski_rules(checked)
    assert veber.is_cuda and lipinski.is_cuda and veber.dtype == lipinski.dtype == torch.int32 and desc.tpsa_A2.is_cuda
    host, hval = _finish(desc, checked)
    mols = _mols(atoms, labels)
    valids = vref.validity_batch(mols)
    want = ref.describe_batch(mols, valids)
    ref.assert_batch_equals(host, want)
    assert veber.tolist() == [ref.veber_rules(w["desc"]) for w in want] == host.veber_rules.tolist()
    assert lipinski.tolist() == [ref.lipinski_rules(v["mol"], w["desc"]) for v, w in zip(valids, want)] == host.lipinski_rules(hval).tolist()
    assert host.n_rot.tolist()[:2] == [10, 11] and hval.mass.tolist()[2:5] == [35 * 120000 + 72 * 10078, 34 * 120000 + 349689 + 69 * 10078,
                                                                              34 * 120000 + 799165 + 70 * 10078]
    assert hval.mass[2] < 5000000 < hval.mass[3] < hval.mass[4]
    assert hval.n_donors.tolist()[5:7] == [6, 5] and hval.n_acceptors.tolist()[7:9] == [11, 10] and host.tpsa[9] == 15 * 2023
    #                 rot 10   rot 11   492 Da, rot 32   over 500   over 500   6 donors   5 donors   11 acc.  10 acc.  303 A^2  invalid
    assert veber.tolist() == [2, 1, 1, 1, 1, 2, 2, 1, 1, 0, 0]
    assert lipinski.tolist() == [4, 3, 3, 2, 2, 3, 4, 2, 3, 1, 0]
