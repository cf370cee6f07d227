"""GPU tests of the validity check (`dg_mol_validity` through `druggen_amd.validity`) against the plain-Python restatement of
tests/mol_valid_ref.py.  Batches are built from label tensors as in tests/test_hip_mol_fp.py (logits = 4 x one-hot, the
reference molecules from tests/decode_graph_ref.py, not from the GPU decode).  Every output is an integer: every `mol` field
and `hcount` are compared with `==`; the Kekule rows are a certificate and are checked as one (mol_valid_ref.check_certificate).
There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_fp_ref as fref
import mol_valid_ref as ref
from test_hip_mol_canon import _finish, _mols, _stack, _store_graphs
from test_hip_mol_smiles import _decode
from test_mol_valid_host import fixture_molecules

pytestmark = pytest.mark.gpu

E = 5      # bond labels of the test tables: none, single, double, triple, aromatic
FILL = 0xA5


def _tables(atom_decoder=fref.ATOM_DECODER, bond_decoder=fref.BOND_DECODER):
    from druggen_amd import validity
    return validity.ValenceTables.from_decoders(atom_decoder, bond_decoder, "cuda")


def _check(atoms, labels, tables, cap=None, scopes=("largest",), batch=None, known=None, **tab):
    """Kernel outputs of the batch against the restatement under every scope, certificate included.  `known`: per molecule the
    deficiency derived by construction (scope `whole` only), where the restatement's matching refuses the size."""
    from druggen_amd import canon, validity
    batch = batch if batch is not None else _decode(atoms, labels, E, cap)
    mols = _mols(atoms, labels)
    out = None
    for scope in scopes:
        host, = _finish(validity.check_molecules(batch, tables, scope))
        if known is None:
            want = ref.validity_batch(mols, cap, canon.SCOPES[scope], **tab)
        else:
            assert scope == "whole"
            want = [ref.validity(m["atoms"], m["bonds"], deficiency=d, **tab) for m, d in zip(mols, known)]
        ref.assert_batch_equals(host, want, mols)
        out = host, want
    return out


# ---- 1. the fixture molecules ---------------------------------------------------------------------------------------------------
def test_fixture_molecules_equal_the_restatement():
    """The eight molecules of tests/golden/chembl_like_smiles.csv under the decoders `smiles.build_encoders` gives them, both
    scopes (the molecules are connected: the scopes agree): seven valid, one not kekulisable (its [nH] has lost its H)."""
    from druggen_amd import decode, validity
    strings, atoms, labels, atom_dec, bond_dec = fixture_molecules()
    tables = _tables(atom_dec, bond_dec)
    tab = dict(atom_rows=tables.atom_rows.tolist(), bond_rows=tables.bond_rows.tolist())
    node, edge = dref.one_hot_logits(atoms, labels, len(atom_dec), len(bond_dec))
    batch = decode.decode_molecule_graphs(torch.from_numpy(4.0 * node).cuda(), torch.from_numpy(4.0 * edge).cuda())
    host, _ = _check(atoms, labels, tables, scopes=("largest", "whole"), batch=batch, **tab)
    assert host.status.tolist() == [0] * 7 + [5] and host.valid.tolist() == [True] * 7 + [False]
    assert host.n_h.tolist() == [35, 27, 24, 32, 18, 45, 26, 0] and host.valid_fraction() == 7 / 8
    got = validity.check_molecules(batch, tables)
    assert float(got.valid_fraction()) == 7 / 8 and got.valid_fraction().is_cuda


# ---- 2. seeded molecule-like graphs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 9, 33, 64, 65, 96, 97, 255, 256])
def test_molecule_like_graphs_equal_the_restatement(N):
    """Rings and chains with aromatic labels (mol_valid_ref.aromatic_like: every second molecule clean, the others with odd
    carbon rings and defects) at every size at which a bit row gains a word (32 k, 32 k + 1), the wave boundaries and the
    maximum; both scopes; and a bond list one row short of the largest molecule (no graph)."""
    rng = np.random.default_rng([N, 328])
    tables = _tables()
    B = 8 if N <= 97 else 6
    atoms, labels = _stack([ref.aromatic_like(rng, N, b % 2 == 0) for b in range(B)])
    host, want = _check(atoms, labels, tables, scopes=("largest", "whole"))
    if N >= 9:
        assert 0 in host.status and (host.status != 0).any()
    most = max(int(np.count_nonzero(l)) for l in labels)
    host, _ = _check(atoms, labels, tables, cap=max(most - 1, 0))
    if most > 0:
        cut = host.status == ref.NO_GRAPH
        assert cut.any() and not host.kekule[cut][..., 3].any() and (host.hcount[cut] == 0xFF).all()


def test_old_families_equal_the_restatement():
    """The molecule-like family of the canonical-form tests (random trees with ring closures labelled single or aromatic: most
    aromatic bonds are bridges or sit in rings that are not aromatic all round), dense random graphs (over-valent) and pads."""
    rng = np.random.default_rng(2)
    tables = _tables()
    for N in (9, 21):
        graphs = [cref.molecule_like(rng, N, (0, 1, 2, 4)[b % 4], b == 5) for b in range(6)]
        graphs += [(rng.integers(1, 7, N), np.tril(rng.integers(0, E, (N, N)), -1)), (np.zeros(N, dtype=np.int64), dref.empty_graph(N)),
                   cref.cycle(N, label=4), cref.cycle(N - 1 if N > 9 else N - 3, label=4)]
        graphs = [(np.pad(a, (0, N - len(a))), np.pad(l, ((0, N - len(a)), (0, N - len(a))))) for a, l in graphs]
        host, _ = _check(*_stack(graphs), tables, scopes=("largest", "whole"))
        assert host.status[6] == ref.OVER_VALENT and host.n_over[6] >= 1 and host.status[7] == ref.EMPTY      # (whole)
        assert (host.status[8], host.deficiency[8]) == (5, 1) and host.status[9] == 0      # an odd and an even carbon ring


# ---- 3. families whose deficiency is known by construction -----------------------------------------------------------------------
# mol_valid_ref.fused_chain: a chain of fused aromatic carbon rings in which no atom lies on two fusion bonds has its perimeter
# as a Hamiltonian cycle and every atom is a candidate; so its deficiency is 0 when the atom count is even (every second
# perimeter bond) and 1 when it is odd (one atom must stay free by parity, and the perimeter without it is a path with an even
# number of vertices).  Disjoint systems add up.  The restatement refuses these sizes; everything but the matching still comes
# from it, certificate included.
def _systems(N, *systems):
    atoms, labels, used = ref.disjoint(systems, N)
    return (atoms, labels), sum(ref.chain_atoms(s) % 2 for s in systems), used


def test_families_with_a_known_deficiency_at_255_and_256_atoms():
    tables = _tables()
    cases = [
        _systems(255, *[[5]] * 51),                        # 51 disjoint five-rings: deficiency 51
        _systems(256, *[[7]] * 36),                        # 36 seven-rings and four pads: 36
        _systems(255, *[[3]] * 85),                        # 85 triangles: the most free vertices 255 atoms can leave
        _systems(256, [5, 7] * 31),                        # fused five- and seven-rings, 250 atoms: nested blossoms, deficiency 0
        _systems(255, [5, 7] * 31 + [5]),                  # ... 253 atoms: 1
        _systems(256, *[[5, 5]] * 32),                     # odd rings fused in pairs, 8 atoms each: 0
        _systems(256, *[[5, 7]] * 25),                     # ... 10 atoms each
        _systems(255, [6] * 62 + [5]),                     # a flower: a ladder of 62 six-rings that ends in a five-ring, 253 atoms: 1
        _systems(256, [5] + [6] * 61 + [7]),               # ... with an odd ring at either end, 254 atoms: 0
        _systems(256, [6] * 63),                           # the ladder alone, 254 atoms: 0
    ]
    assert [c[1] for c in cases] == [51, 36, 85, 0, 1, 0, 0, 1, 0, 0] and [c[2] for c in cases] == [255, 252, 255, 250, 253, 256, 250, 253, 254, 254]
    ring = cref.cycle(256, label=4)                        # one even ring of 256: every second bond
    for N in (255, 256):
        graphs = [c[0] for c in cases if len(c[0][0]) == N] + ([ring] if N == 256 else [])
        known = [c[1] for c in cases if len(c[0][0]) == N] + ([0] if N == 256 else [])
        host, want = _check(*_stack(graphs), tables, scopes=("whole",), known=known)
        assert host.deficiency.tolist() == known and host.status.tolist() == [5 if d else 0 for d in known]
        if N == 256:
            assert host.mol[-1].tolist() == [0, 256, 0, 0, 256, 256 * (120000 + 10078), 0, 0] and (host.hcount[-1] == 1).all()
    # under `largest` one system is left
    (atoms, labels), _, _ = cases[0]
    host, _ = _check(atoms[None], labels[None], tables)
    assert host.mol[0].tolist() == [5, 5, 0, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("sizes,N", [([6] * 14 + [5], 63), ([5] + [6] * 13 + [7], 64), ([5, 7, 5, 7, 5, 7, 5, 7, 5, 7, 5, 7, 5], 64)])
def test_a_flower_at_every_rotation_of_the_atom_order(sizes, N):
    """A ladder of six-rings (the stem: even rings) that ends in odd rings, and a chain of odd rings, with atom 0 at every
    position in turn: the greedy start and every search begin somewhere else, the deficiency stays what the parity says."""
    tables = _tables()
    atoms, labels, used = ref.fused_chain(sizes, N)
    graphs = [ref.rotated(atoms, labels, shift) for shift in range(N)]
    host, _ = _check(*_stack(graphs), tables, scopes=("whole",), known=[used % 2] * N)
    assert (host.deficiency == used % 2).all() and (host.n_atoms == used).all()
    assert len({tuple(sorted(h.tolist())) for h in host.hcount}) == 1


# ---- 4. the same bytes on every run; every element is written, nothing outside ----------------------------------------------------
def test_two_runs_give_identical_bytes_between_untouched_guards():
    """The record is a view into a buffer filled with 0xA5 bytes, a guard of 256 bytes on both sides: after the call every `mol`
    and `hcount` element equals the restatement (molecules without a graph included), the Kekule rows past min(n_bonds, cap),
    the padding between the fields and the guards still hold the fill, and a second run into a second buffer gives the same
    bytes everywhere."""
    from druggen_amd import validity
    rng = np.random.default_rng(4)
    tables = _tables()
    B, N, G = 9, 33, 256
    atoms, labels = _stack([ref.aromatic_like(rng, N, b % 3 == 0) for b in range(B)])
    counts = [int(np.count_nonzero(l)) for l in labels]
    cap = max(counts) - 1
    batch = _decode(atoms, labels, E, cap)
    table, size = validity.MoleculeValidity.layout(B, N, cap)
    runs = []
    for _ in range(2):
        buf = torch.full((G + size + G,), FILL, dtype=torch.uint8, device="cuda")
        out = validity.MoleculeValidity(buf[G:G + size], B, N, cap)
        assert validity.check_molecules(batch, tables, "whole", out=out) is out
        host, = _finish(out)
        runs.append(buf.cpu().numpy())
    mols = _mols(atoms, labels)
    want = ref.validity_batch(mols, cap, ref.WHOLE)
    ref.assert_batch_equals(host, want, mols)
    assert any(w["mol"][0] == ref.NO_GRAPH for w in want) and any(w["mol"][0] == 0 for w in want)
    assert np.array_equal(runs[0], runs[1])
    written = np.zeros(G + size + G, dtype=bool)
    for name in ("mol", "hcount"):
        off, nbytes = table[name][:2]
        written[G + off:G + off + nbytes] = True
    off = G + table["kekule"][0]
    for b, n in enumerate(counts):
        written[off + 4 * cap * b:off + 4 * (cap * b + min(n, cap))] = True
    assert (runs[0][~written] == FILL).all() and (~written).sum() >= 2 * G + 4 * (cap - min(counts))
    with pytest.raises(ValueError, match="out="):
        validity.check_molecules(batch, tables, out=validity.MoleculeValidity.empty(B + 1, N, cap, "cuda"))


# ---- 5. truncated lists, flags, cap = 0, unknown labels ---------------------------------------------------------------------------
def test_truncated_lists_flags_and_an_empty_bond_list():
    from druggen_amd import _lib, validity
    rng = np.random.default_rng(5)
    tables = _tables()
    B, N = 6, 17
    atoms, labels = _stack([ref.aromatic_like(rng, N, True) for _ in range(B)])
    labels[2] = 0                                                  # a molecule without bonds: it has a graph at every cap
    counts = np.array([int(np.count_nonzero(l)) for l in labels])
    for cap in (0, 1, int(sorted(counts)[3]), int(max(counts))):
        for scope in ("largest", "whole"):
            host, _ = _check(atoms, labels, tables, cap=cap, scopes=(scope,))
            assert ((host.status == ref.NO_GRAPH) == (counts > cap)).all() and host.status[2] == 0
    # flags: a negative value means no graph, whatever the list holds (the Python layer passes none: the entry itself)
    batch = _decode(atoms, labels, E)
    flags = torch.tensor([0, -2, 5, -1, 0, -2], dtype=torch.int32, device="cuda")
    out = validity.MoleculeValidity.empty(B, N, batch.cap, "cuda")
    out.buffer.fill_(FILL)
    _lib.launch("dg_mol_validity", batch.buffer, batch.atoms.data_ptr(), batch.bonds.data_ptr(), batch.n_bonds.data_ptr(),
                batch.component.data_ptr(), batch.largest.data_ptr(), flags.data_ptr(), tables.atoms.data_ptr(),
                tables.n_atom_labels, tables.bonds.data_ptr(), tables.n_bond_labels, B, N, batch.cap, 1, ref.H_MASS,
                out.mol.data_ptr(), out.hcount.data_ptr(), out.kekule.data_ptr())
    mols = _mols(atoms, labels)
    want = [ref.validity(m["atoms"], m["bonds"], flag=f, scope=ref.LARGEST, component=m["component"], largest=m["largest"])
            for m, f in zip(mols, flags.tolist())]
    host, = _finish(out)
    ref.assert_batch_equals(host, want, mols)
    assert [w["mol"][0] == ref.NO_GRAPH for w in want] == [False, True, False, True, False, True]
    # another hydrogen mass reaches the sum (modulo 2^32)
    _lib.launch("dg_mol_validity", batch.buffer, batch.atoms.data_ptr(), batch.bonds.data_ptr(), batch.n_bonds.data_ptr(),
                None, None, None, tables.atoms.data_ptr(), tables.n_atom_labels, tables.bonds.data_ptr(), tables.n_bond_labels, B,
                N, batch.cap, 0, 0x7FFFFFFF, out.mol.data_ptr(), out.hcount.data_ptr(), out.kekule.data_ptr())
    host, = _finish(out)
    ref.assert_batch_equals(host, ref.validity_batch(mols, None, ref.WHOLE, h_mass=0x7FFFFFFF), mols)
    # an empty batch launches nothing
    empty = validity.check_molecules(_decode(atoms[:0], labels[:0], E), tables)
    assert len(empty) == 0 and empty.mol.shape == (0, 8)


def test_unknown_atom_and_bond_labels_and_a_valence_byte_of_nine():
    """Labels past the tables, empty rows, a bond row of order 0 / 4 / aromatic with order 2, and an atom row with a valence
    byte of 9 are all UNKNOWN -- for the molecules that use them, and only for those."""
    from druggen_amd import validity
    rng = np.random.default_rng(6)
    N = 12
    plain = [cref.from_edges(N, [(0, 1)]), cref.from_edges(N, [(0, 1), (1, 2), (2, 3)])]      # ethane, butane: known to both
    atoms, labels = _stack([ref.aromatic_like(rng, N, True) for _ in range(6)] + plain)
    short = validity.ValenceTables(np.array(ref.ATOM_ROWS[:4], dtype=np.uint32), np.array(ref.BOND_ROWS[:3], dtype=np.uint32), "cuda")
    rows = [list(r) for r in ref.ATOM_ROWS]
    rows[3][0] = 2 | 9 << 8                                        # O: a valence byte of 9
    bonds = list(ref.BOND_ROWS)
    bonds[2], bonds[3] = 2 | 1 << 8, 4                             # double: aromatic with order 2; triple: order 4
    odd = validity.ValenceTables(np.array(rows, dtype=np.uint32), np.array(bonds, dtype=np.uint32), "cuda")
    for tables in (short, odd):
        tab = dict(atom_rows=tables.atom_rows.tolist(), bond_rows=tables.bond_rows.tolist())
        host, want = _check(atoms, labels, tables, scopes=("largest", "whole"), **tab)
        assert (host.status[:6] == 2).any() and (host.status[6:] == 0).all()
        assert (host.hcount[host.status == 2] == 0xFF).all() and (host.deficiency[host.status == 2] == -1).all()


# ---- 6. atom order ----------------------------------------------------------------------------------------------------------------
def test_a_permuted_batch_gives_identical_rows_and_permuted_hydrogens():
    rng = np.random.default_rng(7)
    tables = _tables()
    N, copies = 33, 4
    base = [ref.aromatic_like(rng, N, k % 2 == 0) for k in range(8)]
    graphs, perms = [], []
    for g in base:
        graphs.append(g)
        perms.append(np.arange(N))
        for _ in range(copies - 1):
            a, l, perm = ref.renumbered(rng, *g)
            graphs.append((a, l))
            perms.append(perm)
    host, _ = _check(*_stack(graphs), tables, scopes=("whole",))
    for k in range(len(base)):
        first = copies * k
        for c in range(copies):
            assert host.mol[first + c].tolist() == host.mol[first].tolist()
            assert host.hcount[first + c].tolist() == host.hcount[first][perms[first + c]].tolist()
    assert {0, 5} <= set(host.status.tolist())


# ---- 7. stores, the sampler, a captured graph -------------------------------------------------------------------------------------
def test_validity_of_a_resident_store_in_uneven_chunks():
    """`validity_store` equals `check_molecules` on the whole set and the restatement, whatever the chunk (1, 7, n)."""
    from druggen_amd import validity
    from druggen_amd.resident import ResidentMolecules
    n, N = 11, 9
    graphs, atoms, labels = _store_graphs(n, N, E, 1)
    store = ResidentMolecules.from_graphs(graphs, device="cuda", m_dim=4, b_dim=E)
    tables = _tables()
    mols = _mols(atoms, labels)
    want = ref.validity_batch(mols)
    whole, = _finish(validity.check_molecules(_decode(atoms, labels, E), tables))
    for chunk in (1, 7, n):
        host, = _finish(validity.validity_store(store, tables, chunk=chunk))
        assert len(host) == n
        ref.assert_batch_equals(host, want, mols)
        assert np.array_equal(host.mol, whole.mol) and np.array_equal(host.hcount, whole.hcount)
    other, = _finish(validity.validity_store(store, tables, chunk=5, scope="whole"))
    ref.assert_batch_equals(other, ref.validity_batch(mols, scope=ref.WHOLE), mols)


@pytest.mark.parametrize("graph", [False, True])
def test_sampler_checks_its_batch(graph):
    """`MoleculeSampler(..., validity=tables)`: the record on the returned batch equals `check_molecules` on that batch field for
    field (graphed: a replay against the eager call), and the batch itself is bit for bit the one a sampler without tables
    returns, which carries no record."""
    from druggen_amd import synth, validity
    from druggen_amd.model import Generator
    from druggen_amd.sampling import MoleculeSampler
    N, Mn, B = 9, 13, 4
    net = Generator("relu", N, E, Mn, 0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
    params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=11)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net = net.cuda()
    decoder = {0: 0, 1: 6, 2: 7, 3: 8, 4: 9, 5: 15, 6: 16, 7: 17, 8: 35, 9: 53, 10: 34, 11: 14, 12: 5}
    tables = _tables(decoder)
    tab = dict(atom_rows=tables.atom_rows.tolist(), bond_rows=tables.bond_rows.tolist())
    rng = np.random.default_rng(4)
    inputs = []
    for _ in range(2):
        atoms, labels = _stack([cref.molecule_like(rng, N, b % 3) for b in range(B)])
        node, edge = dref.one_hot_logits(atoms, labels + labels.transpose(0, 2, 1), Mn, E)
        inputs.append((torch.from_numpy(edge).cuda(), torch.from_numpy(node).cuda()))
    with pytest.raises(TypeError, match="ValenceTables"):
        MoleculeSampler(net, *inputs[0], graph=False, validity=decoder)
    plain = MoleculeSampler(net, *inputs[0], graph=graph)
    checking = MoleculeSampler(net, *inputs[0], graph=graph, validity=tables)
    assert plain.validity is None
    for edge, node in inputs[::-1]:
        bare = plain.sample(edge, node)
        assert bare.validity is None and plain.validity is None
        before, = _finish(bare)
        batch = checking.sample(edge, node)
        assert batch.validity is checking.validity and isinstance(batch.validity, validity.MoleculeValidity)
        got, host = _finish(batch.validity, batch)
        for name in ("atoms", "n_bonds", "component", "n_components", "largest", "largest_size"):
            assert np.array_equal(getattr(host, name), getattr(before, name)), name
        assert all(np.array_equal(host.edge_list(b), before.edge_list(b)) for b in range(B))      # (rows past n_bonds are unwritten)
        eager, = _finish(validity.check_molecules(batch, tables))
        for name in ref.MOL_FIELDS + ("hcount",):
            assert np.array_equal(getattr(got, name), getattr(eager, name)), name
        rows = [min(int(n), host.cap) for n in host.n_bonds]
        assert all(np.array_equal(got.kekule[b, :rows[b]], eager.kekule[b, :rows[b]]) for b in range(B))
        mols = [dict(atoms=host.atoms[b], bonds=host.edge_list(b), n_bonds=int(host.n_bonds[b]), component=host.component[b],
                     largest=int(host.largest[b])) for b in range(B)]
        ref.assert_batch_equals(got, ref.validity_batch(mols, **tab), mols)


def test_a_captured_graph_follows_its_static_inputs():
    """Decode and check captured into one hipGraph with `out=`: the capture allocates nothing, and replays on new logits give
    the eager results, field for field and Kekule row for Kekule row, and the restatement's."""
    from druggen_amd import decode, validity
    rng = np.random.default_rng(8)
    B, N, M = 5, 9, 7
    tables = _tables()
    sets = [_stack([ref.aromatic_like(rng, N, b % 2 == 0) for b in range(B)]) for _ in range(3)]
    node, edge = (torch.from_numpy(4.0 * t).cuda() for t in dref.one_hot_logits(*sets[0], M, E))
    cap = N * (N - 1) // 2
    decoded = decode.MoleculeBatch.empty(B, N, cap, False, "cuda")
    out = validity.MoleculeValidity.empty(B, N, cap, "cuda")

    def chain():
        decode.decode_molecule_graphs(node, edge, out=decoded)
        validity.check_molecules(decoded, tables, "whole", out=out)
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
        eager, = _finish(validity.check_molecules(_decode(atoms, labels, E), tables, "whole"))
        mols = _mols(atoms, labels)
        assert np.array_equal(got.mol, eager.mol) and np.array_equal(got.hcount, eager.hcount)
        assert all(np.array_equal(got.kekule[b, :m["n_bonds"]], eager.kekule[b, :m["n_bonds"]]) for b, m in enumerate(mols))
        ref.assert_batch_equals(got, ref.validity_batch(mols, scope=ref.WHOLE), mols)
        seen.append(got.mol.tobytes())
    assert len(set(seen)) == 3
