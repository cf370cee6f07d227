"""GPU tests of the substructure matcher (`dg_mol_substructure` through `druggen_amd.substructure`) against the plain-Python
restatement of tests/mol_sub_ref.py, whose inputs are the restatements of tests/mol_valid_ref.py and tests/mol_desc_ref.py --
never the GPU's own verdicts, keys or classes.  Batches are built from label tensors as in tests/test_hip_mol_desc.py.  Every
output is an integer and a pinned value: every `mol` field, every hit count and every atom type is compared with `==`.  There is
no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_desc_ref as descref
import mol_fp_ref as fref
import mol_sub_ref as ref
import mol_valid_ref as vref
from test_hip_mol_canon import _finish, _mols, _stack, _store_graphs
from test_hip_mol_desc import _chain, _graph
from test_hip_mol_smiles import _decode
from test_mol_sub_host import (LATTICE_SIDE, dead_end_chain, fixture_sub_tables, fixture_wanted, golden_sub_rows, make_tables,
                               probe_patterns, table_args)

pytestmark = pytest.mark.gpu

E = 5      # bond labels of the test tables: none, single, double, triple, aromatic
FILL = 0xA5
C, N_, O = 1, 2, 3      # atom labels of mol_fp_ref.ATOM_DECODER


def _base_tables(atom_decoder=fref.ATOM_DECODER, bond_decoder=fref.BOND_DECODER):
    from druggen_amd import descriptors, validity
    return (validity.ValenceTables.from_decoders(atom_decoder, bond_decoder, "cuda"),
            descriptors.DescriptorTables.from_decoders(atom_decoder, bond_decoder, "cuda"))


def _probe_tables():
    typing, patterns = probe_patterns()
    return make_tables(typing=typing, patterns=patterns, device="cuda")


def _check(atoms, labels, stables, cap=None, scopes=("largest",), batch=None, known=None, vtab=None, dtab=None, base=None):
    """Kernel outputs of the batch against the restatement under every scope.  `known`: per molecule the deficiency of the
    aromatic graph where the validity restatement's matching refuses the size.  Returns the last scope's (host matches, host
    descriptors, host validity, wanted matches, wanted descriptors, wanted validity)."""
    from druggen_amd import canon, descriptors, substructure, validity
    vtables, dtables = base or _base_tables()
    batch = batch if batch is not None else _decode(atoms, labels, E, cap)
    mols = _mols(atoms, labels)
    vtab, dtab = vtab or {}, dtab or {}
    out = None
    for scope in scopes:
        checked = validity.check_molecules(batch, vtables, scope)
        described = descriptors.describe_molecules(batch, checked, dtables, scope)
        host, hdesc, hval = _finish(substructure.match_molecules(batch, described, stables), described, checked)
        code = canon.SCOPES[scope]
        if known is None:
            valids = vref.validity_batch(mols, cap, code, **vtab)
        else:
            valids = [vref.validity(m["atoms"], m["bonds"], n_bonds=m["n_bonds"], cap=cap, scope=code, component=m["component"],
                                    largest=m["largest"], deficiency=d, **vtab) for m, d in zip(mols, known)]
        descs = descref.describe_batch(mols, valids, cap, code, **dtab)
        want = ref.match_batch(mols, descs, **table_args(stables))
        assert hdesc.status.tolist() == [d["desc"][0] for d in descs]
        ref.assert_batch_equals(host, want)
        assert host.names == stables.names
        out = host, hdesc, hval, want, descs, valids
    return out


# ---- 1. the fixture molecules ---------------------------------------------------------------------------------------------------
def test_fixture_molecules_equal_the_restatement_and_their_recorded_rows():
    from druggen_amd import decode, substructure
    strings, atoms, labels, atom_dec, bond_dec, vtab, dtab, host_tables = fixture_sub_tables()
    stables = make_tables(typing=None, patterns=None, atom_decoder=atom_dec, bond_decoder=bond_dec, device="cuda")
    assert np.array_equal(stables.pattern_rows, host_tables.pattern_rows)
    node, edge = dref.one_hot_logits(atoms, labels, len(atom_dec), len(bond_dec))
    batch = decode.decode_molecule_graphs(torch.from_numpy(4.0 * node).cuda(), torch.from_numpy(4.0 * edge).cuda())
    golden = golden_sub_rows()
    for scope, code in (("largest", descref.LARGEST), ("whole", descref.WHOLE)):
        host, hdesc, hval, want, _, _ = _check(atoms, labels, stables, scopes=(scope,), batch=batch, vtab=vtab, dtab=dtab,
                                               base=_base_tables(atom_dec, bond_dec))
        assert want == [w for _, _, w in fixture_wanted(code)]
        valid = [g["status"] == 0 for g in golden]
        assert host.status.tolist() == [g["status"] for g in golden] and not host.n_untyped.any() and not host.n_over.any()
        assert host.sum0[valid].tolist() == [g["logp_1e4"] for g in golden if g["status"] == 0]
        assert host.logp[valid].tolist() == [g["logp_1e4"] / 1e4 for g in golden if g["status"] == 0]
        for name, _ in substructure.GROUPS:
            assert host.count(name)[valid].tolist() == [g["groups"][name] for g in golden if g["status"] == 0], name
        assert substructure.lipinski_rules5(hval, hdesc, host)[valid].tolist() == [g["lipinski5"] for g in golden if g["status"] == 0]


# ---- 2. seeded molecule-like graphs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 33, 64, 65, 96, 97, 255, 256])
def test_molecule_like_graphs_equal_the_restatement(N):
    """Rings and chains with aromatic labels (mol_valid_ref.aromatic_like, most of them clean so that most are valid) under the
    built-in and the probe patterns: a single atom, a single bond, the smallest triangle, the wave boundaries (64 / 65 atoms: one /
    two waves of anchors per pattern), 96 / 97 and the maximum; both scopes; nothing runs over; and a bond list one row short of
    the largest molecule (no graph)."""
    rng = np.random.default_rng([N, 332])
    stables = _probe_tables()
    B = 8 if N <= 97 else 4
    graphs = [vref.aromatic_like(rng, N, b % 4 != 3) for b in range(B)]
    if N == 3:
        graphs[0] = _graph(3, [C, N_, O], [(0, 1, 1), (1, 2, 1), (0, 2, 1)])      # the smallest triangle
        graphs[1] = _graph(3, [C, C, O], [(0, 1, 2), (1, 2, 1)])
    atoms, labels = _stack(graphs)
    host, _, _, want, _, _ = _check(atoms, labels, stables, scopes=("largest", "whole"))
    assert 0 in host.status and not host.n_over.any()
    if N >= 33:
        assert (host.status != 0).any() and host.n_typed.max() > N // 2 and host.n_patterns_hit.max() >= 10
        assert host.hits[:, stables.index["ring6"]].max() >= 6
    if N == 3:
        name = {k: n for n, k in stables.index.items()}
        assert [name[t] for t in host.atom_type[0]] == ["C.sp3.hetero", "N.secondary", "O"] and host.hits[0, stables.index["ringbond"]] == 0
        assert [name[t] for t in host.atom_type[1]] == ["C.dbl", "C.dbl", "O.hydroxyl"] and host.sum0[:2].tolist() == [-5213, 1222]
    most = max(int(np.count_nonzero(l)) for l in labels)
    host, _, _, _, _, _ = _check(atoms, labels, stables, cap=max(most - 1, 0))
    if most > 0:
        cut = host.status == vref.NO_GRAPH
        assert cut.any() and not host.hits[cut].any() and (host.atom_type[cut] == -1).all() and not host.mol[cut][:, 1:].any()


# ---- 3. the strided pair loop and its tail ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_patterns", [0, 1, 63, 64, 65, 1024])
def test_pattern_counts_around_the_strides(n_patterns):
    """N = 7, so that the pair count n_patterns x 7 is 0, 7 (one wave, mostly idle), 441, 448 and 455 (the last wave of 256
    threads' second round full, one short, one over) and 7168; typing and counted rows interleaved in one pool."""
    pool = [("[C]", 1), ("[C;H3]", 0), ("[*]~[*]", 0), ("[N,O]", 1), ("[C]-[!C]", 1), ("[*]1~[*]~[*]~[*]~[*]~1", 0),
            ("[C](~[*])(~[*])~[*]", 0), ("[O;H1]", 1), ("[S]", 0), ("[*;R]", 1), ("[C]=[*]", 0), ("[*]~[*]~[*]~[*]~[*]~[*]~[*]", 0)]
    typing = [(f"t{k}", pool[k % len(pool)][0], 10 + k, 3 * k + 1, -k, 2) for k in range(n_patterns) if pool[k % len(pool)][1]]
    counted = [(f"c{k}", pool[k % len(pool)][0]) for k in range(n_patterns) if not pool[k % len(pool)][1]]
    stables = make_tables(typing=typing, patterns=counted, device="cuda")
    assert stables.n_patterns == n_patterns
    rng = np.random.default_rng([n_patterns, 7])
    atoms, labels = _stack([vref.aromatic_like(rng, 7, True) for _ in range(8)])
    host, _, _, want, _, _ = _check(atoms, labels, stables, scopes=("whole",))
    assert host.hits.shape == (8, n_patterns) and (host.status == 0).sum() >= 4
    if n_patterns >= 63:
        assert host.hits[:, -1].any() or host.hits[:, -2].any() or host.hits[:, -3].any()      # the tail of the table is reached
        assert host.sum1.any() and host.n_patterns_hit.max() > n_patterns // 3
    if n_patterns == 0:
        assert not host.mol[:, 2].any() and (host.atom_type == -1).all() and (host.n_untyped == host.n_heavy).all()


# ---- 4. the largest pattern; closures on fused rings ----------------------------------------------------------------------------------
def test_a_sixteen_atom_pattern_on_chains_of_fifteen_and_sixteen_atoms():
    rows = [("chain16", "[C]" * 16), ("chain15", "[C]" * 15), ("ring16", "[C]1" + "[C]" * 14 + "[C]1"), ("ring15", "[C]1" + "[C]" * 13 + "[C]1")]
    stables = make_tables(patterns=rows, device="cuda")
    N = 20
    graphs = [_chain(15, N), _chain(16, N), _chain(17, N), tuple(np.pad(x, [(0, N - 16)] * x.ndim) for x in cref.cycle(16)),
              tuple(np.pad(x, [(0, N - 15)] * x.ndim) for x in cref.cycle(15))]
    host, _, _, _, _, _ = _check(*_stack(graphs), stables, scopes=("whole",))
    #                              chain16 from both ends; chain15 from the ends, and from the ends' neighbours in a longer chain
    assert host.hits.tolist() == [[0, 2, 0, 0], [2, 4, 0, 0], [4, 6, 0, 0], [16, 16, 16, 0], [0, 15, 0, 15]]
    assert not host.n_over.any()


def test_closures_on_fused_rings():
    """Naphthalene-, azulene- and anthracene-like aromatic systems and their saturated copies: six- and five-ring closures, the
    two-closure fused pattern, and a ring bond that is no bond of the ring walked (the fusion bond closes both rings)."""
    rows = [("ring6", "[C]1:[C]:[C]:[C]:[C]:[C]:1"), ("ring5", "[*]1~[*]~[*]~[*]~[*]~1"), ("ring7", "[*]1~[*]~[*]~[*]~[*]~[*]~[*]~1"),
            ("fused66", "[*]1~[*]~[*]~[*]2~[*]~[*]~[*]~[*]~[*]~2~[*]~1"), ("fused57", "[*]1~[*]~[*]~[*]2~[*]~[*]~[*]~[*]~[*]~[*]~2~1"),
            ("fusion", "[C;D3](~@[C;D3])(~[C;D2])~[C;D2]"), ("perimeter10", "[*]1" + "~[*;D2]" * 3 + "~[*]" * 5 + "~[*]~1")]
    stables = make_tables(patterns=rows, device="cuda")
    N = 16
    systems = [[6, 6], [5, 7], [6, 6, 6], [7, 5], [6]]
    graphs = [vref.fused_chain(s, N)[:2] for s in systems]
    graphs += [(a, np.where(l == 4, 1, 0)) for a, l in graphs[:2]]      # decalin- and bicyclo[5.3.0]decane-like
    host, _, _, _, _, _ = _check(*_stack(graphs), stables, scopes=("whole",))
    assert host.status.tolist() == [0] * 7 and not host.n_over.any()
    hits = {name: host.hits[:, k].tolist() for name, k in stables.index.items()}
    assert hits["ring6"] == [10, 0, 14, 0, 6, 0, 0] and hits["ring5"] == [0, 5, 0, 5, 0, 0, 5] and hits["ring7"] == [0, 7, 0, 7, 0, 0, 7]
    # the fused pattern starts two atoms away from a fusion atom: four such atoms in naphthalene, eight in anthracene
    assert hits["fused66"] == [4, 0, 8, 0, 0, 4, 0] and hits["fused57"][0] == 0 and hits["fused57"][4] == 0
    assert hits["fused57"][1] == hits["fused57"][3] == hits["fused57"][6] > 0 and hits["fusion"] == [2, 2, 4, 2, 0, 2, 2]


# ---- 5. the step bound --------------------------------------------------------------------------------------------------------------
def test_the_lattice_runs_over_exactly_where_the_restatement_does():
    """The 6 x 6 lattice of carbons as a real molecule through the whole chain (decode, validity, descriptors, matcher): the
    10-atom dead-end chain is OVER from the centre, the 4-atom one completes everywhere, and n_over and hits equal the
    restatement's, beside two ordinary molecules in the same batch."""
    rows = [("dead10", dead_end_chain(10)), ("dead4", dead_end_chain(4)), ("dead8", dead_end_chain(8)), ("square", "[C]1[C][C][C]1"),
            ("chain16", "~".join(["[*]"] * 16))]
    stables = make_tables(typing=[("c", "[C]", 5, 1)], patterns=rows, device="cuda")
    side = LATTICE_SIDE
    l_atoms, l_rows = ref.lattice(side)
    N = side * side
    rng = np.random.default_rng(6)
    graphs = [_graph(N, l_atoms, l_rows), vref.aromatic_like(rng, N, True), _graph(N, *ref.lattice(side - 1))]
    host, _, _, want, descs, _ = _check(*_stack(graphs), stables, scopes=("whole",))
    assert host.status.tolist()[0::2] == [0, 0] and host.n_over[0] > 0 and host.n_over[0] == want[0]["mol"][7]
    steps = {}
    m = _mols(*_stack(graphs))[0]
    ref.match(m["atoms"], m["bonds"], descs[0], steps_out=steps, **table_args(stables))
    centre = (side // 2) * side + side // 2
    assert steps[(1, centre)] == (-1, 4096) and steps[(2, centre)][0] == 0 and steps[(2, centre)][1] < 4096
    assert host.hits[0].tolist() == [36, 0, 0, 0, 36, 36] and host.n_typed[0] == 36 and host.sum0[0] == 36 * 5 + (4 * 2 + 16 * 1)


# ---- 6. every element is written, nothing outside -----------------------------------------------------------------------------------
def test_out_reuse_over_a_filled_buffer_leaves_nothing_unwritten():
    """The record is a view into a buffer filled with 0xA5 bytes, a guard of 256 bytes on both sides: after the call every `mol`,
    `hits` and `atom_type` element equals the restatement (molecules without a graph and invalid ones included), the padding
    between the fields and the guards still hold the fill, and a second run into a second buffer gives the same bytes."""
    from druggen_amd import descriptors, substructure, validity
    rng = np.random.default_rng(4)
    vtables, dtables = _base_tables()
    stables = _probe_tables()
    B, N, G = 8, 33, 256
    atoms, labels = _stack([vref.aromatic_like(rng, N, b % 3 != 2) for b in range(B)])
    cap = max(int(np.count_nonzero(l)) for l in labels) - 1
    batch = _decode(atoms, labels, E, cap)
    checked = validity.check_molecules(batch, vtables, "whole")
    described = descriptors.describe_molecules(batch, checked, dtables, "whole")
    table, size = substructure.MoleculeMatches.layout(B, N, stables.n_patterns)
    runs = []
    for _ in range(2):
        buf = torch.full((G + size + G,), FILL, dtype=torch.uint8, device="cuda")
        out = substructure.MoleculeMatches(buf[G:G + size], B, N, stables.n_patterns)
        assert substructure.match_molecules(batch, described, stables, out=out) is out
        host, = _finish(out)
        runs.append(buf.cpu().numpy())
    mols = _mols(atoms, labels)
    descs = descref.describe_batch(mols, vref.validity_batch(mols, cap, descref.WHOLE), cap, descref.WHOLE)
    want = ref.match_batch(mols, descs, **table_args(stables))
    ref.assert_batch_equals(host, want)
    assert any(w["mol"][0] == vref.NO_GRAPH for w in want) and sum(w["mol"][0] == 0 for w in want) >= 2
    assert np.array_equal(runs[0], runs[1])
    written = np.zeros(G + size + G, dtype=bool)
    for name in ("mol", "hits", "atom_type"):
        off, nbytes = table[name][:2]
        written[G + off:G + off + nbytes] = True
    assert (runs[0][~written] == FILL).all() and (~written).sum() >= 2 * G
    with pytest.raises(ValueError, match="out="):
        substructure.match_molecules(batch, described, stables, out=substructure.MoleculeMatches.empty(B, N, 3, "cuda"))
    # an empty batch launches nothing
    empty = _decode(atoms[:0], labels[:0], E)
    none = validity.check_molecules(empty, vtables)
    got = substructure.match_molecules(empty, descriptors.describe_molecules(empty, none, dtables), stables)
    assert len(got) == 0 and got.hits.shape == (0, stables.n_patterns)


def test_foreign_arrays_stay_inside_their_buffers():
    """Inputs outside the definition: a descriptor record that claims status 0 over graphs it was not made from -- an atom with
    nine and with eleven bonds, atom indices >= N, atom labels >= n_atom_labels, bond labels >= n_bond_labels and UNKNOWN ones,
    a self bond, keys with every field at its largest.  The results have no meaning; only the guard bytes around the three
    outputs are checked, and that the call ends."""
    from druggen_amd import descriptors, substructure
    from druggen_amd.decode import MoleculeBatch
    stables = _probe_tables()
    B, N, G = 4, 12, 256
    cap = N * (N - 1) // 2
    batch = MoleculeBatch.empty(B, N, cap, False, "cuda")
    batch.buffer.zero_()
    rows = np.zeros((B, cap, 4), dtype=np.uint8)
    star9 = [(k, 0, 1) for k in range(1, 10)]                                              # degree 9
    star11 = [(k, 0, 1 + k % 4) for k in range(1, 12)]                                     # degree 11, every bond label
    wild = [(200, 0, 1), (3, 255, 1), (4, 4, 1), (5, 1, 77), (6, 1, 0), (7, 1, 255), (2, 1, 1), (3, 2, 4), (8, 3, 1)]
    ring = [(k, k - 1, 4) for k in range(1, 12)] + [(11, 0, 4)] + [(k, 0, 1) for k in range(2, 11)]      # a wheel: degree 11 at the hub
    for b, listed in enumerate((star9, star11, wild, ring)):
        rows[b, :len(listed), :3] = listed
        batch.n_bonds[b] = len(listed)
    batch.bonds.copy_(torch.from_numpy(rows))
    batch.atoms.copy_(torch.from_numpy(np.array([[C] * N, [C, N_, O, 4, 5, 6] * 2, [200, 7, 255, C] * 3, [C] * N], dtype=np.uint8)))
    described = descriptors.MoleculeDescriptors.empty(B, N, cap, "cuda")
    described.buffer.zero_()                                                               # status 0 everywhere
    keys = np.full((B, N), C | 4 << 12, dtype=np.uint32)
    keys[1] = 0x01FFFFFF                                                                   # every field at its largest
    keys[2, ::3] = 0xFFFFFFFF                                                              # some atoms outside the scope
    keys[3] = C | 15 << 8 | 15 << 12 | 7 << 16 | 3 << 19 | 7 << 21 | 1 << 24
    described.atom_key.copy_(torch.from_numpy(keys.view(np.int32)))
    described.bond_class.fill_(3)                                                          # every row a ring BOND
    table, size = substructure.MoleculeMatches.layout(B, N, stables.n_patterns)
    buf = torch.full((G + size + G,), FILL, dtype=torch.uint8, device="cuda")
    out = substructure.MoleculeMatches(buf[G:G + size], B, N, stables.n_patterns)
    substructure.match_molecules(batch, described, stables, out=out)
    _finish(out)
    got = buf.cpu().numpy()
    written = np.zeros(G + size + G, dtype=bool)
    for name in ("mol", "hits", "atom_type"):
        off, nbytes = table[name][:2]
        written[G + off:G + off + nbytes] = True
    assert (got[~written] == FILL).all()


# ---- 7. atom order ----------------------------------------------------------------------------------------------------------------
def test_a_permuted_batch_gives_identical_rows_and_permuted_types():
    rng = np.random.default_rng(7)
    stables = _probe_tables()
    N, copies = 33, 4
    base = [vref.aromatic_like(rng, N, True) for k in range(4)]
    graphs, perms = [], []
    for g in base:
        graphs.append(g)
        perms.append(np.arange(N))
        for _ in range(copies - 1):
            a, l, perm = vref.renumbered(rng, *g)
            graphs.append((a, l))
            perms.append(perm)
    host, _, _, _, _, _ = _check(*_stack(graphs[:8]), stables, scopes=("whole",))
    more, _, _, _, _, _ = _check(*_stack(graphs[8:]), stables, scopes=("whole",))
    mol, hits, types = (np.concatenate([getattr(host, n), getattr(more, n)]) for n in ("mol", "hits", "atom_type"))
    assert not mol[:, 7].any()
    for k in range(len(base)):
        first = copies * k
        for c in range(copies):
            assert mol[first + c].tolist() == mol[first].tolist() and hits[first + c].tolist() == hits[first].tolist()
            assert types[first + c].tolist() == types[first][perms[first + c]].tolist()
    assert (mol[:, 0] == 0).sum() >= 8 and (mol[:, 6] >= 8).any()


# ---- 8. stores, the sampler, the rule count -------------------------------------------------------------------------------------------
def test_matches_of_a_resident_store_do_not_depend_on_the_chunk():
    from druggen_amd import descriptors, substructure, validity
    from druggen_amd.resident import ResidentMolecules
    n, N = 11, 9
    graphs, atoms, labels = _store_graphs(n, N, E, 1)
    store = ResidentMolecules.from_graphs(graphs, device="cuda", m_dim=4, b_dim=E)
    vtables, dtables = _base_tables()
    stables = _probe_tables()
    mols = _mols(atoms, labels)
    descs = descref.describe_batch(mols, vref.validity_batch(mols))
    want = ref.match_batch(mols, descs, **table_args(stables))
    seen = []
    for chunk in (1, 7, n, 64):
        checked, described, out = substructure.match_store(store, vtables, dtables, stables, chunk=chunk)
        host, hdesc, hval = _finish(out, described, checked)
        assert len(host) == n == len(hdesc) == len(hval) and host.names == stables.names
        ref.assert_batch_equals(host, want)
        descref.assert_batch_equals(hdesc, descs)
        seen.append(host.mol.tobytes() + host.hits.tobytes() + host.atom_type.tobytes())      # (the padding between them is unwritten)
    assert len(set(seen)) == 1
    whole = ref.match_batch(mols, descref.describe_batch(mols, vref.validity_batch(mols, scope=descref.WHOLE), scope=descref.WHOLE),
                            **table_args(stables))
    host, = _finish(substructure.match_store(store, vtables, dtables, stables, chunk=5, scope="whole")[2])
    ref.assert_batch_equals(host, whole)


@pytest.mark.parametrize("graph", [False, True])
def test_sampler_matches_its_batch(graph):
    """`MoleculeSampler(..., validity=, descriptors=, substructures=)`: the record on the returned batch equals
    `match_molecules` on that batch field for field (graphed: a replay against the eager call) and the restatement, and a
    sampler without the tables carries none."""
    from druggen_amd import substructure, synth
    from druggen_amd.model import Generator
    from druggen_amd.sampling import MoleculeSampler
    N, Mn, B = 9, 13, 4
    net = Generator("relu", N, E, Mn, 0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
    params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=11)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net = net.cuda()
    decoder = {0: 0, 1: 6, 2: 7, 3: 8, 4: 9, 5: 15, 6: 16, 7: 17, 8: 35, 9: 53, 10: 34, 11: 14, 12: 5}
    vtables, dtables = _base_tables(decoder)
    stables = make_tables(typing=None, patterns=None, atom_decoder=decoder, device="cuda")
    vtab = dict(atom_rows=vtables.atom_rows.tolist(), bond_rows=vtables.bond_rows.tolist())
    dtab = dict(bond_rows=dtables.bond_rows.tolist(), atom_flags=dtables.atom_flag_rows.tolist(),
                atom_class=dtables.atom_class_rows.tolist(), env=descref.env_for(decoder))
    rng = np.random.default_rng(4)
    inputs = []
    for _ in range(2):
        atoms, labels = _stack([cref.molecule_like(rng, N, b % 3) for b in range(B)])
        node, edge = dref.one_hot_logits(atoms, labels + labels.transpose(0, 2, 1), Mn, E)
        inputs.append((torch.from_numpy(edge).cuda(), torch.from_numpy(node).cuda()))
    with pytest.raises(ValueError, match="needs validity= and descriptors="):
        MoleculeSampler(net, *inputs[0], graph=False, validity=vtables, substructures=stables)
    plain = MoleculeSampler(net, *inputs[0], graph=graph, validity=vtables, descriptors=dtables)
    matching = MoleculeSampler(net, *inputs[0], graph=graph, validity=vtables, descriptors=dtables, substructures=stables)
    assert plain.matches is None
    for edge, node in inputs[::-1]:
        bare = plain.sample(edge, node)
        assert bare.matches is None and plain.matches is None
        batch = matching.sample(edge, node)
        assert batch.matches is matching.matches and isinstance(batch.matches, substructure.MoleculeMatches)
        got, gdesc, gval, host = _finish(batch.matches, batch.descriptors, batch.validity, batch)
        eager, = _finish(substructure.match_molecules(batch, batch.descriptors, stables))
        assert all(np.array_equal(getattr(got, name), getattr(eager, name)) for name in ("mol", "hits", "atom_type"))
        mols = [dict(atoms=host.atoms[b], bonds=host.edge_list(b), n_bonds=int(host.n_bonds[b]), component=host.component[b],
                     largest=int(host.largest[b])) for b in range(B)]
        descs = descref.describe_batch(mols, vref.validity_batch(mols, **vtab), **dtab)
        descref.assert_batch_equals(gdesc, descs)
        ref.assert_batch_equals(got, ref.match_batch(mols, descs, **table_args(stables)))


def test_the_five_rule_count_on_the_device_equals_the_host():
    """`lipinski_rules5` on the device records against the host copies and the restatement: chains of 13 and 14 carbons (10 and 11
    rotatable bonds; both have a logP above 5 under the built-in table), a chain of 35 carbons, a polyol whose logP is below -2, a
    molecule with a selenium (no typing row: the logP rule does not count), ethanol (all five) and an invalid one."""
    from druggen_amd import descriptors, substructure, validity
    N = 40
    polyol = _graph(N, [C] * 15 + [O] * 15, [(i, i + 1, 1) for i in range(14)] + [(i, 15 + i, 1) for i in range(15)])
    selenide = _chain(5, N)
    selenide[0][2] = 6
    graphs = [_chain(13, N), _chain(14, N), _chain(35, N), polyol, selenide, _graph(N, [C, C, O], [(0, 1, 1), (1, 2, 1)]),
              _graph(N, [C, C], [(0, 1, 4)])]
    vtables, dtables = _base_tables()
    stables = make_tables(typing=None, patterns=None, device="cuda")
    atoms, labels = _stack(graphs)
    batch = _decode(atoms, labels, E)
    checked = validity.check_molecules(batch, vtables)
    described = descriptors.describe_molecules(batch, checked, dtables)
    matches = substructure.match_molecules(batch, described, stables)
    rules = substructure.lipinski_rules5(checked, described, matches)
    assert rules.is_cuda and rules.dtype == torch.int32 and matches.logp.is_cuda and matches.count("alcohol").is_cuda
    host, hdesc, hval = _finish(matches, described, checked)
    mols = _mols(atoms, labels)
    valids = vref.validity_batch(mols)
    descs = descref.describe_batch(mols, valids)
    want = ref.match_batch(mols, descs, **table_args(stables))
    ref.assert_batch_equals(host, want)
    wanted = [ref.lipinski_rules5(v["mol"], d["desc"], w["mol"]) for v, d, w in zip(valids, descs, want)]
    assert rules.tolist() == wanted == substructure.lipinski_rules5(hval, hdesc, host).tolist()
    # a chain of n carbons: 2 x (1441 + 3 x 1230) + (n - 2) x (1441 + 2 x 1230)
    assert host.sum0.tolist()[:3] == [2 * 5131 + (n - 2) * 3901 for n in (13, 14, 35)] and host.sum0[0] > 50000
    assert host.sum0[3] < -20000 and host.n_untyped.tolist() == [0, 0, 0, 0, 1, 0, 0] and host.count("alcohol").tolist() == [0, 0, 0, 15, 0, 1, 0]
    #                logP 5.3  ... and rot 11  ... and rot 32  only the mass  Se untyped  ethanol  invalid
    assert rules.tolist() == [4, 3, 3, 1, 4, 5, 0]
