"""GPU tests of the SMILES writer (`dg_mol_smiles` through `druggen_amd.smiles_out`) against the plain-Python restatement of
tests/mol_smiles_ref.py, and -- without it -- against the project's own parser.  Batches are built from label tensors as in
tests/test_hip_mol_canon.py (logits = 4 x one-hot, the reference molecules from tests/decode_graph_ref.py, not from the GPU
decode).  Every output is an integer or a byte: every comparison is `==`."""
import numpy as np
import pytest
import torch

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_smiles_ref as ref
from test_hip_mol_canon import _clip, _finish, _mols, _stack

pytestmark = pytest.mark.gpu

M = 7      # atom labels 0..6: pad, C, N, O, S, Cl, Se (ref.ATOM_DECODER)


def _tables():
    from druggen_amd import smiles_out
    return smiles_out.SmilesTables.from_decoders(ref.ATOM_DECODER, ref.BOND_DECODER, "cuda")


def _decode(atoms, labels, E, cap=None, out=None):
    from druggen_amd import decode
    node, edge = dref.one_hot_logits(atoms, labels, M, E)
    return decode.decode_molecule_graphs(torch.from_numpy(4.0 * node).cuda(), torch.from_numpy(4.0 * edge).cuda(),
                                         bond_cap=cap, out=out)


def _family(name, rng, B, N, E):
    """B molecules of N positions, labels below E: the families of tests/test_hip_mol_canon.py over seven atom labels, and the
    molecule-like one once more with six elements and four bond types."""
    if name in ("molecule-like", "one label", "relabelled"):
        graphs = [cref.molecule_like(rng, N, (0, 1, 2, 4)[b % 4], name == "one label") for b in range(B)]
        if name == "relabelled":
            graphs = [ref.relabelled(rng, *g) for g in graphs]
    elif name == "dense":      # a random label per pair: the untrained generator's regime
        graphs = [(rng.integers(0, M, N), np.tril(rng.integers(0, E, (N, N)), -1)) for _ in range(B)]
    elif name == "no bonds":
        graphs = [(np.full(N, 1 + b % 2), dref.empty_graph(N)) for b in range(B)]
    elif name == "all pad":
        graphs = [(np.zeros(N, dtype=np.int64), dref.empty_graph(N)) for _ in range(B)]
    elif name == "cycles and a star":
        graphs = [cref.cycle(N, label=1 + 3 * (b % 4 == 2)) if b % 2 == 0 else (np.ones(N, dtype=np.int64), dref.star(N, b % N))
                  for b in range(B)]
    else:                      # two components of equal size (N even) or sizes that differ by one
        graphs = [(1 + (np.arange(N) + b) % 2 * (b % 2), dref.two_equal_components(N)) for b in range(B)]
    atoms, labels = _stack(graphs)
    return atoms, _clip(labels, E)


FAMILIES = ("molecule-like", "relabelled", "one label", "dense", "no bonds", "all pad", "cycles and a star", "two components")
SHAPES = [(1, 1), (3, 2), (5, 9), (4, 45), (3, 64), (3, 65), (2, 256), (257, 5)]


def _check(atoms, labels, E, cap=None, scope="largest", str_cap=None, tables=None):
    from druggen_amd import canon, smiles_out
    tables = tables or _tables()
    got = smiles_out.write_smiles(_decode(atoms, labels, E, cap), tables, scope, str_cap)
    want = ref.write_batch(_mols(atoms, labels), tables.atom_rows, tables.bond_rows, cap, canon.SCOPES[scope], str_cap)
    got, = _finish(got)
    ref.assert_batch_equals(got, want)
    return got


@pytest.mark.parametrize("E", [2, 5])
@pytest.mark.parametrize("B,N", SHAPES)
def test_bytes_equal_the_restatement(B, N, E):
    """text (all str_cap bytes), length, n_written and order of every family at this shape, with an ample bond list and with
    one a row short of the largest molecule (-2); both scopes where they differ.  The shapes cover the 64-lane boundary, the
    LDS maximum (N = 256) and more molecules than one dispatch wave of workgroups; the dense family answers -3 from N = 45 on."""
    rng = np.random.default_rng([B, N, E])
    tables = _tables()
    for name in FAMILIES:
        atoms, labels = _family(name, rng, B, N, E)
        scopes = ("largest", "whole") if name in ("two components", "all pad", "molecule-like", "no bonds") else ("largest",)
        most = max(int(np.count_nonzero(l)) for l in labels)
        for scope in scopes:
            got = _check(atoms, labels, E, scope=scope, tables=tables)
            if name == "no bonds":
                assert (got.n_written == (1 if scope == "largest" else N)).all()
            if name == "dense" and N >= 45:
                assert (got.length == ref.RINGS).all() and not got.text.any()
            if name in ("molecule-like", "relabelled", "one label", "cycles and a star"):
                assert (got.length > 0).all()
        got = _check(atoms, labels, E, scope="whole", cap=max(most - 1, 0), tables=tables)
        if most > 0:
            assert (got.length == ref.NO_GRAPH).any()


@pytest.mark.parametrize("B,N", [(4, 45), (2, 256)])
def test_strings_parse_back_to_the_input_graph(B, N):
    """Independent of the restatement: `smiles.parse_smiles` of every string is the input graph read through `order`, exactly --
    atomic numbers, bonds, bond types.  None is left out."""
    from druggen_amd import smiles_out
    rng = np.random.default_rng([B, N, 11])
    tables = _tables()
    for name in ("molecule-like", "relabelled"):
        atoms, labels = _family(name, rng, B, N, 5)
        for scope in ("whole", "largest"):
            got, = _finish(smiles_out.write_smiles(_decode(atoms, labels, 5), tables, scope))
            strings = got.strings()
            for b in range(B):
                n = int(got.n_written[b])
                assert got.length[b] > 0 and n == N and len(strings[b]) == got.length[b], (name, b, got.length[b])
                ref.parse_back(strings[b], atoms[b], labels[b], got.order[b, :n].tolist())


def test_strings_from_forms_do_not_depend_on_the_atom_order():
    """Renumbered copies of molecules whose forms have n_splits == 0 give the same bytes, two different molecules different
    ones, each string parses back to the form it was written from, and a molecule without a form (n_splits == -2) answers -2."""
    from druggen_amd import canon, smiles_out
    rng = np.random.default_rng(326)
    N, E, copies = 17, 5, 3
    tables = _tables()
    base = [ref.relabelled(rng, *cref.molecule_like(rng, N, k % 3)) for k in range(12)]
    atoms, labels = _stack([cref.renumbered(rng, *g) if c else g for g in base for c in range(copies)])
    B = len(atoms)
    forms = canon.canonical_forms(_decode(atoms, labels, E), "whole")
    with pytest.raises(ValueError, match="carries its scope"):
        smiles_out.write_smiles(forms, tables)
    got, host = _finish(smiles_out.write_smiles(forms, tables, scope="whole"), forms)
    strings = got.strings()
    settled = [k for k in range(len(base)) if (host.n_splits[copies * k:copies * (k + 1)] == 0).all()]
    assert len(settled) >= 4, host.n_splits
    for k in settled:
        rows = got.text[copies * k:copies * (k + 1)]
        assert got.length[copies * k] > 0 and (rows == rows[0]).all() and len(set(strings[copies * k:copies * (k + 1)])) == 1
    assert len({strings[copies * k] for k in settled}) == len({host.form(copies * k) for k in settled}) > 1
    for b in range(B):      # the string is the form: parsed back through `order` (ranks), it is canon_atoms / canon_bonds
        n, nb, canon_atoms, canon_bonds = host.form(b)
        dense = np.zeros((N, N), dtype=np.int64)
        for hi, lo, l in canon_bonds:
            dense[hi, lo] = l
        assert int(got.n_written[b]) == n == N
        ref.parse_back(strings[b], canon_atoms, dense, got.order[b, :n].tolist())
    # the restatement under the forms scope, and forms without a graph
    most = max(int(np.count_nonzero(l)) for l in labels)
    cut = canon.canonical_forms(_decode(atoms, labels, E, most - 1), "whole")
    got, host = _finish(smiles_out.write_smiles(cut, tables, scope="whole"), cut)
    assert (host.n_splits == -2).any() and (host.n_splits >= 0).any()
    want = [ref.write(host.canon_atoms[b], host.canon_bonds[b, :, :3], tables.atom_rows, tables.bond_rows,
                      n_bonds=int(host.n_bonds[b]), cap=host.cap, flag=int(host.n_splits[b]), scope=ref.FORMS) for b in range(B)]
    ref.assert_batch_equals(got, want)
    assert ((got.length == ref.NO_GRAPH) == (host.n_splits == -2)).all() and not got.text[host.n_splits == -2].any()


def test_dirty_buffers_and_a_captured_graph_give_the_eager_result():
    from druggen_amd import decode, smiles_out
    rng = np.random.default_rng(52)
    B, N, E = 5, 9, 5
    tables = _tables()
    sets = [_family("relabelled", rng, B, N, E) for _ in range(3)]
    batch = _decode(*sets[0], E)
    fresh, = _finish(smiles_out.write_smiles(batch, tables, "whole"))
    for fill in (0xAA, 0x00):
        out = smiles_out.SmilesBatch.empty(B, N, 8 * N, "cuda")
        out.buffer.fill_(fill)
        assert smiles_out.write_smiles(batch, tables, "whole", out=out) is out
        dirty, = _finish(out)
        for name in ("length", "n_written", "order", "text"):      # (the packed buffer has alignment gaps between its fields)
            assert np.array_equal(getattr(dirty, name), getattr(fresh, name)), name
    with pytest.raises(ValueError, match="out="):
        smiles_out.write_smiles(batch, tables, out=smiles_out.SmilesBatch.empty(B, N, 8 * N + 1, "cuda"))
    assert smiles_out.write_smiles(_decode(sets[0][0][:0], sets[0][1][:0], E), tables).cpu().strings() == []
    # decode and writer captured into one hipGraph, replayed on new logits: the eager results
    node, edge = (torch.from_numpy(4.0 * t).cuda() for t in dref.one_hot_logits(*sets[0], M, E))
    decoded = decode.MoleculeBatch.empty(B, N, N * (N - 1) // 2, False, "cuda")
    out = smiles_out.SmilesBatch.empty(B, N, 8 * N, "cuda")

    def chain():
        decode.decode_molecule_graphs(node, edge, out=decoded)
        smiles_out.write_smiles(decoded, tables, "whole", out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    seen = []
    for atoms, labels in sets[1:] + sets[:1]:
        n, e = dref.one_hot_logits(atoms, labels, M, E)
        node.copy_(torch.from_numpy(4.0 * n))
        edge.copy_(torch.from_numpy(4.0 * e))
        out.buffer.fill_(0xAA)
        graph.replay()
        got, = _finish(out)
        eager, = _finish(smiles_out.write_smiles(_decode(atoms, labels, E), tables, "whole"))
        assert np.array_equal(got.text, eager.text) and np.array_equal(got.length, eager.length)
        assert np.array_equal(got.order, eager.order) and np.array_equal(got.n_written, eager.n_written)
        ref.assert_batch_equals(got, ref.write_batch(_mols(atoms, labels), tables.atom_rows, tables.bond_rows, scope=ref.WHOLE))
        seen.append(got.strings())
    assert seen[0] != seen[1] and np.array_equal(got.text, fresh.text)


@pytest.mark.parametrize("graph", [False, True])
def test_sampler_writes_the_strings_of_its_batch(graph):
    """`MoleculeSampler(..., smiles=tables)`: the strings of the last sample equal `write_smiles` on its `MoleculeBatch`, and the
    batch itself is bit for bit the one a sampler without tables returns."""
    from druggen_amd import smiles_out, synth
    from druggen_amd.model import Generator
    from druggen_amd.sampling import MoleculeSampler
    N, E, Mn, B = 9, 5, 13, 4
    net = Generator("relu", N, E, Mn, 0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
    params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=11)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    net = net.cuda()
    decoder = {0: 0, 1: 6, 2: 7, 3: 8, 4: 9, 5: 15, 6: 16, 7: 17, 8: 35, 9: 53, 10: 34, 11: 14, 12: 5}
    tables = smiles_out.SmilesTables.from_decoders(decoder, ref.BOND_DECODER, "cuda")
    rng = np.random.default_rng(4)
    inputs = []
    for _ in range(2):
        atoms, labels = _family("relabelled", rng, B, N, E)
        node, edge = dref.one_hot_logits(atoms, labels + labels.transpose(0, 2, 1), Mn, E)
        inputs.append((torch.from_numpy(edge).cuda(), torch.from_numpy(node).cuda()))
    with pytest.raises(TypeError, match="SmilesTables"):
        MoleculeSampler(net, *inputs[0], graph=False, smiles=ref.BOND_DECODER)
    plain = MoleculeSampler(net, *inputs[0], graph=graph)
    writing = MoleculeSampler(net, *inputs[0], graph=graph, smiles=tables)
    assert plain.smiles is None
    for edge, node in inputs[::-1]:
        before, = _finish(plain.sample(edge, node))
        assert plain.smiles is None
        batch = writing.sample(edge, node)
        got, host = _finish(writing.smiles, batch)
        assert isinstance(writing.smiles, smiles_out.SmilesBatch)
        for name in ("atoms", "n_bonds", "component", "n_components", "largest", "largest_size"):
            assert np.array_equal(getattr(host, name), getattr(before, name)), name
        assert all(np.array_equal(host.edge_list(b), before.edge_list(b)) for b in range(B))      # (rows past n_bonds are unwritten)
        want, = _finish(smiles_out.write_smiles(batch, tables))
        for name in ("length", "n_written", "order", "text"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name
        assert got.strings() == want.strings() and all(s for s in got.strings())
        mols = [dict(atoms=host.atoms[b], bonds=host.edge_list(b), n_bonds=int(host.n_bonds[b]), component=host.component[b],
                     largest=int(host.largest[b])) for b in range(B)]
        ref.assert_batch_equals(got, ref.write_batch(mols, tables.atom_rows, tables.bond_rows))


def test_two_digit_numbers_and_the_two_overflows():
    """The constructions of the host test: twelve nested rings (%10, %11), 99 and 100 rings open at once, dense graphs at N = 45
    (-3), a str_cap that is exact and one a byte short (-4; the byte-wise write-out: str_cap is no multiple of 4)."""
    from druggen_amd import smiles_out
    tables = _tables()
    nested = cref.from_edges(24, [(i, i + 1) for i in range(23)] + [(i, 23 - i) for i in range(11)])
    got = _check(*_stack([nested, cref.cycle(24)]), 2, scope="whole", tables=tables)
    text = got.strings()[0]
    assert "%10" in text and "%11" in text and got.strings()[1] == "C1" + "C" * 22 + "C1"
    ref.parse_back(text, *nested, got.order[0].tolist())
    hubs = [cref.from_edges(102, [(i, i + 1) for i in range(101)] + [(0, i) for i in range(2, n)]) for n in (101, 102)]
    got = _check(*_stack(hubs), 2, scope="whole", tables=tables)
    assert "%99" in got.strings()[0] and got.length[1] == ref.RINGS and got.n_written.tolist() == [102, 102]
    rng = np.random.default_rng(45)
    atoms, labels = _family("dense", rng, 3, 45, 5)
    assert (_check(atoms, labels, 5, scope="whole", tables=tables).length == ref.RINGS).all()
    assert (_check(atoms, labels, 5, scope="whole", str_cap=3, tables=tables).length == ref.RINGS).all()      # -3 outranks -4
    atoms, labels = _family("relabelled", rng, 4, 17, 5)
    lengths = _check(atoms, labels, 5, scope="whole", tables=tables).length
    for str_cap in sorted({int(lengths.max()), int(lengths.max()) - 1, int(lengths.min()), int(lengths.min()) - 1, 1}):
        got = _check(atoms, labels, 5, scope="whole", str_cap=str_cap, tables=tables)
        assert ((got.length == ref.LONG) == (lengths > str_cap)).all() and not got.text[got.length < 0].any()
