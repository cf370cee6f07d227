"""GPU tests of the circular fingerprint (`dg_mol_fingerprint` through `druggen_amd.fingerprint`) against the plain-Python
restatement of tests/mol_fp_ref.py.  Batches are built from label tensors as in tests/test_hip_mol_smiles.py (logits = 4 x
one-hot, the reference molecules from tests/decode_graph_ref.py, not from the GPU decode).  Every output is an integer: words,
counts and n_features are compared with `==`, bit for bit; there is no tolerance anywhere in this file."""
import csv
import os

import numpy as np
import pytest
import torch

import decode_graph_ref as dref
import mol_canon_ref as cref
import mol_fp_ref as ref
from test_hip_mol_canon import _finish, _mols, _stack, _store_graphs
from test_hip_mol_smiles import _decode, _family

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII_BITS = ((0, 32), (2, 1024), (4, 4096))      # every radius with a width of its own; the fixture test crosses them


def _tables(atom_decoder=ref.ATOM_DECODER, bond_decoder=ref.BOND_DECODER):
    from druggen_amd import fingerprint
    return fingerprint.FingerprintTables.from_decoders(atom_decoder, bond_decoder, "cuda")


def _host(fps):
    fps, = _finish(fps)
    return fps.words.numpy(), fps.counts.numpy(), fps.n_features.numpy()


def _check(atoms, labels, E, tables, cap=None, scopes=("largest",), grid=RADII_BITS, batch=None, **tab):
    """Kernel outputs of the batch against the restatement for every (radius, nbits) of `grid` under every scope.  The feature
    sets are computed once per radius and folded per width."""
    from druggen_amd import canon, fingerprint
    batch = batch if batch is not None else _decode(atoms, labels, E, cap)
    mols = _mols(atoms, labels)
    last = None
    for scope in scopes:
        sets = {}
        for radius, nbits in grid:
            if radius not in sets:
                sets[radius] = ref.feature_sets(mols, radius, cap, canon.SCOPES[scope], **tab)
            got = _host(fingerprint.circular_fingerprints(batch, tables, radius, nbits, scope))
            ref.assert_batch_equals(*got, [ref.folded(F, nbits) for F in sets[radius]])
            last = got
    return last


# ---- 1. the fixture molecules ---------------------------------------------------------------------------------------------------
def test_fixture_molecules_equal_the_restatement():
    """The eight molecules of tests/golden/chembl_like_smiles.csv under the decoders `smiles.build_encoders` gives them: radius
    0, 2, 4 crossed with 32, 1024 and 4096 bits, both scopes (the molecules are connected: the scopes agree)."""
    from druggen_amd import fingerprint, smiles
    with open(os.path.join(ROOT, "tests", "golden", "chembl_like_smiles.csv")) as f:
        strings = [r["SMILES"] for r in csv.DictReader(line for line in f if not line.startswith("#"))]
    assert len(strings) == 8
    atom_enc, atom_dec, bond_enc, bond_dec, kept, N = smiles.build_encoders(strings, 64)
    assert kept == strings and 30 <= N <= 64
    atoms, labels = np.zeros((8, N), dtype=np.int64), np.zeros((8, N, N), dtype=np.int64)
    for b, s in enumerate(strings):
        z, _, bonds = smiles.parse_smiles(s)
        atoms[b, :len(z)] = [atom_enc[a] for a in z]
        for i, j, t in bonds:
            labels[b, max(i, j), min(i, j)] = bond_enc[t]
    tables = _tables(atom_dec, bond_dec)
    atom_words, bond_rows = fingerprint.table_words(atom_dec, bond_dec)
    tab = dict(atom_words=atom_words.tolist(), bond_rows=[tuple(r) for r in bond_rows.tolist()])
    node, edge = dref.one_hot_logits(atoms, labels, len(atom_dec), len(bond_dec))
    from druggen_amd import decode
    batch = decode.decode_molecule_graphs(torch.from_numpy(4.0 * node).cuda(), torch.from_numpy(4.0 * edge).cuda())
    grid = [(r, nbits) for r in (0, 2, 4) for nbits in (32, 1024, 4096)]
    for scope in ("largest", "whole"):
        words, counts, n_features = _check(atoms, labels, None, tables, scopes=(scope,), grid=grid, batch=batch, **tab)
        assert (n_features > 40).all() and (counts > 30).all()      # radius 4, 4096 bits
    assert len({tuple(w) for w in words.tolist()}) == 8


# ---- 2. seeded sparse graphs at the word boundaries of the atom sets -----------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 9, 33, 64, 65, 96, 97, 255, 256])
def test_sparse_graphs_equal_the_restatement(N):
    """Molecule-like graphs with 0, 1, 2, 4 ring closures over six elements and four bond types, and two components, at every
    size at which a bit row gains a word (32 k, 32 k + 1), the short / long boundary (96, 97) and the maximum; both scopes
    where they differ; and a bond list one row short of the largest molecule (no graph)."""
    rng = np.random.default_rng([N, 327])
    tables = _tables()
    B = 4 if N <= 97 else 2
    atoms, labels = _family("relabelled", rng, B, N, 5)
    _check(atoms, labels, 5, tables, scopes=("largest", "whole") if N <= 65 else ("largest",))
    most = max(int(np.count_nonzero(l)) for l in labels)
    words, counts, n_features = _check(atoms, labels, 5, tables, cap=max(most - 1, 0), grid=((2, 1024),))
    if most > 0:
        cut = n_features == ref.NO_GRAPH
        assert cut.any() and not words[cut].any() and not counts[cut].any()
    if N <= 97:
        atoms, labels = _family("two components", rng, 3, N, 5)
        _check(atoms, labels, 5, tables, scopes=("largest", "whole"), grid=((2, 1024), (4, 4096)))


@pytest.mark.parametrize("name", ["one label", "cycles and a star", "no bonds", "all pad"])
def test_degenerate_families_equal_the_restatement(name):
    """Many equal ids and environments (one label everywhere; cycles; a star), and molecules without bonds: layer 0 only, one
    feature per distinct atom label under `whole`, the single atom of component 0 under `largest`, nothing for pads."""
    rng = np.random.default_rng(len(name))
    tables = _tables()
    for B, N in ((5, 9), (4, 45)):
        atoms, labels = _family(name, rng, B, N, 5)
        words, counts, n_features = _check(atoms, labels, 5, tables, scopes=("largest", "whole"))
        if name == "all pad":
            assert (n_features == 0).all() and not words.any()      # (the last scope is `whole`)
        if name == "no bonds":
            assert (n_features == 1).all() and (counts == 1).all()


# ---- 3. bond lists that exceed any LDS copy -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,bonds", [(40, 780), (64, 2016)])
def test_complete_graphs_equal_the_restatement(N, bonds):
    """Every pair bonded (the untrained generator's regime): the bond list is walked from global memory.  One molecule
    complete, one with a few pairs taken out, one dense at random."""
    rng = np.random.default_rng(N)
    full = dref.complete(N, 5)
    assert np.count_nonzero(full) == bonds
    holes = full.copy()
    for i, j in rng.integers(0, N, (12, 2)):
        holes[max(i, j), min(i, j)] = 0
    atoms = np.stack([rng.integers(0, 7, N), np.ones(N, dtype=np.int64), rng.integers(0, 7, N)])
    labels = np.stack([full, holes, np.tril(rng.integers(0, 5, (N, N)), -1)])
    tables = _tables()
    words, counts, n_features = _check(atoms, labels, 5, tables)
    assert (n_features > 0).all()
    _check(atoms, labels, 5, tables, scopes=("whole",), grid=((2, 1024),))


# ---- 4. truncated lists, flags, cap = 0 -------------------------------------------------------------------------------------------
def test_truncated_lists_flags_and_an_empty_bond_list():
    from druggen_amd import _lib, fingerprint
    rng = np.random.default_rng(4)
    tables = _tables()
    B, N, E = 6, 17, 5
    atoms, labels = _family("relabelled", rng, B, N, E)
    labels[2] = 0                                                  # a molecule without bonds: it has a graph at every cap
    counts = [int(np.count_nonzero(l)) for l in labels]
    for cap in (0, 1, sorted(counts)[3], max(counts)):
        for scope in ("largest", "whole"):
            words, _, n_features = _check(atoms, labels, E, tables, cap=cap, scopes=(scope,), grid=((2, 1024),))
            assert ((n_features == ref.NO_GRAPH) == (np.array(counts) > cap)).all() and n_features[2] > 0
    # flags: a negative value means no graph, whatever the list holds (the Python layer passes none: the entry itself)
    batch = _decode(atoms, labels, E)
    flags = torch.tensor([0, -2, 5, -1, 0, -2], dtype=torch.int32, device="cuda")
    out = fingerprint.CircularFingerprints.empty(B, 1024, "cuda")
    for t in (out.words, out.counts, out.n_features):
        t.fill_(0x5A5A5A5A)
    _lib.launch("dg_mol_fingerprint", batch.buffer, batch.atoms.data_ptr(), batch.bonds.data_ptr(), batch.n_bonds.data_ptr(),
                batch.component.data_ptr(), batch.largest.data_ptr(), flags.data_ptr(), tables.atoms.data_ptr(),
                tables.n_atom_labels, tables.bonds.data_ptr(), tables.n_bond_labels, B, N, batch.cap, 1, 2, 1024,
                out.words.data_ptr(), out.counts.data_ptr(), out.n_features.data_ptr())
    mols = _mols(atoms, labels)
    want = [ref.fingerprint(m["atoms"], m["bonds"], 2, 1024, flag=f, scope=ref.LARGEST, component=m["component"],
                            largest=m["largest"]) for m, f in zip(mols, flags.tolist())]
    ref.assert_batch_equals(*_host(out), want)
    assert [w["n_features"] == ref.NO_GRAPH for w in want] == [False, True, False, True, False, True]
    # an empty batch launches nothing
    empty = fingerprint.circular_fingerprints(_decode(atoms[:0], labels[:0], E), tables)
    assert len(empty) == 0 and empty.words.shape == (0, 32)


# ---- 5. every element is written, nothing outside ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [32, 1024, 4096])
def test_dirty_outputs_between_guards(nbits):
    """words, counts and n_features are views into one buffer filled with 0xA5 bytes, a guard of 64 words on both sides of
    each: after the call every element equals the restatement (molecules without a graph included) and every guard word still
    holds the fill."""
    from druggen_amd import fingerprint
    rng = np.random.default_rng(nbits)
    tables = _tables()
    B, N, E, G, W = 7, 33, 5, 64, nbits // 32
    atoms, labels = _family("relabelled", rng, B, N, E)
    most = max(int(np.count_nonzero(l)) for l in labels)
    batch = _decode(atoms, labels, E, most - 1)
    fill = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]
    buf = torch.full((G + B * W + G + B + G + B + G,), int(fill), dtype=torch.int32, device="cuda")
    at = [G, G + B * W + G, G + B * W + G + B + G]
    out = fingerprint.CircularFingerprints(buf[at[0]:at[0] + B * W].view(B, W), buf[at[1]:at[1] + B], nbits, buf[at[2]:at[2] + B])
    assert fingerprint.circular_fingerprints(batch, tables, 2, nbits, "whole", out=out) is out
    want = ref.fingerprint_batch(_mols(atoms, labels), 2, nbits, most - 1, ref.WHOLE)
    ref.assert_batch_equals(*_host(out), want)
    assert any(w["n_features"] == ref.NO_GRAPH for w in want) and any(w["n_features"] > 0 for w in want)
    host = buf.cpu().numpy()
    inside = np.zeros(len(host), dtype=bool)
    for start, size in zip(at, (B * W, B, B)):
        inside[start:start + size] = True
    assert (host[~inside] == fill).all() and (~inside).sum() == 4 * G
    with pytest.raises(ValueError, match="out="):
        fingerprint.circular_fingerprints(batch, tables, 2, nbits, out=fingerprint.CircularFingerprints.empty(B + 1, nbits, "cuda"))


# ---- 6. atom order ----------------------------------------------------------------------------------------------------------------
def test_a_permuted_batch_gives_identical_words():
    """Every molecule next to three copies with its atoms in a random order: identical words, counts and feature counts; and
    the restatement agrees with all of them."""
    rng = np.random.default_rng(6)
    tables = _tables()
    N, E, copies = 33, 5, 4
    base = [cref.molecule_like(rng, N, k % 4, k == 5) for k in range(6)]
    base += [(rng.integers(0, 7, N), np.tril(rng.integers(0, E, (N, N)) * (rng.random((N, N)) < 0.1), -1))]      # with fragments
    atoms, labels = _stack([cref.renumbered(rng, *g) if c else g for g in base for c in range(copies)])
    words, counts, n_features = _check(atoms, labels, E, tables, scopes=("whole",), grid=((3, 1024),))
    for k in range(len(base)):
        rows = slice(copies * k, copies * (k + 1))
        assert (words[rows] == words[copies * k]).all() and len(set(counts[rows])) == 1 and len(set(n_features[rows])) == 1
    assert len({tuple(words[copies * k]) for k in range(len(base))}) == len(base)


# ---- 7. end to end: similarities, stores ------------------------------------------------------------------------------------------
def test_similarities_from_kernel_fingerprints_equal_python_quotients():
    """`tanimoto_aggregate` of kernel fingerprints against the quotients float32(c) / float32(a + b - c) of the restatement's
    bit sets: the maximum and the smallest index that attains it; and the mean -- the float64 sum of S <= 12 float32
    quotients is exact in any order (each has 24 significant bits above 2^-37), so the mean is compared with `==` too."""
    from druggen_amd import fingerprint, metrics
    rng = np.random.default_rng(7)
    tables = _tables()
    N, E, S, G = 17, 5, 12, 7
    stock_g = [cref.molecule_like(rng, N, k % 3) for k in range(S)]
    gen_g = [cref.molecule_like(rng, N, k % 3) for k in range(G - 2)] + [stock_g[4], cref.renumbered(rng, *stock_g[9])]
    sides = []
    for graphs in (stock_g, gen_g):
        atoms, labels = _stack(graphs)
        fps = fingerprint.circular_fingerprints(_decode(atoms, labels, E), tables)
        sides.append((fps, [ref.bit_set(w) for w in ref.fingerprint_batch(_mols(atoms, labels))]))
    (stock, stock_bits), (gen, gen_bits) = sides
    assert isinstance(stock, metrics.PackedFingerprints)
    sim, idx = metrics.tanimoto_aggregate(stock, gen, "max", return_index=True)
    mean = metrics.tanimoto_aggregate(stock, gen, "mean")
    sim, idx, mean = sim.cpu().numpy(), idx.cpu().numpy(), mean.cpu().numpy()
    for g, bits in enumerate(gen_bits):
        q = np.array([ref.tanimoto(s, bits) for s in stock_bits], dtype=np.float32)
        assert sim[g] == np.float64(q.max()) and idx[g] == int(q.argmax()), g
        assert mean[g] == q.astype(np.float64).sum() / S, g
    assert sim[G - 2] == 1.0 and idx[G - 2] == 4 and sim[G - 1] == 1.0 and idx[G - 1] == 9 and (sim[:G - 2] < 1.0).all()
    snn = metrics.average_agg_tanimoto(stock, gen)
    assert snn == np.mean(sim)
    mean_div, std_div = metrics.internal_diversity(gen)
    rows = np.array([[ref.tanimoto(a, b) for a in gen_bits] for b in gen_bits], dtype=np.float32).astype(np.float64)
    assert mean_div == np.mean(1 - rows.sum(1) / G) and std_div == np.std(1 - rows.sum(1) / G)


def test_fingerprints_of_a_resident_store_in_uneven_chunks():
    """`fingerprint_store` equals the restatement and does not depend on the chunk (1, 7, n); a store against itself gives
    SNN 1.0 everywhere, with the smallest index among the molecules that have the same bits."""
    from druggen_amd import fingerprint, metrics
    from druggen_amd.resident import ResidentMolecules
    n, N, E = 11, 9, 5
    graphs, atoms, labels = _store_graphs(n, N, E, 1)
    graphs, atoms, labels = graphs + graphs[:3], np.concatenate([atoms, atoms[:3]]), np.concatenate([labels, labels[:3]])
    n += 3
    store = ResidentMolecules.from_graphs(graphs, device="cuda", m_dim=4, b_dim=E)
    tables = _tables()
    want = ref.fingerprint_batch(_mols(atoms, labels), 2, 1024)
    results = [fingerprint.fingerprint_store(store, tables, chunk=chunk) for chunk in (1, 7, n)]
    for fps in results:
        assert len(fps) == n and fps.nbits == 1024
        ref.assert_batch_equals(*_host(fps), want)
    other = fingerprint.fingerprint_store(store, tables, chunk=5, radius=3, nbits=64, scope="whole")
    ref.assert_batch_equals(*_host(other), ref.fingerprint_batch(_mols(atoms, labels), 3, 64, scope=ref.WHOLE))
    sim, idx = metrics.tanimoto_aggregate(results[0], results[0], "max", return_index=True)
    bits = [ref.bit_set(w) for w in want]
    assert (sim.cpu().numpy() == 1.0).all()
    assert idx.cpu().tolist() == [min(s for s in range(n) if bits[s] == bits[g]) for g in range(n)]
    assert idx.cpu().tolist()[-3:] == [0, 1, 2]
    with pytest.raises(ValueError, match="chunk"):
        fingerprint.fingerprint_store(store, tables, chunk=0)


# ---- 8. a captured graph ----------------------------------------------------------------------------------------------------------
def test_a_captured_graph_follows_its_static_inputs():
    """Decode and fingerprint captured into one hipGraph with `out=`: the capture allocates nothing, and replays on new logits
    give the eager results and the restatement's."""
    from druggen_amd import decode, fingerprint
    rng = np.random.default_rng(8)
    B, N, E, M = 5, 9, 5, 7
    tables = _tables()
    sets = [_family("relabelled", rng, B, N, E) for _ in range(3)]
    node, edge = (torch.from_numpy(4.0 * t).cuda() for t in dref.one_hot_logits(*sets[0], M, E))
    decoded = decode.MoleculeBatch.empty(B, N, N * (N - 1) // 2, False, "cuda")
    out = fingerprint.CircularFingerprints.empty(B, 1024, "cuda")

    def chain():
        decode.decode_molecule_graphs(node, edge, out=decoded)
        fingerprint.circular_fingerprints(decoded, tables, 2, 1024, "whole", out=out)
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
        for t in (out.words, out.counts, out.n_features):
            t.fill_(-1)
        graph.replay()
        got = _host(out)
        eager = _host(fingerprint.circular_fingerprints(_decode(atoms, labels, E), tables, 2, 1024, "whole"))
        assert all(np.array_equal(g, w) for g, w in zip(got, eager))
        ref.assert_batch_equals(*got, ref.fingerprint_batch(_mols(atoms, labels), 2, 1024, scope=ref.WHOLE))
        seen.append(got[0].tobytes())
    assert len(set(seen)) == 3
