"""GPU tests of the resident molecule set (`dg_mol_gather` through `druggen_amd.resident.ResidentMolecules`): a batch built by
index equals, bit for bit, what `load_molecules` makes of the collated batch of the same molecules, and what numpy makes of
the label matrices.  The outputs are exact 0 / 1 floats and integers: every comparison is `torch.equal`."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (n, B, N, M, E): the smallest shapes that hit a boundary -- N = 1 (no pair), E = 1, odd N N E with B >= 2 (misaligned
# molecule bases), E = 16 / M = 16 (the embedding kernels' limits), N = 97 (past the short attention kernels), N = 256
# (64 KiB of LDS, row / col = 255 in the top byte positions)
SHAPES = [(5, 4, 1, 1, 1), (7, 3, 3, 2, 5), (9, 4, 45, 13, 5), (6, 3, 64, 16, 16), (4, 2, 97, 4, 3), (3, 2, 256, 13, 5)]


@functools.lru_cache(maxsize=None)
def _molecules(n, N, M, E):
    """(bond labels [n, N, N] symmetric, density ~0.1, zero diagonal; atom labels [n, N]; graphs).  Molecule 0 has no bond,
    molecule 1 every off-diagonal entry (where E allows a bond at all)."""
    rng = np.random.default_rng([n, N, M, E])
    bonds = np.zeros((n, N, N), dtype=np.int64)
    if E > 1:
        upper = np.triu((rng.random((n, N, N)) < 0.1) * rng.integers(1, E, size=(n, N, N)), 1)
        bonds = upper + upper.transpose(0, 2, 1)
        bonds[0] = 0
        if n > 1:
            full = np.triu(rng.integers(1, E, size=(N, N)), 1)
            bonds[1] = full + full.T
    atoms = rng.integers(0, M, size=(n, N))
    graphs = []
    for i in range(n):
        x = np.zeros((N, M), dtype=np.float32)
        x[np.arange(N), atoms[i]] = 1.0
        src, dst = np.nonzero(bonds[i])
        graphs.append(SimpleNamespace(x=x, edge_index=np.stack([src, dst]).astype(np.int64), edge_attr=bonds[i][src, dst]))
    bonds.setflags(write=False)
    atoms.setflags(write=False)
    return bonds, atoms, tuple(graphs)


@functools.lru_cache(maxsize=None)
def _store(n, N, M, E):
    from druggen_amd.resident import ResidentMolecules
    store = ResidentMolecules.from_graphs(_molecules(n, N, M, E)[2], device="cuda", m_dim=M, b_dim=E)
    assert (len(store), store.vertexes, store.m_dim, store.b_dim) == (n, N, M, E)
    return store


def _index(n, B):
    return [(3 * k + 1) % n for k in range(B)]


def _loaded(graphs, idx, M, E):
    """The existing path: collate on the host, upload, dg_densify."""
    from druggen_amd import smiles as sm
    from druggen_amd.data import load_molecules
    return load_molecules(sm.collate([graphs[i] for i in idx]), b_dim=E, m_dim=M, device="cuda", batch_size=len(idx))


@pytest.mark.parametrize("n,B,N,M,E", SHAPES)
def test_batch_equals_load_molecules(n, B, N, M, E):
    from druggen_amd import functional as dgf
    store, graphs, idx = _store(n, N, M, E), _molecules(n, N, M, E)[2], _index(n, B)
    real, a, x = store.batch(torch.tensor(idx, device="cuda"))
    want_real, want_a, want_x = _loaded(graphs, idx, M, E)
    assert a.shape == (B, N, N, E) and x.shape == (B, N, M) and real.shape == (B, N * M + N * N * E)
    assert a.dtype == x.dtype == real.dtype == torch.float32
    assert torch.equal(a, want_a) and torch.equal(x, want_x) and torch.equal(real, want_real)
    lab, want_lab = dgf.one_hot_labels(a), dgf.one_hot_labels(want_a)
    assert lab is not None and want_lab is not None and lab.dtype == torch.int32 and torch.equal(lab, want_lab)
    store.raise_bad_indices(wait=True)


@pytest.mark.parametrize("n,B,N,M,E", [(9, 4, 45, 13, 5), (3, 2, 256, 13, 5)])
def test_batch_equals_numpy_one_hot(n, B, N, M, E):
    from druggen_amd import functional as dgf
    bonds, atoms, _ = _molecules(n, N, M, E)
    idx = _index(n, B)
    _, a, x = _store(n, N, M, E).batch(torch.tensor(idx, device="cuda"))
    assert np.array_equal(a.cpu().numpy(), np.eye(E, dtype=np.float32)[bonds[idx]])
    assert np.array_equal(x.cpu().numpy(), np.eye(M, dtype=np.float32)[atoms[idx]])
    assert np.array_equal(dgf.one_hot_labels(a).cpu().numpy(), bonds[idx].astype(np.int32))


def _buffers(B, N, M, E):
    return (torch.full((B, N, N, E), float("nan"), device="cuda"), torch.full((B, N, N), -1, dtype=torch.int32, device="cuda"),
            torch.full((B, N, M), float("nan"), device="cuda"))


@pytest.mark.parametrize("n,B,N,M,E", [(7, 3, 3, 2, 5), (9, 4, 45, 13, 5)])
def test_every_output_element_is_written(n, B, N, M, E):
    from druggen_amd import functional as dgf
    store, idx = _store(n, N, M, E), _index(n, B)
    a, labels, x = _buffers(B, N, M, E)
    real, a2, x2 = store.batch(torch.tensor(idx, device="cuda"), out=(a, labels, x))
    assert real is None and a2 is a and x2 is x and dgf.one_hot_labels(a) is labels
    assert not torch.isnan(a).any() and not torch.isnan(x).any() and int(labels.min()) >= 0
    _, want_a, want_x = store.batch(idx)
    assert torch.equal(a, want_a) and torch.equal(x, want_x) and torch.equal(labels, dgf.one_hot_labels(want_a))


def test_index_handling():
    from druggen_amd.resident import ResidentMolecules
    n, N, M, E = 9, 45, 13, 5
    bonds, atoms, graphs = _molecules(n, N, M, E)
    store = _store(n, N, M, E)

    def check(idx, got):
        _, a, x = got
        assert np.array_equal(a.cpu().numpy(), np.eye(E, dtype=np.float32)[bonds[idx]])
        assert np.array_equal(x.cpu().numpy(), np.eye(M, dtype=np.float32)[atoms[idx]])
    check([2, 2, 0], store.batch(torch.tensor([2, 2, 0], device="cuda")))                  # repeats
    perm = np.random.default_rng(3).permutation(n).tolist()
    check(perm, store.batch(torch.tensor(perm, device="cuda")))                            # all of them, shuffled
    check([8, 1], store.batch([8, 1]))                                                     # a CPU list
    check([4, 0, 4], store.batch(torch.tensor([4, 0, 4], dtype=torch.int32)))              # a CPU tensor of another integer type
    real, a, x = store.batch(torch.empty(0, dtype=torch.int64, device="cuda"))             # B = 0: no launch
    assert real.shape == (0, N * M + N * N * E) and a.shape == (0, N, N, E) and x.shape == (0, N, M)
    assert a.is_cuda and a.dtype == torch.float32
    one = ResidentMolecules.from_graphs(graphs[1:2], device="cuda", m_dim=M, b_dim=E)      # n = 1
    assert len(one) == 1 and one.nbytes() == N + 16 + 4 * N * (N - 1)
    _, a, x = one.batch([0, 0])
    assert np.array_equal(a.cpu().numpy(), np.eye(E, dtype=np.float32)[bonds[[1, 1]]])
    batches = list(store.epoch(4, generator=torch.Generator(device="cuda").manual_seed(1)))
    assert [tuple(b.shape) for b in batches] == [(4,), (4,)] and all(b.is_cuda and b.dtype == torch.int64 for b in batches)
    assert len(set(torch.cat(batches).tolist())) == 8
    assert torch.cat(list(store.epoch(4, shuffle=False, drop_last=False))).tolist() == list(range(n))
    store.raise_bad_indices(wait=True)
    with pytest.raises(ValueError, match="1-D"):
        store.batch(torch.zeros(2, 2, dtype=torch.int64, device="cuda"))


def test_bad_index_is_clamped_and_reported_later():
    n, N, M, E = 9, 45, 13, 5
    bonds, atoms, _ = _molecules(n, N, M, E)
    store = _store(n, N, M, E)      # atoms [n, N], ptr [n + 1], entries [nnz]: exactly sized
    assert store.atoms.shape == (n, N) and store.ptr.shape == (n + 1,) and store.entries.shape == (int((bonds != 0).sum()),)
    store.raise_bad_indices(wait=True)
    real, a, x = store.batch(torch.tensor([0, n, -1], device="cuda"))      # returns: n -> n - 1, -1 -> 0
    clamped = [0, n - 1, 0]
    assert np.array_equal(a.cpu().numpy(), np.eye(E, dtype=np.float32)[bonds[clamped]])
    assert np.array_equal(x.cpu().numpy(), np.eye(M, dtype=np.float32)[atoms[clamped]])
    assert torch.isfinite(real).all() and (a.sum(-1) == 1).all() and (x.sum(-1) == 1).all()
    with pytest.raises(RuntimeError, match=r"2 bad indices.*outside \[0, 9\)"):
        store.raise_bad_indices(wait=True)
    store.batch(torch.tensor([1, 2], device="cuda"))      # a clean call: nothing left to report
    store.raise_bad_indices(wait=True)


def test_batch_never_synchronises():
    n, N, M, E = 9, 45, 13, 5
    store = _store(n, N, M, E)
    idx = torch.tensor([5, 0, 7, 7], device="cuda")
    store.batch(idx)      # (warm: library loaded, the pinned slots and the side stream exist)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        real, a, x = store.batch(idx)
        store.raise_bad_indices()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, store.batch(idx)[1])
    store.raise_bad_indices(wait=True)


def test_generator_and_discriminator_take_the_batch():
    from druggen_amd import functional as dgf, synth
    from druggen_amd.model import Discriminator, Generator
    n, B, N, M, E = 9, 4, 9, 5, 5
    store, graphs, idx = _store(n, N, M, E), _molecules(n, N, M, E)[2], _index(n, B)
    _, a, x = store.batch(torch.tensor(idx, device="cuda"))
    _, want_a, want_x = _loaded(graphs, idx, M, E)
    assert dgf.one_hot_labels(a) is not None and dgf.one_hot_labels(want_a) is not None      # both take the table gather
    for cls, seed in ((Generator, 11), (Discriminator, 12)):
        net = cls("relu", N, E, M, 0.0, dim=128, depth=1, heads=8, mlp_ratio=3)
        params = synth.fill_parameters([(k, v.shape) for k, v in net.state_dict().items()], seed=seed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        net = net.cuda().eval()
        with torch.no_grad():
            got, want = net(a, x), net(want_a, want_x)
        got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))


def test_batch_is_capturable():
    from druggen_amd import functional as dgf
    n, B, N, M, E = 9, 4, 45, 13, 5
    store = _store(n, N, M, E)
    idx_static = torch.tensor([0, 1, 2, 3], device="cuda")
    bufs = _buffers(B, N, M, E)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        store.batch(idx_static, out=bufs)      # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        store.batch(idx_static, out=bufs)
    for content in ([8, 1, 1, 5], [3, 7, 0, 2]):
        idx_static.copy_(torch.tensor(content, device="cuda"))
        bufs[0].fill_(float("nan"))
        graph.replay()
        _, want_a, want_x = store.batch(torch.tensor(content, device="cuda"))
        assert torch.equal(bufs[0], want_a) and torch.equal(bufs[2], want_x)
        assert torch.equal(bufs[1], dgf.one_hot_labels(want_a))
    store.raise_bad_indices(wait=True)
    del graph


def test_out_buffers_are_validated_before_any_launch():
    n, B, N, M, E = 7, 3, 3, 2, 5
    store = _store(n, N, M, E)
    idx = torch.tensor(_index(n, B), device="cuda")
    good = _buffers(B, N, M, E)
    wrong = [
        (torch.empty(B, N, N, E + 1, device="cuda"), good[1], good[2]),                      # shape
        (good[0], torch.empty(B + 1, N, N, dtype=torch.int32, device="cuda"), good[2]),
        (good[0], good[1].long(), good[2]),                                                  # dtype
        (good[0], good[1], good[2].double()),
        (good[0].cpu(), good[1], good[2]),                                                   # device
        (torch.empty(B, N, E, N, device="cuda").transpose(2, 3), good[1], good[2]),          # not contiguous
        (good[0], good[1]),
    ]
    for out in wrong:
        with pytest.raises(ValueError, match="out"):
            store.batch(idx, out=out)
    assert torch.isnan(good[0]).all() and (good[1] == -1).all() and torch.isnan(good[2]).all()      # nothing was launched


def test_c_abi_errors_launch_nothing():
    from druggen_amd import _lib
    n, B, N, M, E = 7, 3, 3, 2, 5
    store = _store(n, N, M, E)
    lib = _lib.load()
    idx = torch.tensor(_index(n, B), device="cuda")
    a, labels, x = _buffers(B, N, M, E)
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")

    def call(N_=N, E_=E, a_ptr=a.data_ptr()):
        return lib.dg_mol_gather(store.atoms.data_ptr(), store.ptr.data_ptr(), store.entries.data_ptr(), n, idx.data_ptr(), B, N_,
                                 M, E_, a_ptr, labels.data_ptr(), x.data_ptr(), bad.data_ptr(), _lib.stream_of(a))
    assert call(N_=257) != 0 and b"1 <= N <= 256" in lib.dg_last_error_string()
    assert call(E_=17) != 0 and b"1 <= E <= 16" in lib.dg_last_error_string()
    assert call(a_ptr=None) != 0 and b"dg_mol_gather: null pointer" in lib.dg_last_error_string()
    torch.cuda.synchronize()
    assert torch.isnan(a).all() and (labels == -1).all() and torch.isnan(x).all() and int(bad) == 77
    assert call() == 0
    assert not torch.isnan(a).any() and int(bad) == 0
