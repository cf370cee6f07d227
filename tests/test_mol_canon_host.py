"""Host side of the canonical forms (csrc/mol_canon.hip, druggen_amd/canon.py): the scope codes against the header, every
argument refusal -- all of which return before a launch -- the host checks of canon.py, and the properties of the
plain-Python restatement (tests/mol_canon_ref.py) that the GPU tests lean on.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import decode_graph_ref as dref
import mol_canon_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -1, -2      # DG_E_SHAPE, DG_E_ARG of include/druggen_hip.h


def test_scope_codes_match_the_header():
    """(The two prototypes against their ctypes rows: tests/test_host.py, with every other entry.)"""
    from druggen_amd import canon
    text = open(os.path.join(ROOT, "include", "druggen_hip.h")).read()
    macro = {k: int(v) for k, v in re.findall(r"^#define\s+(DG_CANON_[A-Z]+)\s+(\d+)", text, flags=re.M)}
    assert canon.SCOPES == {"whole": macro["DG_CANON_WHOLE"], "largest": macro["DG_CANON_LARGEST"]}


@pytest.fixture(scope="module")
def lib():
    from druggen_amd import _lib
    return _lib.load()


_buf = (ctypes.c_int64 * 8)()
P = ctypes.addressof(_buf)      # a non-null, 8-byte aligned pointer: no call below gets as far as reading it
assert P % 8 == 0


def _err(lib):
    return lib.dg_last_error_string()


def test_canon_argument_checks(lib):
    """Every refusal of dg_mol_canon; none of these calls launches, and B == 0 returns 0 without one."""
    names = ("atoms", "bonds", "n_bonds", "component", "largest", "n_atoms", "n_bonds_in", "n_splits", "n_rounds", "order",
             "canon_atoms", "canon_bonds", "key")

    def call(B=3, N=9, cap=36, scope=1, **ptrs):
        p = {n: P for n in names}
        p.update(ptrs)
        return lib.dg_mol_canon(p["atoms"], p["bonds"], p["n_bonds"], p["component"], p["largest"], B, N, cap, scope,
                                p["n_atoms"], p["n_bonds_in"], p["n_splits"], p["n_rounds"], p["order"], p["canon_atoms"],
                                p["canon_bonds"], p["key"], None)
    for kw in (dict(B=-1), dict(N=0), dict(N=257), dict(N=-4), dict(N=1 << 20), dict(cap=-1)):
        assert call(**kw) == SHAPE and b"dg_mol_canon: need B >= 0, 1 <= N <= 256" in _err(lib), kw
    for scope in (-1, 2, 3, 256):
        assert call(scope=scope) == ARG and b"scope must be 0 (whole) or 1 (largest)" in _err(lib), scope
    for name in names:
        assert call(**{name: None}) == ARG and b"dg_mol_canon: null pointer" in _err(lib), name
    for name in ("bonds", "canon_bonds", "n_bonds", "largest", "n_atoms", "n_bonds_in", "n_splits", "n_rounds"):
        assert call(**{name: P + 2}) == ARG and b"aligned" in _err(lib), name
    assert call(key=P + 4) == ARG and b"aligned" in _err(lib)
    # the shape comes first, then the scope, then the pointers
    assert call(N=257, scope=5, atoms=None) == SHAPE and call(scope=5, atoms=None) == ARG and b"scope" in _err(lib)
    # an empty batch is no launch; without rows the bond pointers may be null, B == 0 still checks the rest
    assert call(B=0) == 0 and call(B=0, cap=0, bonds=None, canon_bonds=None) == 0
    assert call(B=0, N=256, cap=32640) == 0 and call(B=0, N=1, cap=0, scope=0) == 0
    assert call(B=0, scope=2) == ARG and call(B=0, key=None) == ARG


def test_match_argument_checks(lib):
    """Every refusal of dg_mol_canon_match (the last call of each group would launch, so it is never made with B > 0)."""
    batch = ("key", "n_atoms", "n_bonds_in", "n_splits", "canon_atoms", "canon_bonds")
    stock = ("stock_keys", "stock_index", "stock_n_atoms", "stock_n_bonds_in", "stock_n_splits", "stock_atoms", "stock_bonds")

    def call(B=3, N=9, cap=36, S=0, stock_cap=36, key_bits=64, **ptrs):
        p = {n: P for n in batch + stock + ("match", "tot")}
        p.update(ptrs)
        return lib.dg_mol_canon_match(*[p[n] for n in batch], B, N, cap, *[p[n] for n in stock], S, stock_cap, key_bits,
                                      p["match"], p["tot"], None)
    for kw in (dict(B=-1), dict(S=-1), dict(N=0), dict(N=257), dict(N=-1), dict(cap=-1), dict(stock_cap=-1)):
        assert call(**kw) == SHAPE and b"dg_mol_canon_match: need B >= 0" in _err(lib), kw
    for bits in (0, -1, 65, 128):
        assert call(key_bits=bits) == ARG and b"key_bits must be in 1..64" in _err(lib), bits
    for name in batch + ("match", "tot"):
        assert call(**{name: None}) == ARG and b"dg_mol_canon_match: null pointer" in _err(lib), name
    assert call(B=0, tot=None) == ARG      # an empty batch still writes tot
    for name in stock:
        assert call(S=4, **{name: None}) == ARG and b"null pointer (stock)" in _err(lib), name
    for name in ("key", "stock_keys", "tot"):
        assert call(S=4, **{name: P + 4}) == ARG and b"aligned" in _err(lib), name
    for name in ("n_atoms", "n_bonds_in", "n_splits", "canon_bonds", "match", "stock_index", "stock_n_atoms", "stock_n_bonds_in",
                 "stock_n_splits", "stock_bonds"):
        assert call(S=4, **{name: P + 2}) == ARG and b"aligned" in _err(lib), name
    # the shape comes first, then key_bits, then the pointers
    assert call(N=257, key_bits=0, key=None) == SHAPE and call(key_bits=0, key=None) == ARG and b"key_bits" in _err(lib)


def _host_batch(B=2, N=3, cap=3):
    from druggen_amd.decode import MoleculeBatch, _layout
    _, total = _layout(B, N, cap, False)
    return MoleculeBatch(np.zeros(total, dtype=np.uint8), B, N, cap, False)


def test_python_refusals_without_a_gpu():
    """canon.py refuses host batches, host forms, unknown scopes, bad key widths, a stock of another N and a stock sorted under
    another key width -- all before any launch."""
    from druggen_amd import canon
    host = _host_batch()
    for call in (canon.canonical_forms, canon.uniqueness_novelty):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(host)
        with pytest.raises(TypeError):
            call(np.zeros(4))
    _, total = canon._layout(2, 3, 3)
    forms = canon.CanonicalForms(np.zeros(total, dtype=np.uint8), 2, 3, 3, "largest")
    assert forms.is_host and forms.cpu() is forms and forms.key.dtype == np.int64 and forms.canon_bonds.shape == (2, 3, 4)
    assert forms.form(0) == (0, 0, (), ())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        canon.match_forms(forms)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        canon.CanonicalSet.from_forms(forms)
    with pytest.raises(TypeError):
        canon.match_forms(host)
    with pytest.raises(ValueError, match="scope"):
        canon._scope_code("fragment")
    for bad in (0, 65, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="key_bits"):
            canon._check_key_bits(bad)

    class Device:      # stands in for device forms: the checks below come before anything touches the buffer
        is_cuda, device = True, "cuda:0"

    def device_forms(N):
        f = canon.CanonicalForms(np.zeros(canon._layout(2, N, 3)[1], dtype=np.uint8), 2, N, 3, "largest")
        f.is_host, f.buffer = False, Device()
        return f
    mine = device_forms(3)
    with pytest.raises(ValueError, match="N = 4"):
        canon.match_forms(mine, canon.CanonicalSet(device_forms(4), None, None, 64))
    with pytest.raises(ValueError, match="sorted under key_bits = 8"):
        canon.match_forms(mine, canon.CanonicalSet(device_forms(3), None, None, 8))
    with pytest.raises(TypeError, match="CanonicalSet"):
        canon.match_forms(mine, stock=mine)
    with pytest.raises(ValueError, match="key_bits"):
        canon.match_forms(mine, key_bits=0)


def test_fractions_read_the_totals():
    from druggen_amd import canon
    tot = np.array([10, 6, 3, 5, 2, 4, 0, 0], dtype=np.int64)
    match = np.full((10, 2), -1, dtype=np.int32)
    m = canon.FormMatches(np.concatenate([tot.view(np.uint8), match.reshape(-1).view(np.uint8)]), 10)
    assert m.is_host and m.cpu() is m and m.total("n_distinct") == 6 and canon.TOT_FIELDS[4] == "n_truncated"
    assert m.unique_fraction == 6 / 8 and m.novel_fraction == 5 / 8 and m.unsplit_fraction == 4 / 8
    assert m.duplicate_of.tolist() == [-1] * 10 and m.stock_hit.shape == (10,)
    m.tot[:] = [10, 0, 0, 0, 10, 0, 0, 0]      # all truncated: nothing to divide by
    assert np.isnan(m.unique_fraction) and np.isnan(m.novel_fraction)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _form(atoms, labels, scope=ref.WHOLE):
    m = dref.decode_labels(atoms, labels)
    return ref.canon(m["atoms"], m["bonds"], m["component"], m["largest"], scope)


def test_all_graphs_on_five_vertices_fall_into_34_forms():
    pairs = [(i, j) for i in range(5) for j in range(i)]
    forms = {ref.form_of(_form(*ref.from_edges(5, [pairs[k] for k in range(10) if mask >> k & 1]))) for mask in range(1 << 10)}
    assert len(forms) == 34


def test_all_graphs_on_six_vertices_with_at_most_seven_edges_fall_into_78_forms():
    pairs = [(i, j) for i in range(6) for j in range(i)]
    forms = {ref.form_of(_form(*ref.from_edges(6, edges))) for k in range(8) for edges in itertools.combinations(pairs, k)}
    assert len(forms) == 78


def test_decalin_and_bicyclopentyl_differ_and_are_invariant():
    """Plain refinement colours them alike (three cells of 2, 4 and 4 atoms after the same rounds); the forms differ, and each
    is the same under 200 random renumberings."""
    rng = np.random.default_rng(2024)
    d, b = _form(*ref.decalin()), _form(*ref.bicyclopentyl())
    assert ref.form_of(d) != ref.form_of(b) and d["key"] != b["key"]
    assert (d["n_atoms"], d["n_bonds"]) == (b["n_atoms"], b["n_bonds"]) == (10, 11) and d["n_splits"] > 0 and b["n_splits"] > 0
    for graph, want in ((ref.decalin(), d), (ref.bicyclopentyl(), b)):
        for _ in range(200):
            got = _form(*ref.renumbered(rng, *graph))
            assert ref.form_of(got) == ref.form_of(want) and got["key"] == want["key"]


@pytest.mark.parametrize("n", [3, 6, 12])
def test_cycles_take_two_splits(n):
    f = _form(*ref.cycle(n))
    assert f["n_splits"] == 2 and (f["n_atoms"], f["n_bonds"]) == (n, n)


def test_molecule_like_family_is_invariant_under_renumbering():
    """Every graph of the fixed-seed family the GPU tests use, under 4 random renumberings each; the form read back through
    `order` is the input (soundness)."""
    rng = np.random.default_rng(7)
    worst = [0, 0]
    for N, closures, one_label in ref.MOLECULE_FAMILY:
        atoms, labels = ref.molecule_like(rng, N, closures, one_label)
        want = _form(atoms, labels)
        ref.check_order(atoms, labels, want["order"], want["canon_atoms"], want["canon_bonds"])
        worst = [max(worst[0], want["n_splits"]), max(worst[1], want["n_rounds"])]
        for _ in range(4):
            got = _form(*ref.renumbered(rng, atoms, labels))
            assert ref.form_of(got) == ref.form_of(want), (N, closures, one_label)
            assert (got["n_splits"], got["n_rounds"], got["key"]) == (want["n_splits"], want["n_rounds"], want["key"])
    assert worst[0] <= 8 and worst[1] <= 64, worst      # (a handful of splits: these are molecules, not regular graphs)


def test_scopes_fillers_and_matching_of_the_restatement():
    """Two components of equal size: 'largest' takes the one with the smaller root, 'whole' both; pads are dropped; matching
    points to the FIRST equal form and skips truncated molecules on both sides."""
    N = 8
    atoms = np.array([1, 2, 1, 2, 1, 2, 0, 0])
    labels = dref.two_equal_components(6)
    labels = np.pad(labels, ((0, 2), (0, 2)))
    m = dref.decode_labels(atoms, labels)
    largest = ref.canon(m["atoms"], m["bonds"], m["component"], m["largest"], ref.LARGEST)
    whole = ref.canon(m["atoms"], m["bonds"], m["component"], m["largest"], ref.WHOLE)
    assert (largest["n_atoms"], largest["n_bonds"], sorted(largest["order"])) == (3, 2, [0, 2, 4])
    assert (whole["n_atoms"], whole["n_bonds"], sorted(whole["order"])) == (6, 4, [0, 1, 2, 3, 4, 5])
    pads = dref.decode_labels(np.zeros(N, dtype=np.int64), np.zeros((N, N), dtype=np.int64))
    assert ref.canon(pads["atoms"], pads["bonds"], pads["component"], pads["largest"], ref.WHOLE)["n_atoms"] == 0
    assert ref.canon(pads["atoms"], pads["bonds"], pads["component"], pads["largest"], ref.LARGEST)["n_atoms"] == 1
    rng = np.random.default_rng(3)
    mols = [m, pads, dref.decode_labels(*ref.renumbered(rng, atoms, labels)), dref.decode_labels(*ref.cycle(N)), pads]
    forms = ref.canon_batch(mols, cap=5, scope=ref.WHOLE)      # the cycle has 8 bonds: truncated
    match, tot = ref.match(forms, stock=ref.canon_batch([mols[3], mols[2], mols[0]], cap=8, scope=ref.WHOLE))
    assert match.tolist() == [[-1, 1], [-1, -1], [0, 1], [-2, -2], [1, -1]]
    assert tot.tolist() == [5, 2, 2, 2, 1, 2, 0, 0]
    assert ref.match(forms)[0][:, 1].tolist() == [-3, -3, -3, -2, -3]
