"""Host side of the wide node layers (csrc/node_wide.hip): their rows of the ctypes table and every argument check -- all of
which return before a launch.  No GPU.  tests/test_host.py holds the table against include/druggen_hip.h."""
import ctypes

import pytest

SHAPE, ARG, WORKSPACE = -1, -2, -3      # DG_E_SHAPE, DG_E_ARG, DG_E_WORKSPACE of include/druggen_hip.h
ENTRIES = {"dg_embed_node_wide_chain", "dg_embed_node_wide_bwd", "dg_embed_node_wide_wgrad_workspace_bytes",
           "dg_embed_node_wide_wgrad", "dg_wide_linear_fwd", "dg_wide_linear_dgrad", "dg_wide_linear_wgrad_workspace_bytes",
           "dg_wide_linear_wgrad"}


def test_wide_entries_take_the_narrow_parameter_lists():
    """The contracts the wide entries take over: same parameter lists as the narrow ones."""
    from druggen_amd import _lib
    assert ENTRIES <= set(_lib.SIGNATURES)
    for wide, narrow in (("dg_embed_node_wide_chain", "dg_embed_node_chain"), ("dg_embed_node_wide_bwd", "dg_embed_node_bwd"),
                         ("dg_wide_linear_fwd", "dg_skinny_linear_fwd"), ("dg_wide_linear_dgrad", "dg_skinny_linear_dgrad"),
                         ("dg_wide_linear_wgrad", "dg_skinny_linear_wgrad")):
        assert _lib.SIGNATURES[wide] == _lib.SIGNATURES[narrow]


@pytest.fixture(scope="module")
def lib():
    from druggen_amd import _lib
    return _lib.load()


_buf = (ctypes.c_int64 * 4)()
P = ctypes.addressof(_buf)      # a non-null pointer: no call below gets as far as reading it


def _err(lib):
    return lib.dg_last_error_string()


def test_chain_argument_checks(lib):
    def chain(in_=P, m1=None, m2=None, w1=P, w2=P, o1=P, o2=P, R=3, E=67, act=0):
        return lib.dg_embed_node_wide_chain(in_, m1, m2, w1, P, w2, P, o1, o2, R, E, act, None)
    for kw in (dict(in_=None), dict(w1=None), dict(w2=None), dict(o1=None), dict(o2=None)):
        assert chain(**kw) == ARG and b"dg_embed_node_wide_chain: null pointer" in _err(lib), kw
    assert chain(m1=P) == ARG and chain(m2=P) == ARG and b"given together" in _err(lib)
    for E in (0, 256, -1):
        assert chain(E=E) == SHAPE and b"1 <= E <= 255" in _err(lib), E
    assert chain(R=-1) == SHAPE
    for act in (4, -1):
        assert chain(act=act) == ARG and b"activation" in _err(lib)
    for act in (2, 3):
        assert chain(m1=P, m2=P, act=act) == ARG and b"second-order" in _err(lib)
        assert chain(act=act, R=0) == 0
    for E in (1, 16, 17, 255):
        for act in (0, 1):
            assert chain(R=0, E=E, act=act) == 0 and chain(R=0, E=E, act=act, m1=P, m2=P) == 0


def test_bwd_argument_checks(lib):
    def bwd(g=P, a1=P, a2=P, w1=P, w2=P, g2=P, g1=P, dz=P, R=3, E=67, act=0):
        return lib.dg_embed_node_wide_bwd(g, a1, a2, w1, w2, g2, g1, dz, R, E, act, None)
    for name in ("g", "a1", "a2", "w1", "w2", "g2", "g1"):
        assert bwd(**{name: None}) == ARG and b"dg_embed_node_wide_bwd: null pointer" in _err(lib), name
    for E in (0, 256):
        assert bwd(E=E) == SHAPE and b"1 <= E <= 255" in _err(lib)
    assert bwd(act=4) == ARG
    assert bwd(R=0) == 0 and bwd(R=0, dz=None, act=3, E=255) == 0      # dz is nullable


def test_node_wgrad_argument_checks(lib):
    need = lib.dg_embed_node_wide_wgrad_workspace_bytes(300, 67)
    assert need >= (64 * 67 + 64) * 4
    assert lib.dg_embed_node_wide_wgrad_workspace_bytes(300, 67) == need      # a function of (R, E) alone
    assert lib.dg_embed_node_wide_wgrad_workspace_bytes(300, 0) == 0 and lib.dg_embed_node_wide_wgrad_workspace_bytes(300, 256) == 0
    assert lib.dg_embed_node_wide_wgrad_workspace_bytes(0, 67) == 0

    def wgrad(g1=P, z=P, dw=P, db=P, ws=P, nbytes=need, R=300, E=67):
        return lib.dg_embed_node_wide_wgrad(g1, z, dw, db, ws, nbytes, R, E, None)
    for name in ("g1", "z", "dw", "ws"):
        assert wgrad(**{name: None}) == ARG and b"dg_embed_node_wide_wgrad: null pointer" in _err(lib), name
    for E in (0, 256):
        assert wgrad(E=E) == SHAPE
    assert wgrad(R=0) == SHAPE
    assert wgrad(nbytes=need - 1) == WORKSPACE and wgrad(nbytes=need - 1, db=None) == WORKSPACE
    assert b"workspace too small" in _err(lib)


def test_wide_linear_argument_checks(lib):
    def fwd(x=P, w=P, b=P, y=P, R=3, N=67, K=128, dtype=0):
        return lib.dg_wide_linear_fwd(x, w, b, y, R, N, K, dtype, None)

    def dgrad(dy=P, w=P, dx=P, R=3, N=67, K=128, dtype=0):
        return lib.dg_wide_linear_dgrad(dy, w, dx, R, N, K, dtype, None)
    need = lib.dg_wide_linear_wgrad_workspace_bytes(301, 67, 128)
    assert need >= (67 * 128 + 67) * 4

    def wgrad(dy=P, x=P, dw=P, db=P, ws=P, nbytes=need, R=301, N=67, K=128, dtype=0):
        return lib.dg_wide_linear_wgrad(dy, x, dw, db, ws, nbytes, R, N, K, dtype, None)
    for name in ("x", "w", "y"):
        assert fwd(**{name: None}) == ARG and b"dg_wide_linear_fwd: null pointer" in _err(lib), name
    for name in ("dy", "w", "dx"):
        assert dgrad(**{name: None}) == ARG and b"dg_wide_linear_dgrad: null pointer" in _err(lib), name
    for name in ("dy", "x", "dw", "ws"):
        assert wgrad(**{name: None}) == ARG and b"dg_wide_linear_wgrad: null pointer" in _err(lib), name
    for call in (fwd, dgrad, wgrad):
        for N in (16, 256, 0):
            assert call(N=N) == SHAPE and b"17 <= N <= 255" in _err(lib), (call.__name__, N)
        for K in (64, 127, 256):
            assert call(K=K) == SHAPE and b"K == 128" in _err(lib), (call.__name__, K)
        assert call(dtype=2) == ARG and b"unknown dtype" in _err(lib)
    for N in (17, 64, 255):
        for dtype in (0, 1):
            assert fwd(R=0, N=N, dtype=dtype) == 0 and fwd(R=0, N=N, b=None, dtype=dtype) == 0 and dgrad(R=0, N=N, dtype=dtype) == 0
    assert wgrad(R=0) == SHAPE
    assert wgrad(nbytes=need - 1) == WORKSPACE and b"workspace too small" in _err(lib)
    assert lib.dg_wide_linear_wgrad_workspace_bytes(301, 16, 128) == 0 and lib.dg_wide_linear_wgrad_workspace_bytes(301, 67, 64) == 0


def test_narrow_entries_keep_their_limits(lib):
    """The wide entries are additions: E = 17 and N = 17 are still refused where they were."""
    assert lib.dg_embed_node_chain(P, None, None, P, P, P, P, P, P, 3, 17, 0, None) == SHAPE and b"1 <= E <= 16" in _err(lib)
    assert lib.dg_embed_node_bwd(P, P, P, P, P, P, P, P, 3, 17, 0, None) == SHAPE
    assert lib.dg_skinny_linear_fwd(P, P, P, P, 3, 17, 128, 0, None) == SHAPE
    assert lib.dg_skinny_linear_dgrad(P, P, P, 3, 17, 128, 0, None) == SHAPE
