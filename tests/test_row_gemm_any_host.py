"""Host side of the any-width row GEMM (csrc/row_gemm_any.hip): its rows of the ctypes table, the packed size and every argument
check -- all of which return before a launch.  No GPU.  tests/test_host.py holds the table against include/druggen_hip.h."""
import ctypes

import pytest

SHAPE, ARG = -1, -2      # DG_E_SHAPE, DG_E_ARG of include/druggen_hip.h
ENTRIES = {"dg_row_gemm_any_packed_bytes", "dg_row_gemm_any_pack", "dg_row_gemm_any"}


def test_entries_are_in_the_ctypes_table():
    from druggen_amd import _lib
    assert ENTRIES <= set(_lib.SIGNATURES)


@pytest.fixture(scope="module")
def lib():
    from druggen_amd import _lib
    return _lib.load()


_buf = (ctypes.c_int64 * 4)()
P = ctypes.addressof(_buf)      # a non-null pointer: no call below gets as far as reading it


def _err(lib):
    return lib.dg_last_error_string()


def test_packed_bytes(lib):
    size = lib.dg_row_gemm_any_packed_bytes
    for bad in (16, 48, 1056, 0, -32):
        assert size(bad, 64) == 0 and size(64, bad) == 0, bad
    assert size(32, 0) == 0
    for n_out, k in ((32, 32), (96, 160), (1024, 1024), (128, 384)):
        # hi + lo fp16 planes of the weight and one float32 scale per output channel
        assert size(n_out, k) >= n_out * k * 4 + n_out * 4, (n_out, k)


def test_pack_argument_checks(lib):
    def pack(w=P, packed=P, rows=64, cols=96, mode=0):
        return lib.dg_row_gemm_any_pack(w, packed, rows, cols, mode, None)
    for kw in (dict(w=None), dict(packed=None)):
        assert pack(**kw) == ARG and b"dg_row_gemm_any_pack: null pointer" in _err(lib), kw
    for mode in (-1, 2):
        assert pack(mode=mode) == ARG and b"dg_row_gemm_any_pack: mode" in _err(lib), mode
    for bad in (0, 16, 48, 1056, -32):
        for mode in (0, 1):
            assert pack(rows=bad, mode=mode) == SHAPE and b"dg_row_gemm_any_pack" in _err(lib), bad
            assert pack(cols=bad, mode=mode) == SHAPE and b"multiples of 32" in _err(lib), bad


def test_gemm_argument_checks(lib):
    def gemm(a=P, packed=P, bias=P, y=P, R=3, K=64, N=96):
        return lib.dg_row_gemm_any(a, packed, bias, y, R, K, N, None)
    for kw in (dict(a=None), dict(packed=None), dict(y=None)):
        assert gemm(**kw) == ARG and b"dg_row_gemm_any: null pointer" in _err(lib), kw
    assert gemm(R=-1) == SHAPE and b"dg_row_gemm_any: unsupported shape" in _err(lib)
    for bad in (0, 16, 48, 1056, -64):
        assert gemm(K=bad) == SHAPE and b"dg_row_gemm_any: unsupported shape" in _err(lib), bad
        assert gemm(N=bad) == SHAPE and b"multiples of 32" in _err(lib), bad
    # R == 0: nothing to do, no launch -- with and without a bias, at the corners of the shape range and at dg_row_gemm's shapes
    for K, N in ((32, 32), (1024, 1024), (96, 160), (128, 128), (128, 384), (384, 128)):
        assert gemm(R=0, K=K, N=N) == 0 and gemm(R=0, K=K, N=N, bias=None) == 0, (K, N)
    assert gemm(R=0, K=48) == SHAPE      # the shape is checked first


def test_python_route_terms():
    """``any_gemm_supported`` names what ``_mm_rows`` sends to the new kernel: never dg_row_gemm's three shapes, nothing with the
    switch off; ``row_gemm_supported`` keeps its meaning."""
    from druggen_amd import functional as dgf
    from druggen_amd.options import options
    assert dgf.any_gemm_supported(64, 192) and dgf.any_gemm_supported(32, 32) and dgf.any_gemm_supported(1024, 1024)
    for K, N in ((128, 128), (128, 384), (384, 128)):
        assert dgf.row_gemm_supported(K, N) and not dgf.any_gemm_supported(K, N)
    for K, N in ((64, 48), (16, 64), (64, 1056), (5, 64), (64, 1)):
        assert not dgf.any_gemm_supported(K, N) and not dgf.row_gemm_supported(K, N)
    assert not dgf.row_gemm_supported(64, 64)
    with options.override(row_gemm_any=False):
        assert not dgf.any_gemm_supported(64, 192)
    assert options.row_gemm_any is True and dgf.any_gemm_supported(64, 192)
