"""Argument checks of the sign-keeping edge-embedding entries (csrc/embed_sym_keep.hip): they answer before anything touches a
GPU, so they run everywhere."""
E_ARG = -2
SHAPE = (1, 9, 5, 64, 128)      # B, N, E, H, C
P = 4096                        # any non-NULL address: refused calls read nothing


def _lib():
    from druggen_amd import _lib
    return _lib.load()


def test_sign_words_are_six_per_edge_row():
    lib = _lib()
    assert lib.dg_embed_sym_sign_words(3, 8) == 3 * 8 * 8 * 6
    assert lib.dg_embed_sym_sign_words(256, 45) == 256 * 45 * 45 * 6
    assert lib.dg_embed_sym_sign_words(0, 45) == 0


def test_weight_gradients_come_together_or_not_at_all():
    lib = _lib()
    for k in range(4):
        dw = [P] * 4
        dw[k] = None
        assert lib.dg_embed_sym_bwd_keep(*[P] * 8, None, *dw, P, 1 << 30, *SHAPE, 0, 0, None) == E_ARG
        assert b"all given or all NULL" in lib.dg_last_error_string()
    for gw in ((P, None), (None, P)):
        assert lib.dg_embed_sym_bwd2_keep(*[P] * 10, *gw, P, 1 << 30, *SHAPE, 0, 0, None) == E_ARG
        assert b"both given or both NULL" in lib.dg_last_error_string()
    # nothing wanted: status 0 without a launch
    assert lib.dg_embed_sym_bwd_keep(*[P] * 8, None, None, None, None, None, None, 0, *SHAPE, 0, 0, None) == 0


def test_smooth_activations_and_null_signs_are_refused():
    lib = _lib()
    for act in (2, 3):
        assert lib.dg_embed_sym_fwd_keep(*[P] * 7, *SHAPE, act, 0, None) == E_ARG
        assert b"piecewise-linear" in lib.dg_last_error_string()
        assert lib.dg_embed_sym_bwd_keep(*[P] * 13, P, 1 << 30, *SHAPE, act, 0, None) == E_ARG
        assert b"piecewise-linear" in lib.dg_last_error_string()
        assert lib.dg_embed_sym_bwd2_keep(*[P] * 12, P, 1 << 30, *SHAPE, act, 0, None) == E_ARG
        assert b"piecewise-linear" in lib.dg_last_error_string()
    assert lib.dg_embed_sym_fwd_keep(*[P] * 6, None, *SHAPE, 0, 0, None) == E_ARG
    assert lib.dg_embed_sym_bwd_keep(*[P] * 7, None, *[P] * 5, P, 1 << 30, *SHAPE, 0, 0, None) == E_ARG
    assert lib.dg_embed_sym_bwd2_keep(*[P] * 8, None, *[P] * 3, P, 1 << 30, *SHAPE, 0, 0, None) == E_ARG
    assert b"null pointer" in lib.dg_last_error_string()


def test_entries_are_in_the_ctypes_table():
    """tests/test_host.py holds every row of the table against include/druggen_hip.h."""
    from druggen_amd import _lib
    assert {"dg_embed_sym_sign_words", "dg_embed_sym_fwd_keep", "dg_embed_sym_bwd_keep",
            "dg_embed_sym_bwd2_keep"} <= set(_lib.SIGNATURES)
