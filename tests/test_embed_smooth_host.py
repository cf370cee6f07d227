"""Host-side checks of the smooth-activation work: the declaration of dg_embed_sym_bwd2_smooth and its ctypes row, its
argument checks (they answer before anything touches a GPU, so they run everywhere), the chain kernels' activation checks,
and the flat ``druggen_amd.functional`` namespace after the new autograd nodes."""
import ast
import importlib
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_ARG, E_WORKSPACE = -1, -2, -3
SHAPE = (1, 9, 5, 64, 128)      # B, N, E, H, C
P = 4096                        # any non-NULL address: refused calls read nothing


def _lib():
    from druggen_amd import _lib
    return _lib.load()


def test_header_declares_the_entry_and_the_ctypes_row_matches_it():
    """The entry is declared in include/druggen_hip.h, and its ctypes row is the parameter list written out here
    (tests/test_host.py holds every row against the header, parameter by parameter)."""
    import ctypes
    from druggen_amd import _lib
    main = open(os.path.join(ROOT, "include", "druggen_hip.h")).read()
    assert "dg_embed_sym_bwd2_smooth" in main
    assert _lib.SIGNATURES["dg_embed_sym_bwd2_smooth"] == (
        ctypes.c_int, [ctypes.c_void_p] * 15 + [ctypes.c_size_t] + [ctypes.c_int] * 7 + [ctypes.c_void_p])


def test_second_order_entry_argument_checks():
    lib = _lib()
    ok = [P] * 14 + [P, 1 << 30]
    for act in (0, 1):      # relu / leaky: dg_embed_sym_bwd2 is their entry
        assert lib.dg_embed_sym_bwd2_smooth(*ok, *SHAPE, act, 0, None) == E_ARG
        assert b"smooth activations only" in lib.dg_last_error_string()
    for k in range(10, 14):      # gw1, gb1, gw2, gb2 come together
        args = list(ok)
        args[k] = None
        assert lib.dg_embed_sym_bwd2_smooth(*args, *SHAPE, 3, 0, None) == E_ARG
        assert b"all given or all NULL" in lib.dg_last_error_string()
    for k in range(9):           # required operands and gg
        args = list(ok)
        args[k] = None
        assert lib.dg_embed_sym_bwd2_smooth(*args, *SHAPE, 3, 0, None) == E_ARG
        assert b"null pointer" in lib.dg_last_error_string()
    short = lib.dg_embed_sym_workspace_bytes(1, 9) - 1
    assert lib.dg_embed_sym_bwd2_smooth(*[P] * 14, P, short, *SHAPE, 2, 0, None) == E_WORKSPACE
    assert lib.dg_embed_sym_bwd2_smooth(*[P] * 14, None, 1 << 30, *SHAPE, 2, 0, None) == E_ARG      # weights without a workspace
    assert lib.dg_embed_sym_bwd2_smooth(*ok, 1, 9, 17, 64, 128, 3, 0, None) == E_SHAPE
    assert lib.dg_embed_sym_bwd2_smooth(*ok, *SHAPE, 3, 7, None) == E_ARG                               # dtype
    # the piecewise-linear entry keeps refusing the smooth activations
    assert lib.dg_embed_sym_bwd2(*[P] * 11, P, 1 << 30, *SHAPE, 3, 0, None) == E_ARG
    assert b"piecewise-linear" in lib.dg_last_error_string()


def test_chain_kernels_take_four_activations_unmasked_and_two_masked():
    lib = _lib()
    for act in (2, 3):
        assert lib.dg_embed_node_chain(P, P, P, P, None, P, None, P, P, 4, 5, act, None) == E_ARG
        assert b"second-order" in lib.dg_last_error_string()
        assert lib.dg_head_chain(P, P, P, P, P, None, P, None, P, None, P, P, P, P, 4, act, None) == E_ARG
        assert b"second-order" in lib.dg_last_error_string()
        # unmasked and first backward: accepted (R = 0 returns before a launch)
        assert lib.dg_embed_node_chain(P, None, None, P, P, P, P, P, P, 0, 5, act, None) == 0
        assert lib.dg_embed_node_bwd(P, P, P, P, P, P, P, P, 0, 5, act, None) == 0
        assert lib.dg_head_chain(P, None, None, None, P, P, P, P, P, P, P, P, P, P, 0, act, None) == 0
        assert lib.dg_head_bwd(P, P, P, P, P, P, P, P, P, P, 0, act, None) == 0
    for act in (-1, 4):
        assert lib.dg_embed_node_chain(P, None, None, P, P, P, P, P, P, 0, 5, act, None) == E_ARG
        assert lib.dg_head_bwd(P, P, P, P, P, P, P, P, P, P, 0, act, None) == E_ARG


def test_chain_support_follows_the_pass():
    """sigmoid / tanh: supported outside ``second_order_forward()``, not inside it (the answer needs no launch; CPU
    tensors are never supported)."""
    from druggen_amd.functional import heads
    assert heads._HEAD_ACTS == {"relu": 0, "leaky": 1, "sigmoid": 2, "tanh": 3}
    from druggen_amd import functional as dgf
    for act in ("sigmoid", "tanh"):
        assert heads._chain_act_ok(act)
        with dgf.second_order_forward():
            assert not heads._chain_act_ok(act) and heads._chain_act_ok("relu") and heads._chain_act_ok("leaky")
        assert heads._chain_act_ok(act)
    assert not heads._chain_act_ok("gelu") and not heads._chain_act_ok(None)


def test_recorded_functional_names_are_still_defined_once():
    """Every name test_flat_namespace_kept recorded is still defined by exactly one functional module and reachable from the
    flat namespace; the new nodes are there too."""
    import druggen_amd.functional as dgf
    recorded = open(os.path.join(ROOT, "tests", "golden", "functional_names.txt")).read().split()
    removed = {"_head_launch"}
    defined = {}
    for m in ("_runtime", "layernorm", "dense", "heads", "ffn", "attention", "embed"):
        module = importlib.import_module("druggen_amd.functional." + m)
        for node in ast.parse(open(module.__file__).read()).body:
            targets = []
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                targets = [node.name]
            elif isinstance(node, ast.Assign):
                targets = [e.id for t in node.targets for e in (t.elts if isinstance(t, ast.Tuple) else [t])
                           if isinstance(e, ast.Name)]
            for t in targets:
                assert defined.setdefault(t, module) is module, f"{t} is defined in two modules"
    for name in recorded:
        if name not in removed:
            assert name in defined and getattr(dgf, name) is getattr(defined[name], name), name
    for name in ("_EmbedSymBwdSmooth", "_composite_node_embed", "_composite_head_tail", "_chain_act_ok"):
        assert name in defined and hasattr(dgf, name), name
    assert defined["_EmbedSymBwdSmooth"].__name__.endswith(".embed")
