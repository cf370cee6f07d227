"""The attention-block nodes address their inputs, gradients and saved tensors by name (druggen_amd/functional/attention.py):
the declared name tuples are the nodes' signatures, ``_by_name`` puts a gradient where its input is.  No GPU needed."""
import inspect

import pytest

from druggen_amd.functional import attention as A

NODES = [("_AttnBlock", A._AttnBlock.forward, ("ctx",), A._ATTN_IN),
         ("_AttnBlockBwd", A._AttnBlockBwd._forward, ("ctx", "inb"), A._ATTN_BWD_IN),
         ("_AttnBlockFused", A._AttnBlockFused.forward, ("ctx",), A._ATTN_FUSED_IN)]


@pytest.mark.parametrize("node,fn,lead,names", NODES, ids=[n[0] for n in NODES])
def test_declared_input_names_are_the_forward_signature(node, fn, lead, names):
    params = tuple(inspect.signature(fn).parameters)
    assert params[:len(lead)] == lead
    assert params[len(lead):] == tuple(names)      # same names, same order, same count
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("node,fn,lead,names", NODES, ids=[n[0] for n in NODES])
def test_by_name_fills_one_slot_per_declared_input(node, fn, lead, names):
    assert A._by_name(names, {}) == (None,) * len(names)
    marks = {n: object() for n in names[::3]}
    out = A._by_name(names, marks)
    assert len(out) == len(names)
    for i, n in enumerate(names):
        assert out[i] is marks.get(n)
    with pytest.raises(KeyError):
        A._by_name(names, {"no_such_input": 1})
    with pytest.raises(KeyError):
        A._by_name(names, dict(marks, wq_=1))


def test_backward_outputs_and_saved_names_are_declared_inputs():
    # _AttnBlockBwd returns gradients of _AttnBlock's inputs; both nodes hand them on through _by_name
    assert set(A._ATTN_BWD_OUT) <= set(A._ATTN_IN)
    assert [n for n in A._ATTN_IN if n in A._ATTN_BWD_OUT] == list(A._ATTN_BWD_OUT)
    # what _AttnBlock saves (every tail) goes into _AttnBlockBwd by name
    assert set(A._attn_saved(True, True)) <= set(A._ATTN_BWD_IN)
    assert A._attn_saved(False, False) == A._ATTN_SAVED
    assert A._attn_saved(True, False) == A._ATTN_SAVED + A._ATTN_SAVED_EDGE
    assert A._attn_saved(False, True) == A._ATTN_SAVED + A._ATTN_SAVED_PREV
    assert set(A._ATTN_ADJOINTS) <= set(A._ATTN_BWD_IN)


def test_alias_outputs_are_forward_inputs_in_forward_order():
    assert len(A._ATTN_ALIASES) == 8 and len(set(A._ATTN_ALIASES)) == 8
    for names in (A._ATTN_IN, A._ATTN_FUSED_IN, A._ATTN_BWD_IN):
        assert [n for n in names if n in A._ATTN_ALIASES] == list(A._ATTN_ALIASES)
    # every output of the forward has a distinct name, with and without the edge output and the aliases
    for outs in (A._ATTN_OUT_EDGE, A._ATTN_OUT_NODE):
        assert len(set(outs + A._ATTN_ALIASES)) == len(outs) + 8
    assert [n for n in A._ATTN_OUT_EDGE if n in A._ATTN_OUT_NODE] == list(A._ATTN_OUT_NODE)
