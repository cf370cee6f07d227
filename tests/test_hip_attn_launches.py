"""Launch pin of the attention-block nodes (druggen_amd/functional/attention.py): for every path the nodes take -- fused and
unfused edge half, short and long core, with and without the edge output, first order, the gradient penalty's second order, the
LayerNorm-handle prologue, bf16 fused / unfused / composite fallback -- the launch count, the accounted HBM bytes and the accounted
flops per kernel id equal a recorded table exactly (tests/golden/attn_block_launches.json; its "parent" field names the commit it
was recorded on), and two runs in one process give bit-identical outputs and gradients."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B, C, HEADS = 2, 128, 8
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_block_launches.json")


def _cases():
    out = []
    for N in (5, 49, 97):
        for need_edge in (True, False):
            for kind in ("forward", "forward_backward", "penalty"):
                out.append(("f32", N, need_edge, kind))
    out.append(("f32", 5, True, "handle"))
    for N in (5, 49):
        for need_edge in (True, False):
            out.append(("bf16", N, need_edge, "forward_backward"))
    out.append(("bf16", 5, True, "create_graph"))
    return out


CASES = _cases()


def case_id(case) -> str:
    dtype, N, need_edge, kind = case
    return f"{dtype}-N{N}-{'edge' if need_edge else 'noedge'}-{kind}"


def _setup(case):
    """Modules and operands of one case, from a fixed seed: the same tensors every time it is called."""
    from druggen_amd.model.layers import MHA, MLP
    dtype, N, need_edge, kind = case
    adt = torch.float32 if dtype == "f32" else torch.bfloat16
    torch.manual_seed(11)
    attn, mlp = MHA(C, HEADS).cuda(), MLP(C, 3 * C, C).cuda()
    ln3, ln4, ln6 = (torch.nn.LayerNorm(C).cuda() for _ in range(3))
    with torch.no_grad():
        for ln in (ln3, ln4, ln6):
            ln.weight.add_(0.1 * torch.randn_like(ln.weight)); ln.bias.add_(0.1 * torch.randn_like(ln.bias))
    rn = lambda *s: torch.randn(*s, device="cuda")
    x1, y = rn(B, N, C).to(adt), (0.5 * rn(B, N, N, C)).to(adt)
    gouts = [rn(B, N, C).to(adt)] + ([rn(B, N, N, C).to(adt)] if need_edge else [])
    probes = [rn(B, N, C).to(adt), rn(B, N, N, C).to(adt)]
    params = list(attn.parameters()) + list(ln3.parameters()) + list(ln4.parameters())
    if kind == "handle":
        params += list(mlp.parameters()) + list(ln6.parameters())
    if kind == "forward":      # needs_input_grad follows requires_grad, not the grad mode: the parameters must not ask either
        for p in params:
            p.requires_grad_(False)
    return dict(attn=attn, mlp=mlp, ln3=ln3, ln4=ln4, ln6=ln6, x1=x1, y=y, gouts=gouts, probes=probes, params=params)


def _run_pass(case, s):
    """One pass of ``case`` over the operands ``s``; returns every output and gradient it produced (None for a parameter
    the pass does not reach)."""
    from druggen_amd import functional as dgf
    dtype, N, need_edge, kind = case
    attn, ln3, ln4 = s["attn"], s["ln3"], s["ln4"]
    pick = lambda x2, y2: (x2, y2) if need_edge else (x2,)
    if kind == "forward":      # no input requires a gradient (the Generator's forward inside the D step): nothing is kept
        with torch.no_grad():
            return list(pick(*dgf.attn_block(s["x1"], s["y"], attn, ln3, ln4, need_edge)))
    x1, y = s["x1"].clone().requires_grad_(True), s["y"].clone().requires_grad_(True)
    if kind == "forward_backward":
        outs = pick(*dgf.attn_block(x1, y, attn, ln3, ln4, need_edge))
        return list(outs) + list(torch.autograd.grad(outs, [x1, y] + s["params"], s["gouts"], allow_unused=True))
    if kind == "handle":       # y is the output of a feed-forward node's LayerNorm, whose handle comes along
        yl, handle = dgf.ffn_ln(y, *s["mlp"].ffn_ln_args(s["ln6"]), want_handle=True)
        assert handle is not None
        outs = pick(*dgf.attn_block(x1, yl, attn, ln3, ln4, need_edge, y_ln=handle))
        return list(outs) + list(torch.autograd.grad(outs, [x1, y] + s["params"], s["gouts"], allow_unused=True))
    if kind == "penalty":      # the gradient penalty's shape (model/loss.py): the first-order gradient is differentiated again
        with dgf.second_order_forward():
            outs = pick(*dgf.attn_block(x1, y, attn, ln3, ln4, need_edge))
        with dgf.inputs_only_backward():
            g1 = torch.autograd.grad(outs, [x1, y], s["gouts"], create_graph=True)
        scalar = sum((g.float() * t.float()).sum() for g, t in zip(g1, s["probes"]))
        return list(outs) + list(g1) + list(torch.autograd.grad(scalar, [x1, y] + s["params"], allow_unused=True))
    assert kind == "create_graph"      # outside second_order_forward(): the fused bf16 node falls back to the composite
    outs = pick(*dgf.attn_block(x1, y, attn, ln3, ln4, need_edge))
    g1 = torch.autograd.grad(outs, [x1, y], s["gouts"], create_graph=True)
    scalar = sum((g.float() ** 2).sum() for g in g1)
    return list(outs) + list(g1) + list(torch.autograd.grad(scalar, [attn.q.weight, attn.e.weight]))


def collect(case):
    """Run ``case`` once with the profiler on for every kernel id and the traffic counters cleared.  Returns
    ({kernel: [launches, bytes, flops]} for the kernels that ran, the pass's tensors)."""
    from druggen_amd import _lib
    from druggen_amd import functional as dgf
    from druggen_amd.options import options
    s = _setup(case)
    _lib.prof_enable(True)
    try:
        _lib.prof_reset()
        dgf.traffic_reset()
        with options.override(attn_half_f32_bwd="force"):      # (the fused float32 backward otherwise waits for B >= 128)
            tensors = _run_pass(case, s)
        torch.cuda.synchronize()
        table = {}
        for key in _lib.KERNEL_IDS:
            row = [_lib.prof_read(key)[0], int(dgf.traffic_bytes(key)), int(dgf.traffic_flops(key))]
            if any(row):
                table[key] = row
    finally:
        _lib.prof_enable(False)
    return table, [None if t is None else t.detach().clone() for t in tensors]


@pytest.fixture(scope="module")
def golden():
    with open(TABLE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_attn_block_launches_and_traffic_match_the_recorded_table(case, golden):
    want = golden["cases"][case_id(case)]
    first, a = collect(case)
    second, b = collect(case)
    assert first == want["kernels"]
    assert second == want["kernels"]
    assert len(a) == len(b)
    if want.get("bit_stable", True):
        for i, (t, u) in enumerate(zip(a, b)):
            assert (t is None) == (u is None), i
            assert t is None or torch.equal(t, u), i
