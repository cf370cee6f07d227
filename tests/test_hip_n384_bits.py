"""Bit pins of the 128 -> 384 producer / consumer row GEMM (csrc/row_gemm_n384.hip) on its two hot instances: the forward of
fc1 writing the pre-split hidden tensor (DG_DTYPE_F32_H32: hi + lo fp16 planes, inverse row scales, ReLU bit words) and its
twin in the backward, dh = (dz W2) * m as one fp16 plane (DG_DTYPE_F32_H16, mask words taken from the forward launch).

A change of that kernel's SCHEDULE must not change one bit of what it writes: every output buffer of every case below is
hashed (SHA-256) and compared with tests/golden/n384_bits.json, recorded by scripts/record_n384_bits.py at the commit the
fixture names in its ``parent`` field.  Independently of the fixture every case is held against the float64 product at the
tolerances tests/test_hip_kernels.py uses for this kernel, a sentinel region behind every output must stay untouched, and a
second launch must give the same bytes."""
import hashlib
import json
import os

import pytest
import torch

from test_hip_kernels import TOL, _ffn_f32_masks, _gen, _rel

pytestmark = pytest.mark.gpu

C, H = 128, 384
FILL = 0xA5                      # every output buffer is filled with this byte before the launch
GUARD = 4096                     # bytes behind every output that no launch may touch
EDGE_R = 65536 + 33              # >= DG_EDGE_ROWS: the launch alternates its traversal direction; partial last stage
PAIR_RN, PAIR_RE = 180, 16200    # node rows riding in the launch over the edge rows (pair.h)
SINGLE_ROWS = [1, 31, 32, 33, 95, 97, 193, 8193]      # T mod 3 in {0, 1, 2} for the workgroups, partial last stages
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "n384_bits.json")
OUTPUTS = ("hi", "lo", "scale", "bits", "dh", "dh_scale")


def make_inputs(R, seed):
    """Inputs of one problem from the seeded CPU generator (the recipe of test_hip_kernels._ffn_f32_case), float64 on the CPU."""
    return dict(R=R, x=_gen((R, C), seed + 1), w1=_gen((H, C), seed + 2) * 0.1, b1=_gen((H,), seed + 3),
                w2=_gen((C, H), seed + 4) * 0.1, dz=_gen((R, C), seed + 8) * 1e-3)


class Problem:
    """Device operands and sentinel-filled output buffers of one forward + backward launch pair over R rows."""

    def __init__(self, inp):
        from druggen_amd import _lib as L, functional as dgf
        lib = L.load()
        self.R = R = inp["R"]
        f = lambda t: t.float().cuda().contiguous()
        self.x, self.w1, self.b1, self.w2, self.dz = (f(inp[k]) for k in ("x", "w1", "b1", "w2", "dz"))
        self.pw1, self.pw2 = dgf.packed_weight(self.w1, 0), dgf.packed_weight(self.w2, 1)
        self.off = int(lib.dg_hidden_scale_offset(R, H))
        self.h_bytes = int(lib.dg_hidden_bytes(R, H, L.F32_H32))
        self.dh_bytes = int(lib.dg_hidden_bytes(R, H, L.F32_H16))
        assert self.h_bytes == 2 * self.off + 4 * R and self.dh_bytes == self.off + 4 * R
        self.words = (R + 31) // 32 * 8 * 64          # [stages][8 waves][64 lanes]
        assert self.words <= int(lib.dg_row_gemm_mask_words(R, C, H, L.F32_H32))
        new = lambda n: torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.h, self.bits, self.dh = new(self.h_bytes), new(4 * self.words), new(self.dh_bytes)

    def forward(self):
        from druggen_amd import _lib as L
        L.launch("dg_row_gemm", self.x, L.fptr(self.x), self.pw1.data_ptr(), self.h.data_ptr(), self.R, C, H, L.fptr(self.b1), 1,
                 self.bits.data_ptr(), None, None, None, None, None, None, None, 0.0, L.F32_H32)

    def backward(self):
        from druggen_amd import _lib as L
        L.launch("dg_row_gemm", self.dz, L.fptr(self.dz), self.pw2.data_ptr(), self.dh.data_ptr(), self.R, C, H, None, 0,
                 None, self.bits.data_ptr(), None, None, None, None, None, None, 0.0, L.F32_H16)

    def regions(self):
        """name -> (buffer, start, stop) of every byte range a launch writes."""
        R, off = self.R, self.off
        return {"hi": (self.h, 0, R * H * 2), "lo": (self.h, off, off + R * H * 2), "scale": (self.h, 2 * off, 2 * off + 4 * R),
                "bits": (self.bits, 0, 4 * self.words), "dh": (self.dh, 0, R * H * 2), "dh_scale": (self.dh, off, off + 4 * R)}

    def outputs(self):
        """name -> bytes of every output (CPU), after checking that nothing outside those ranges was written."""
        torch.cuda.synchronize()
        reg = self.regions()
        out = {}
        for buf in (self.h, self.bits, self.dh):
            host = buf.cpu()
            untouched = torch.ones(host.numel(), dtype=torch.bool)
            for name, (b, lo, hi) in reg.items():
                if b is buf:
                    untouched[lo:hi] = False
                    out[name] = host[lo:hi]
            assert int(untouched.sum()) >= GUARD
            assert bool((host[untouched] == FILL).all()), "a launch wrote outside its output ranges"
        return out


def run_single(inp):
    p = Problem(inp)
    p.forward()
    p.backward()
    return p.outputs()


def run_both_directions(inp):
    """Two problems over the same edge-level inputs, issued forward, forward, backward, backward.  Every launch over at least
    DG_EDGE_ROWS rows flips the thread's traversal direction (csrc/traversal.h), so the two forward launches walk the stages in
    opposite directions, and so do the two backward launches (each against the mask words of its own forward)."""
    from druggen_amd import _lib as L
    prev = L.edge_rows()
    L.set_edge_rows(0)      # (a step run earlier in the process may have raised the threshold: DG_EDGE_ROWS for these launches)
    try:
        assert inp["R"] >= L.edge_rows()
        pa, pb = Problem(inp), Problem(inp)
        pa.forward()
        pb.forward()
        pa.backward()
        pb.backward()
        return pa.outputs(), pb.outputs()
    finally:
        L.set_edge_rows(prev)


def run_pair(node, edge):
    """Both problems inside one riding-launch region: node, edge, node, edge."""
    from druggen_amd import functional as dgf
    pn, pe = Problem(node), Problem(edge)
    with dgf._pair_launches(pe.x):
        pn.forward()
        pe.forward()
        pn.backward()
        pe.backward()
    return pn.outputs(), pe.outputs()


def digest(outs):
    return {k: hashlib.sha256(v.numpy().tobytes()).hexdigest() for k, v in outs.items()}


def check_float64(inp, outs):
    """The decoded outputs against the float64 product: h = relu(x W1^T + b1) is float32 class (TOL), its mask words the sign of
    the float64 pre-activations wherever those are not within 1e-6 of zero; dh = (dz W2) * m, GIVEN the forward's mask, within
    the 3.5e-4 of the two-product fp16-plane writer, and exactly zero where the mask is."""
    R = inp["R"]
    plane = lambda b: b.view(torch.float16).view(R, H).double()
    scale = lambda b: b.view(torch.float32).double()[:, None]
    v64 = inp["x"].float().double() @ inp["w1"].float().double().t() + inp["b1"].float().double()
    h = (plane(outs["hi"]) + plane(outs["lo"])) * scale(outs["scale"])
    assert bool(torch.isfinite(h).all())
    assert _rel(h, torch.relu(v64)) < TOL
    m = _ffn_f32_masks(outs["bits"].view(torch.int32), R)
    wrong = m != (v64 > 0)
    assert not wrong.any() or float((v64[wrong].abs() / v64.abs().max()).max()) < 1e-6
    assert bool((h[~m] == 0).all())
    dh = plane(outs["dh"]) * scale(outs["dh_scale"])
    dh64 = (inp["dz"].float().double() @ inp["w2"].float().double()) * m
    assert _rel(dh, dh64) < 3.5e-4
    assert bool((dh[~m] == 0).all())


_cache = {}


def case_outputs(name):
    """(inputs, first run, second run) of a case, computed once per session; a paired case returns lists of two."""
    if name not in _cache:
        if name == "pair":
            ins = [make_inputs(PAIR_RN, 3), make_inputs(PAIR_RE, 4)]
            _cache[name] = (ins, run_pair(*ins), run_pair(*ins))
        else:
            R = EDGE_R if name == "edge" else int(name[1:])
            inp = make_inputs(R, R % 11)
            _cache[name] = (inp, *run_both_directions(inp)) if name == "edge" else (inp, run_single(inp), run_single(inp))
    return _cache[name]


def case_names():
    return [f"R{R}" for R in SINGLE_ROWS] + ["edge", "pair"]


def record():
    """The fixture's ``cases`` table (scripts/record_n384_bits.py)."""
    table = {}
    for name in case_names():
        _, first, _ = case_outputs(name)
        if name == "pair":
            table[name] = {f"{who}.{k}": v for who, o in zip(("node", "edge"), first) for k, v in digest(o).items()}
        else:
            table[name] = digest(first)
    return table


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", [f"R{R}" for R in SINGLE_ROWS] + ["edge"])
def test_n384_hot_instances_bit_identical_to_the_recorded_parent(name):
    """Single launches: stage counts 1, 1, 1, 2, 3, 4, 7 and 257 (more stages than workgroups), and one launch over at least
    DG_EDGE_ROWS rows whose two runs walk the stages in opposite directions, for both instances (``run_both_directions``)."""
    inp, first, second = case_outputs(name)
    assert set(first) == set(OUTPUTS)
    assert digest(first) == digest(second)                  # a second launch; at the edge level: the other direction
    check_float64(inp, first)
    assert digest(first) == _golden()["cases"][name]


def test_n384_riding_launch_bit_identical_to_single_launches_and_parent():
    """Node rows riding in the launch over the edge rows equal the two single launches and the fixture, bit for bit."""
    ins, first, second = case_outputs("pair")
    want = _golden()["cases"]["pair"]
    for who, inp, a, b in zip(("node", "edge"), ins, first, second):
        single = run_single(inp)
        assert digest(a) == digest(b) == digest(single)
        check_float64(inp, a)
        assert {f"{who}.{k}": v for k, v in digest(a).items()} == {k: v for k, v in want.items() if k.startswith(who + ".")}
    assert len(want) == 2 * len(OUTPUTS)
