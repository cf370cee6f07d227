"""Input cases, the per-row metric and the launch helpers of tests/test_hip_attn_range.py and
tests/test_attn_range_cases_host.py: the attention kernels away from N(0,1) data -- saturated softmaxes, scores far below
zero, a single dominant neighbour in the last or the first slot, exact ties, molecules of very different magnitude --
and the same kernels under non-finite neighbours and with guarded output buffers.

Cases are built in float64 on the CPU from fixed seeds and rounded to the kernel's storage type; the rounded values are
what the references see.  Nothing here needs a GPU until a ``run_*`` helper is called."""
import torch

import kernel_math as km

ALPHA = 0.25
TOL = 2e-5           # float32 kernels against float64 (tests/test_hip_kernels.py)
BF16_IO = 4e-3       # a bf16-stored result against float64 on the same bf16 operands (tests/test_hip_bf16.py)
SENTINEL = -1.5e38   # guard fill (tests/test_hip_long_molecules.py)
C_HALF = 128         # the fused halves fix C

CORE_CASES = ["saturated", "far_negative", "max_last", "max_first", "ties", "molecule_scales"]
MOLECULE_SCALES = (1e-12, 1.0, 1e12)

# (N, C), B = 3: one shape per (LQS, JPL) instance of csrc/attn_core.hip's `Geometries` through pick_geometry():
#   (1,16) (7,12) -> (2,1);  (9,8) -> (1,1);  (33,8) -> (1,2);  (65,8) -> (1,3);  (17,16) -> (2,2);  (33,12) -> (2,3);
#   (49,16) -> (2,6);  (8,32) -> (3,1);  (9,32) -> (3,2);  (17,32) -> (3,3);  (48,128) -> (3,6);
#   (96,64) -> (3,12) in the forward and backward, (2,6) in the second order (narrow slices above 48 neighbours when
#   C / 4 is a multiple of 4);  (49,20) -> (3,12) in all three: C / 4 = 5 keeps the second order on its 12-slot instance
SHORT_SHAPES = [(1, 16), (7, 12), (9, 8), (33, 8), (65, 8), (17, 16), (33, 12), (49, 16), (8, 32), (9, 32), (17, 32),
                (48, 128), (96, 64), (49, 20)]
# csrc/attn_core_long.hip through long_geometry(), (forward | backward | second order):
#   (33,8)   -> (2,1) | (2,1) | (2,1);   (33,32)  -> (3,2) | (3,2) | (2,1);   (97,8)   -> (2,2) | (2,2) | (2,2)
#   (97,32)  -> (3,4) | (3,4) | (2,2);   (129,8)  -> (2,3) | (2,3) | (2,3);   (129,32) -> (3,6) | (2,3) | (2,3)
#   (193,32) -> (3,8) | (2,4) | (1,2);   (256,8)  -> (2,4) | (2,4) | (1,2)
# The two shapes at N = 33 are below what the modules route here (97..256): the entries take them, and they are the only
# way to LongFwd's (3,2) / (2,1) and LongBwd's (3,2).
LONG_SHAPES = [(33, 8), (33, 32), (97, 8), (97, 32), (129, 8), (129, 32), (193, 32), (256, 8)]

FIRST = ("s", "o", "dq", "dk", "dv", "de")
SECOND = ("gq", "gk", "gv", "ge", "gws", "gwo")


def gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def rounded(t, dtype):
    """float64 values that the storage type holds exactly."""
    return t.to(dtype).double()


def _scale_molecules(t, scales):
    return t * torch.tensor(scales, dtype=torch.float64).view(-1, *([1] * (t.dim() - 1)))


# ------------------------------------------------------------------------------------------------ core cases
def core_case(case, B, N, C, dtype=torch.float32):
    """-> dict of float64 CPU tensors q k v e ws wo tq tk tv te ae, every value representable in ``dtype``.
    ``ae`` is the outside adjoint of e that dg_attn_core_bwd_add / dg_attn_core_long_bwd add to de."""
    q, k, v = (gen((B, N, C), s) for s in (1, 2, 3))
    e = gen((B, N, N, C), 4, 0.8)
    ws, wo = gen((B, N, N, C), 5), gen((B, N, C), 6)
    t = [gen((B, N, C), 7), gen((B, N, C), 8), gen((B, N, C), 9), gen((B, N, N, C), 10)]
    ae = gen((B, N, N, C), 11, 0.5)
    if case == "normal":            # the data of the existing tests: the host test measures the cases against it
        pass
    elif case == "saturated":
        q, k, e = 6 * q, 6 * k, 2.5 * e
    elif case == "far_negative":
        q, k, e = q.abs() + 10, -(k.abs() + 10), 0.5 * e.abs() / 0.8 + 2
    elif case in ("max_last", "max_first"):
        q, k, e = q.abs() + 1, 0.1 * k.abs(), e.abs() / 0.8 + 0.5
        k[:, N - 1 if case == "max_last" else 0] = 30.0
    elif case == "ties":
        e = -(torch.arange(N) % 2).double().view(1, 1, N, 1).expand(B, N, N, C).clone()
        ws = torch.zeros_like(ws)
    elif case == "molecule_scales":
        assert B == len(MOLECULE_SCALES)
        v, wo = _scale_molecules(v, MOLECULE_SCALES), _scale_molecules(wo, MOLECULE_SCALES[::-1])
    else:
        raise ValueError(case)
    names = "q k v e ws wo tq tk tv te ae".split()
    return {n: rounded(x, dtype) for n, x in zip(names, [q, k, v, e, ws, wo] + t + [ae])}


def core_reference(ops, alpha=ALPHA, dtype=torch.float64, device=None, order=None):
    """tests/kernel_math.py on ``ops`` in ``dtype`` -> the twelve tensors of FIRST + SECOND plus ``de_add``.
    ``order``: a permutation of the neighbours j under which the sums run (the results come back in the original order):
    the same math, another summation order."""
    x = {n: t.to(device=device, dtype=dtype) for n, t in ops.items()}
    inv = None
    if order is not None:
        order = order.to(x["q"].device)
        inv = torch.argsort(order)
        for n in ("k", "v", "tk", "tv"):
            x[n] = x[n][:, order].contiguous()
        for n in ("e", "ws", "te", "ae"):
            x[n] = x[n][:, :, order].contiguous()
    a = [x[n] for n in "q k v e ws wo".split()]
    tt = [x[n] for n in "tq tk tv te".split()]
    s, o = km.attn_core_fwd(*a[:4], alpha)
    dq, dk, dv, de = km.attn_core_bwd(*a, alpha)
    h = km.attn_core_bwd2(*a, *tt, alpha)
    out = dict(zip(FIRST + SECOND, (s, o, dq, dk, dv, de) + tuple(h)))
    out["de_add"] = de + x["ae"]
    if inv is not None:
        for n in ("dk", "dv", "gk", "gv"):
            out[n] = out[n][:, inv]
        for n in ("s", "de", "de_add", "ge", "gws"):
            out[n] = out[n][:, :, inv]
    return out


def reference_orders(N):
    """The neighbour orders E_ref is measured over: as given, reversed, one fixed permutation."""
    return [None, torch.arange(N - 1, -1, -1), torch.randperm(N, generator=torch.Generator().manual_seed(N))]


def reference_error(ops, want, B, N, device=None):
    """E_ref per tensor: row_err of tests/kernel_math.py evaluated in float32 with torch on the same inputs, against the
    float64 evaluation ``want`` -- the worst of reference_orders(N), because the float32 error of one summation order is a
    matter of luck where a row has a dominant neighbour (tests/test_attn_range_cases_host.py)."""
    worst = {}
    for order in reference_orders(N):
        got = core_reference(ops, dtype=torch.float32, device=device, order=order)
        for name, w in want.items():
            worst[name] = max(worst.get(name, 0.0), row_err(got[name], w, B, N))
    return worst


def float32_bar(name, e_ref, factor=2.0):
    """first order: max(TOL, 2 E_ref); second order: max(5 TOL, 2 E_ref).  The factor 2 over a reference of the same
    precision is the project's convention (test_wgrad_running_column_scales_hold_fp32_accuracy_over_the_fp32_range)."""
    return max(5 * TOL if name in SECOND else TOL, factor * e_ref)


def scores(ops, alpha=ALPHA):
    """float64 s[b,i,j,c] of a core case."""
    e = ops["e"]
    return alpha * ops["q"].unsqueeze(2) * ops["k"].unsqueeze(1) * (e * e + e)


def naive_softmax_broken(s):
    """Fraction of the (b, i, c) softmaxes that a float32 exp(s) WITHOUT max subtraction cannot evaluate: the sum over j
    overflows, or every term underflows to zero."""
    p = torch.exp(s.float())
    l = p.sum(2)
    return float((~torch.isfinite(l) | (l == 0)).double().mean())


# ------------------------------------------------------------------------------------------------ the metric
def rel(got, want):
    """The whole-tensor relative L2 of the existing tests."""
    want = want.double().cpu()
    den = want.norm().item()
    return (got.double().cpu() - want).norm().item() / (den if den > 0 else 1.0)


def row_err(got, want, B, N):
    """max over rows r = (b, i) of |got_r - want_r| / max(|want_r|, rms_b), rms_b the rms row norm of molecule b in
    ``want``.  Tensors are [B, N, ...] in any flattening ([B,N,C], [B,N,N,C], [B N N, C], [B N N]): the row of dk / dv is
    (b, j), the row of an edge tensor is (b, i) over all j.  A row wrong by delta shows as delta whatever the other
    molecules hold; a non-finite result is an infinite error; where a whole molecule of ``want`` is zero the error is
    absolute."""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    w = want.double().reshape(B, N, -1)
    g = got.double().to(w.device).reshape(B, N, -1)
    wn = w.norm(dim=2)
    rms = wn.pow(2).mean(dim=1, keepdim=True).sqrt()
    den = torch.maximum(wn, rms)
    den = torch.where(den > 0, den, torch.ones_like(den))
    return float(((g - w).norm(dim=2) / den).max())


# ------------------------------------------------------------------------------------------------ launches
def _lib():
    from druggen_amd import _lib
    return _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(B, shape, dtype=torch.float32):
    """[Bpad, *shape] buffer filled with SENTINEL, Bpad = B rounded up to a multiple of 8 -- the molecules place() pads a
    grid with -- in ONE allocation: a launch gets the first B molecules, the rest is the guard."""
    return torch.full(((B + 7) // 8 * 8,) + tuple(shape), SENTINEL, dtype=dtype, device="cuda")


def guard_untouched(buf, B):
    return bool((buf[B:] == torch.tensor(SENTINEL, dtype=buf.dtype, device=buf.device)).all())


def all_written(buf, B):
    return not bool((buf[:B] == torch.tensor(SENTINEL, dtype=buf.dtype, device=buf.device)).any())


def to_gpu(ops, dtype):
    return {n: t.to(dtype).cuda().contiguous() for n, t in ops.items()}


def run_core(family, x, B, N, C, alpha=ALPHA):
    """Every entry of one core family (``short``: dg_attn_core_fwd / _bwd / _bwd_add / _bwd2, ``long``:
    dg_attn_core_long_fwd / _bwd with and without add_e / _bwd2) on the GPU tensors ``x`` (to_gpu(core_case(...))), each
    output in a guarded buffer.  -> dict name -> [Bpad, ...] tensor: FIRST + SECOND + de_add (+ dq_add, dk_add, dv_add,
    which must equal dq, dk, dv)."""
    L = _lib()
    lib = L.load()
    dtype = x["q"].dtype
    code = L.DTYPES[dtype]
    row, edge = (N, C), (N, N, C)
    G = lambda shape: guarded(B, shape, dtype)
    out = {n: G(edge if n in ("s", "de", "ge", "gws") else row) for n in FIRST + SECOND}
    out.update(de_add=G(edge), dq_add=G(row), dk_add=G(row), dv_add=G(row))
    p = {n: t.data_ptr() for n, t in x.items()}
    o = {n: t.data_ptr() for n, t in out.items()}
    st = _stream()
    if family == "short":
        L.check(lib.dg_attn_core_fwd(p["q"], p["k"], p["v"], p["e"], o["s"], o["o"], B, N, C, alpha, code, st), "fwd")
        L.check(lib.dg_attn_core_bwd(p["q"], p["k"], p["v"], p["e"], p["ws"], p["wo"], o["dq"], o["dk"], o["dv"], o["de"],
                                     B, N, C, alpha, code, st), "bwd")
        L.check(lib.dg_attn_core_bwd_add(p["q"], p["k"], p["v"], p["e"], p["ws"], p["wo"], p["ae"], o["dq_add"],
                                         o["dk_add"], o["dv_add"], o["de_add"], B, N, C, alpha, code, st), "bwd_add")
        L.check(lib.dg_attn_core_bwd2(p["q"], p["k"], p["v"], p["e"], p["ws"], p["wo"], p["tq"], p["tk"], p["tv"], p["te"],
                                      o["gq"], o["gk"], o["gv"], o["ge"], o["gws"], o["gwo"], B, N, C, alpha, code, st),
                "bwd2")
    else:
        need = int(lib.dg_attn_core_long_workspace_bytes(B, N, C))
        work = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
        L.check(lib.dg_attn_core_long_fwd(p["q"], p["k"], p["v"], p["e"], o["s"], o["o"], B, N, C, alpha, code, st), "fwd")
        L.check(lib.dg_attn_core_long_bwd(p["q"], p["k"], p["v"], p["e"], p["ws"], p["wo"], None, o["dq"], o["dk"],
                                          o["dv"], o["de"], work.data_ptr(), need, B, N, C, alpha, code, st), "bwd")
        L.check(lib.dg_attn_core_long_bwd(p["q"], p["k"], p["v"], p["e"], p["ws"], p["wo"], p["ae"], o["dq_add"],
                                          o["dk_add"], o["dv_add"], o["de_add"], work.data_ptr(), need, B, N, C, alpha,
                                          code, st), "bwd_add")
        L.check(lib.dg_attn_core_long_bwd2(p["q"], p["k"], p["v"], p["e"], p["ws"], p["wo"], p["tq"], p["tk"], p["tv"],
                                           p["te"], o["gq"], o["gk"], o["gv"], o["ge"], o["gws"], o["gwo"],
                                           work.data_ptr(), need, B, N, C, alpha, code, st), "bwd2")
    torch.cuda.synchronize()
    return out


def run_core_forward(family, x, B, N, C, alpha=ALPHA):
    """The forward alone -> (s, o)."""
    L = _lib()
    lib = L.load()
    s, o = torch.empty_like(x["e"]), torch.empty_like(x["q"])
    fn = lib.dg_attn_core_fwd if family == "short" else lib.dg_attn_core_long_fwd
    L.check(fn(x["q"].data_ptr(), x["k"].data_ptr(), x["v"].data_ptr(), x["e"].data_ptr(), s.data_ptr(), o.data_ptr(),
               B, N, C, alpha, L.DTYPES[x["q"].dtype], _stream()), "fwd")
    return s, o


# ------------------------------------------------------------------------------------------------ fused halves
HALF_CASES = ["saturated", "far_negative", "max_last", "max_first", "ties", "molecule_scales"]


def half_case(case, B, N, dtype=torch.float32):
    """Operands of the fused attention halves, float64 on the CPU, activations representable in ``dtype``:
    y q k v (activations), We be Woe boe g4 b4 (float32 parameters), d_o dz (upstream gradients of o and of the
    pre-LayerNorm sum).  e = y We^T + be is produced inside the kernels, so the score regimes come from the operands:
    saturated scales y, q, k; far_negative and ties take We = 0, so that e == be exactly (be = 2.5: gate 8.75; be in
    {0, -1} alternating over the channels: gate exactly 0); max_last / max_first take y, We >= 0 and be = 0.5, so that the
    gate is positive and the neighbour with k = 30 dominates every row."""
    C = C_HALF
    y = gen((B, N, N, C), 400)
    q, k, v = (gen((B, N, C), 401 + i) for i in range(3))
    We, Woe = gen((C, C), 404, 0.1), gen((C, C), 405, 0.1)
    be, boe = gen((C,), 406, 0.1), gen((C,), 407, 0.1)
    g4, b4 = gen((C,), 408, 0.1) + 1, gen((C,), 409, 0.1)
    d_o, dz = gen((B, N, C), 410), gen((B, N, N, C), 411)
    if case == "normal":            # the data of tests/test_hip_kernels.py
        pass
    elif case == "saturated":
        y, q, k = 2.5 * y, 6 * q, 6 * k
    elif case == "far_negative":
        We, be = torch.zeros_like(We), torch.full_like(be, 2.5)
        q, k = q.abs() + 10, -(k.abs() + 10)
    elif case in ("max_last", "max_first"):
        y, We, be = 0.5 * y.abs(), 0.3 * We.abs(), torch.full_like(be, 0.5)
        q, k = q.abs() + 1, 0.1 * k.abs()
        k[:, N - 1 if case == "max_last" else 0] = 30.0
    elif case == "ties":
        We, be = torch.zeros_like(We), -(torch.arange(C) % 2).double()
    elif case == "molecule_scales":
        v = _scale_molecules(v, MOLECULE_SCALES)
        d_o, dz = _scale_molecules(d_o, MOLECULE_SCALES[::-1]), _scale_molecules(dz, MOLECULE_SCALES[::-1])
    else:
        raise ValueError(case)
    act = dict(y=y, q=q, k=k, v=v, d_o=d_o, dz=dz)
    par = dict(We=We, be=be, Woe=Woe, boe=boe, g4=g4, b4=b4)
    out = {n: rounded(t, dtype) for n, t in act.items()}
    out.update({n: rounded(t, torch.float32) for n, t in par.items()})
    return out


def half_forward_reference(h, dtype=torch.float64, device=None, eps=1e-5, wdtype=None, round_s=None):
    """e = y We^T + be; s = alpha q_i k_j (e^2 + e); o = softmax_j(s) v; pre = y + s Woe^T + boe; y2 = LN(pre) g4 + b4,
    with plain torch ops in ``dtype``.  wdtype: the weights rounded to the MFMA operand type first; round_s: s rounded to
    that type where it enters out_e (the bf16 kernel's operand)."""
    x = {n: t.to(device=device, dtype=dtype) for n, t in h.items()}
    We, Woe = x["We"], x["Woe"]
    if wdtype is not None:
        We, Woe = We.to(wdtype).to(dtype), Woe.to(wdtype).to(dtype)
    e = x["y"] @ We.t() + x["be"]
    s, o = km.attn_core_fwd(x["q"], x["k"], x["v"], e, ALPHA)
    s_in = s if round_s is None else s.to(round_s).to(dtype)
    pre = x["y"] + s_in @ Woe.t() + x["boe"]
    y2, mean, rstd = km.ln_fwd(pre, x["g4"], x["b4"], eps)
    return dict(e=e, s=s, o=o, pre=pre, y2=y2, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1))


def run_half_f32_fwd(x, B, N, eps=1e-5):
    """dg_attn_half_f32_fwd on float32 GPU operands (to_gpu(half_case(...), torch.float32)), every output guarded."""
    from druggen_amd import functional as dgf
    L = _lib()
    lib = L.load()
    C = C_HALF
    pe, po = dgf.packed_weight(x["We"], 0), dgf.packed_weight(x["Woe"], 0)
    out = {n: guarded(B, (N, N, C)) for n in ("e", "s", "y2", "pre")}
    out.update(o=guarded(B, (N, C)), mean=guarded(B, (N, N)), rstd=guarded(B, (N, N)))
    L.check(lib.dg_attn_half_f32_fwd(x["y"].data_ptr(), x["q"].data_ptr(), x["k"].data_ptr(), x["v"].data_ptr(),
                                     pe.data_ptr(), x["be"].data_ptr(), po.data_ptr(), x["boe"].data_ptr(),
                                     x["g4"].data_ptr(), x["b4"].data_ptr(), out["e"].data_ptr(), out["s"].data_ptr(),
                                     out["o"].data_ptr(), out["y2"].data_ptr(), out["pre"].data_ptr(),
                                     out["mean"].data_ptr(), out["rstd"].data_ptr(), B, N, C, ALPHA, eps, _stream()),
            "dg_attn_half_f32_fwd")
    torch.cuda.synchronize()
    return out


BWD1_PER_MOLECULE = ("dz", "ds", "de", "dq", "dk", "dv")
BWD1_OVER_MOLECULES = ("dgamma", "dbeta")      # sums over every row of every molecule, by definition


def bwd1_case(case, B, N):
    """Operands of dg_attn_half_f32_bwd1: the core case (q k v e, wo as d_o) at C = 128 plus dy2, the pre-LayerNorm sum
    with its statistics, gamma4 and Woe.  ws of the core is ds = dz4 Woe here."""
    C = C_HALF
    c = core_case(case, B, N, C)
    R = B * N * N
    dy2 = gen((R, C), 500)
    pre = gen((R, C), 501, 2.0) + 0.3
    if case == "molecule_scales":
        dy2 = _scale_molecules(dy2.view(B, -1), MOLECULE_SCALES[::-1]).view(R, C)
    out = dict(q=c["q"], k=c["k"], v=c["v"], e=c["e"], d_o=c["wo"], dy2=dy2, pre=pre, Woe=gen((C, C), 507, 0.1),
               g4=gen((C,), 508, 0.1) + 1)
    out = {n: rounded(t, torch.float32) for n, t in out.items()}
    out["mean"] = rounded(out["pre"].mean(1), torch.float32)
    out["rstd"] = rounded((out["pre"].var(1, unbiased=False) + 1e-5).rsqrt(), torch.float32)
    return out


def bwd1_reference(h, B, N, dtype=torch.float64, device=None):
    """dz4 = LayerNormBackward(dy2; pre, mean, rstd, gamma4); ds = dz4 Woe; (dq, dk, dv, de) = the core's backward with
    ws = ds, wo = d_o (tests/kernel_math.py), in ``dtype``."""
    C = C_HALF
    x = {n: t.to(device=device, dtype=dtype) for n, t in h.items()}
    dz, dgamma, dbeta = km.ln_bwd(x["pre"], x["g4"], x["mean"].unsqueeze(1), x["rstd"].unsqueeze(1), x["dy2"])
    ds = dz @ x["Woe"]
    dq, dk, dv, de = km.attn_core_bwd(x["q"], x["k"], x["v"], x["e"], ds.view(B, N, N, C), x["d_o"], ALPHA)
    return dict(dz=dz, ds=ds, de=de, dq=dq, dk=dk, dv=dv, dgamma=dgamma, dbeta=dbeta)


def run_half_f32_bwd1(x, B, N):
    """dg_attn_half_f32_bwd1 (the instance that also writes ds), per-molecule outputs guarded."""
    from druggen_amd import functional as dgf
    L = _lib()
    lib = L.load()
    C = C_HALF
    pwo = dgf.packed_weight(x["Woe"], 1)
    ws = torch.empty(int(lib.dg_attn_half_f32_bwd1_workspace_bytes(B)), dtype=torch.uint8, device="cuda")
    out = {n: guarded(B, (N, N, C)) for n in ("dz", "ds", "de")}
    out.update({n: guarded(B, (N, C)) for n in ("dq", "dk", "dv")})
    dgb = torch.full((2, C), float("nan"), device="cuda")
    L.check(lib.dg_attn_half_f32_bwd1(x["dy2"].data_ptr(), x["pre"].data_ptr(), x["mean"].data_ptr(), x["rstd"].data_ptr(),
                                      x["g4"].data_ptr(), pwo.data_ptr(), x["e"].data_ptr(), x["q"].data_ptr(),
                                      x["k"].data_ptr(), x["v"].data_ptr(), x["d_o"].data_ptr(), out["dz"].data_ptr(),
                                      out["ds"].data_ptr(), out["de"].data_ptr(), out["dq"].data_ptr(), out["dk"].data_ptr(),
                                      out["dv"].data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(), ws.numel(),
                                      B, N, C, ALPHA, _stream()), "dg_attn_half_f32_bwd1")
    torch.cuda.synchronize()
    out.update(dgamma=dgb[0], dbeta=dgb[1])
    return out


HALF_BF16_PER_MOLECULE = ("dy", "dq", "dk", "dv")
HALF_BF16_OVER_MOLECULES = ("dwe", "dbe", "dwoe", "dboe")      # weight gradients: sums over every molecule


def half_bf16_reference(x):
    """float64 autograd on the operands the bf16 kernel sees -- tests/test_hip_attn_half.py::_reference, the one model of
    the kernel's bf16 operands (weights rounded to bf16, s rounded to bf16 where it enters out_e) -- on the GPU operands
    ``x`` of run_half_bf16."""
    import test_hip_attn_half as thh
    ref = thh._reference(x["y"], x["q"], x["k"], x["v"], x["We"], x["be"], x["Woe"], x["boe"], x["g4"], x["b4"],
                         torch.bfloat16, dz=x["dz"], dO=x["d_o"])
    return {n: t.detach() for n, t in ref.items()}


def run_half_bf16(x, B, N, eps=1e-5):
    """dg_attn_half_fwd and dg_attn_half_bwd on GPU operands (activations bf16, parameters float32), per-molecule outputs
    guarded (which is why the launches of tests/test_hip_attn_half.py, which allocate their own outputs, are not used;
    the weights are packed by its _pack)."""
    import test_hip_attn_half as thh
    L = _lib()
    lib = L.load()
    C, bf = C_HALF, torch.bfloat16
    code = L.DTYPES[bf]
    packed = thh._pack(x["We"], x["Woe"], bf)
    out = dict(o=guarded(B, (N, C), bf), y2=guarded(B, (N, N, C), bf), pre=guarded(B, (N, N, C), bf),
               mean=guarded(B, (N, N)), rstd=guarded(B, (N, N)), dy=guarded(B, (N, N, C), bf))
    out.update({n: guarded(B, (N, C), bf) for n in ("dq", "dk", "dv")})
    out.update(dwe=torch.zeros(C, C, device="cuda"), dwoe=torch.zeros(C, C, device="cuda"),
               dbe=torch.zeros(C, device="cuda"), dboe=torch.zeros(C, device="cuda"))
    P = lambda n: x[n].data_ptr()
    O = lambda n: out[n].data_ptr()
    L.check(lib.dg_attn_half_fwd(P("y"), P("q"), P("k"), P("v"), packed.data_ptr(), P("be"), P("boe"), P("g4"), P("b4"),
                                 O("o"), O("y2"), O("pre"), O("mean"), O("rstd"), B, N, C, ALPHA, eps, code, _stream()),
            "dg_attn_half_fwd")
    ws = torch.empty(int(lib.dg_attn_half_bwd_workspace_bytes(B, N)), dtype=torch.uint8, device="cuda")
    L.check(lib.dg_attn_half_bwd(P("y"), P("dz"), P("q"), P("k"), P("v"), P("d_o"), packed.data_ptr(), P("be"), O("dy"),
                                 O("dq"), O("dk"), O("dv"), O("dwe"), O("dbe"), O("dwoe"), O("dboe"), ws.data_ptr(),
                                 ws.numel(), B, N, C, ALPHA, code, _stream()), "dg_attn_half_bwd")
    torch.cuda.synchronize()
    return out


def half_to_gpu(h, dtype):
    """Activations in ``dtype``, parameters float32."""
    par = ("We", "be", "Woe", "boe", "g4", "b4")
    return {n: t.to(torch.float32 if n in par else dtype).cuda().contiguous() for n, t in h.items()}


def poison_molecule(x, b, value, names):
    """A copy of the GPU operands with every element of molecule ``b`` of the tensors ``names`` set to ``value``.  Row
    tensors [B N N, C] / [B N N] are addressed through their [B, ...] view."""
    out = dict(x)
    B = x["q"].shape[0]
    for n in names:
        t = x[n].clone()
        t.view(B, -1)[b] = value
        out[n] = t
    return out


def report(lines):
    """Print the measured figures of one test; with DG_ATTN_RANGE_TABLE=<file> also append them there
    (profiles/attn_range.txt is such a file)."""
    import os
    for ln in lines:
        print(ln)
    path = os.environ.get("DG_ATTN_RANGE_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
