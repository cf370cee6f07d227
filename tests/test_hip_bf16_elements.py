"""The dense kernels of the bf16 configuration, element by element (cases, float64 references and bars: tests/bf16_cases.py,
checked on the CPU by tests/test_bf16_cases_host.py): dg_row_gemm (bf16), the bf16 instance of dg_linear_wgrad,
dg_skinny_linear_wgrad, dg_ffn_ln_fwd_bf16 / dg_ffn_ln_bwd_bf16, dg_attn_half_fwd / _bwd, dg_embed_sym_bwd_bf16, through the C ABI so that every output lives inside a buffer of
payload NaNs and every row operand is followed by NaN rows.

  * exact cases: integer data on which a correct kernel gives the float64 result bit for bit, at R = 1 .. 129 around the
    64-row tile and at one R past the persistent grid (a workgroup's second round, with the tail tile in it);
  * bounded cases: N(0,1) and scaled data against the derived single-product bar; the chained outputs of the fused
    feed-forward against the float32 restatement's own error;
  * planted rows: weight gradients whose upstream gradient is zero outside at most 8 named rows;
  * guards, non-finite rows, run-to-run and graph-replay reproducibility, refusal of misaligned pointers.

Run with -s for the figures (profiles/bf16_element_bars.txt)."""
import pytest
import torch

import bf16_cases as bc

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PAD = 128          # guard rows (elements of a vector) on each side of an output, NaN rows behind an input
PAST = "past"      # a row count past the persistent grid: workgroups x 64 + 65


def _L():
    from druggen_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(status, what):
    _L().check(status, what)


# ---------------------------------------------------------------------------------------------- grids
def _row_gemm_grid(K, N):
    """Workgroups of a dg_row_gemm (bf16) launch with more tiles than workgroups: csrc/gemm_bf16.hip fixes its grid at 256
    compute units (the MI355X) times the workgroups per unit of the instance -- two for 128 -> 128, one for the 384-wide
    ones.  The library has no query for it; a device with more units only moves the test's R, not what it asserts."""
    cus = max(256, torch.cuda.get_device_properties(0).multi_processor_count)
    return cus * (2 if (K, N) == (128, 128) else 1)


def _ffn_grid():
    """Workgroups of the fused feed-forward kernels at a large R, from the library's own workspace query (one partial-sum
    block of 128 x 384 + 384 + 3 x 128 floats per workgroup)."""
    lib = _L().load()
    return int(lib.dg_ffn_bf16_workspace_bytes(1 << 24)) // ((128 * 384 + 384 + 3 * 128) * 4)


def _rows(R, grid):
    return grid * 64 + 65 if R == PAST else R


# ---------------------------------------------------------------------------------------------- guarded buffers
def _sentinel(n, dtype):
    """Payload NaNs (an int pattern for bit-mask words): a guard that is read shows as well as one that is written."""
    if dtype == BF:
        return torch.full((n,), 0x7FA5, dtype=torch.int16)
    if dtype == F32:
        return (0x7FC00000 + torch.arange(n, dtype=torch.int64) % 4096).to(torch.int32)
    return torch.full((n,), 0x5A5A5A5A, dtype=torch.int32)


class Guarded:
    """An output of ``rows`` x ``cols`` inside an allocation of ``alloc`` rows (the rows the kernel may write) with PAD
    rows of sentinels on both sides; everything starts as sentinels."""

    def __init__(self, rows, cols, dtype, alloc=None, vector=False):
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.alloc = rows if alloc is None else alloc
        n = (2 * PAD + self.alloc) * cols
        self.sent = _sentinel(n, dtype)
        self.raw = self.sent.cuda()
        whole = self.raw if dtype == torch.int32 else self.raw.view(dtype)
        self.t = whole[PAD * cols:(PAD + rows) * cols]
        self.t = self.t if vector else self.t.view(rows, cols)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, written=True, what=""):
        raw = self.raw.cpu()
        lo, hi, end = PAD * self.cols, (PAD + self.rows) * self.cols, (PAD + self.alloc) * self.cols
        assert torch.equal(raw[:lo], self.sent[:lo]), f"{what}: written in front of the output"
        assert torch.equal(raw[end:], self.sent[end:]), f"{what}: written behind the rows the kernel may write"
        if written and self.dtype != torch.int32:
            assert not bool((raw[lo:hi] == self.sent[lo:hi]).any()), f"{what}: an element of rows [0, R) was not written"
        return self

    def cpu(self):
        return self.t.detach().cpu()


def _rows_in(t, dtype=BF, pad="nan"):
    """``t`` [R, C] on the device as ``dtype``, followed by PAD rows of NaN (or zeros)."""
    R, C = t.shape
    whole = torch.full((R + PAD, C), float("nan") if pad == "nan" else 0.0, dtype=dtype)
    whole[:R] = t.to(dtype)
    return whole.cuda()[:R]


def _vec(t):
    return t.to(F32).cuda().contiguous()


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = torch.int16 if a.dtype == BF else torch.int32
    return bool(torch.equal(a.view(it), b.view(it)))


# ---------------------------------------------------------------------------------------------- dg_row_gemm (bf16)
def _packed(w_prime, mode):
    """The packed operand of y = a W'^T: the forward pack of W' (mode 0) or the input-gradient pack of W'^T (mode 1)."""
    from druggen_amd import functional as dgf
    w = w_prime.to(F32) if mode == 0 else w_prime.to(F32).t().contiguous()
    w = w.cuda()
    return dgf.packed_weight(w, mode, BF), w        # (the parameter keeps its pack alive in the cache)


def _row_gemm(a, packed, R, K, N, bias=None, relu=False, want_bits=False, mask_bits=None, residual=None, ln=None, want_pre=False,
              check=True):
    lib = _L().load()
    out = dict(y=Guarded(R, N, BF))
    if want_bits:
        out["bits"] = Guarded(int(lib.dg_row_gemm_mask_words(R, K, N, 1)), 1, torch.int32, vector=True)
    gamma = beta = None
    if ln is not None:
        gamma, beta = ln
        out["mean"], out["rstd"] = Guarded(R, 1, F32, vector=True), Guarded(R, 1, F32, vector=True)
        if want_pre:
            out["pre"] = Guarded(R, N, BF)
    p = lambda k: out[k].ptr() if k in out else None
    d = lambda t: None if t is None else t.data_ptr()
    _ok(lib.dg_row_gemm(a.data_ptr(), packed.data_ptr(), p("y"), R, K, N, d(bias), 1 if relu else 0, p("bits"), d(mask_bits),
                        d(residual), d(gamma), d(beta), p("mean"), p("rstd"), p("pre"), bc.EPS, 1, _stream()), "dg_row_gemm")
    torch.cuda.synchronize()
    if check:
        for k, g in out.items():
            g.check(what=f"dg_row_gemm {k} R={R} K={K} N={N}")
    return out


def _exact(got, want, what):
    got = got.double().cpu() if got.is_cuda else got.double()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


@pytest.mark.parametrize("K,N", bc.GEMM_SHAPES)
@pytest.mark.parametrize("R", bc.ROW_COUNTS + (PAST,))
def test_row_gemm_exact_cases_bit_for_bit(R, K, N):
    """Integer operands (exact by construction): every epilogue of dg_row_gemm (bf16) equals float64, element by element, for
    the forward and the input-gradient pack; NaN rows behind a / residual and NaN guards round every output."""
    R = _rows(R, _row_gemm_grid(K, N))
    c = bc.gemm_exact_case(R, K, N)
    a, a2, res = _rows_in(c["a"]), _rows_in(c["a2"]), _rows_in(c["residual"])
    bias = _vec(c["bias"])
    tag = f"R={R} K={K} N={N}"
    for mode in (0, 1):
        pk, _keep = _packed(c["w"], mode)
        tag = f"pack mode {mode}, R={R} K={K} N={N}"
        _exact(_row_gemm(a, pk, R, K, N)["y"].t, bc.gemm_chain(c["a"], c["w"])[0], f"plain, {tag}")
        _exact(_row_gemm(a, pk, R, K, N, bias=bias)["y"].t, bc.gemm_chain(c["a"], c["w"], c["bias"])[0], f"bias, {tag}")
        want, z = bc.gemm_chain(c["a"], c["w"], c["bias"], relu=True)
        out = _row_gemm(a, pk, R, K, N, bias=bias, relu=True, want_bits=True)
        _exact(out["y"].t, want, f"bias + ReLU, {tag}")
        pk2, _keep2 = _packed(c["w2"], 1 - mode)
        masked = _row_gemm(a2, pk2, R, K, N, mask_bits=out["bits"].t)
        _exact(masked["y"].t, bc.gemm_chain(c["a2"], c["w2"], mask=(z > 0))[0], f"mask bits into a second launch, {tag}")
        want, _ = bc.gemm_chain(c["a"], c["w"], c["bias"], residual=c["residual"])
        _exact(_row_gemm(a, pk, R, K, N, bias=bias, residual=res)["y"].t, want, f"bias + residual, {tag}")
        if N == 128:
            gamma, beta = _vec(c["gamma"]), _vec(c["beta"])
            out = _row_gemm(a, pk, R, K, N, bias=bias, residual=res, ln=(gamma, beta), want_pre=True)
            y64, mean, rstd = bc.ln_rows(want, c["gamma"], c["beta"])
            _exact(out["pre"].t, want, f"pre-LayerNorm sum, {tag}")
            _exact(out["mean"].t, mean, f"mean, {tag}")
            rel = float(((out["rstd"].cpu().double() - rstd).abs() / rstd).max())
            ratio = bc.worst_ratio(out["y"].cpu(), y64, bc.ln_out_bar(want, c["gamma"], c["beta"]))
            print(f"row GEMM LayerNorm epilogue {tag}: rstd rel {rel:.2e} (bar {bc.RSTD_REL:.2e}), y error / bar {ratio:.3f}")
            assert rel <= bc.RSTD_REL and ratio <= 1.0, (tag, rel, ratio)


@pytest.mark.parametrize("variant", ["normal", "scaled"])
@pytest.mark.parametrize("K,N", bc.GEMM_SHAPES)
@pytest.mark.parametrize("R", [1, 65, PAST])
def test_row_gemm_inside_the_single_product_bar(R, K, N, variant):
    """N(0,1) rows, and rows x 2^(-30..30) with weight columns x 10^(-3..3): every element of every stored output inside
    2^-8 |want| + (K + 4) 2^-23 (1 + 2^-8) S."""
    R = _rows(R, _row_gemm_grid(K, N))
    c = bc.gemm_random_case(R, K, N, variant)
    a, res, bias = _rows_in(c["a"]), _rows_in(c["residual"]), _vec(c["bias"])
    worst = {}
    for mode in (0, 1):
        pk, _keep = _packed(c["w"], mode)
        for name, kw, dev in (("plain", dict(), dict()), ("bias + ReLU", dict(bias=c["bias"], relu=True), dict(bias=bias, relu=True)),
                              ("bias + residual", dict(bias=c["bias"], residual=c["residual"]), dict(bias=bias, residual=res))):
            want, _ = bc.gemm_chain(c["a"], c["w"], store=False, **kw)
            bar = bc.product_bar(want, bc.gemm_scale(c["a"], c["w"], kw.get("bias"), kw.get("residual")), K)
            got = _row_gemm(a, pk, R, K, N, **dev)["y"].cpu()
            worst[f"{name}, pack mode {mode}"] = bc.worst_ratio(got, want, bar)
        # the ReLU bits of a launch into a second launch of the same geometry: the mask is the sign the first launch stored
        # (an element within rounding of zero may sit on either side of it; which side is not this bar's business)
        first = _row_gemm(a, pk, R, K, N, bias=bias, relu=True, want_bits=True)
        mask = first["y"].cpu().double() > 0
        want, _ = bc.gemm_chain(c["a"], c["w"], mask=mask, store=False)
        got = _row_gemm(a, pk, R, K, N, mask_bits=first["bits"].t)["y"].cpu()
        worst[f"mask bits, pack mode {mode}"] = bc.worst_ratio(got, want, bc.product_bar(want, bc.gemm_scale(c["a"], c["w"]), K))
        if N == 128:      # the pre-LayerNorm sum of the LayerNorm epilogue is a stored single product as well
            g = torch.Generator().manual_seed(K)
            gamma, beta = _vec(torch.rand(N, generator=g) + 0.5), _vec(torch.randn(N, generator=g) * 0.1)
            want, _ = bc.gemm_chain(c["a"], c["w"], c["bias"], residual=c["residual"], store=False)
            pre = _row_gemm(a, pk, R, K, N, bias=bias, residual=res, ln=(gamma, beta), want_pre=True)["pre"].cpu()
            bar = bc.product_bar(want, bc.gemm_scale(c["a"], c["w"], c["bias"], c["residual"]), K)
            worst[f"pre of the LayerNorm epilogue, pack mode {mode}"] = bc.worst_ratio(pre, want, bar)
    for name, ratio in worst.items():
        print(f"row GEMM single-product bar R={R} K={K} N={N} {variant} {name}: worst error / bar {ratio:.3f}")
    assert max(worst.values()) <= 1.0, worst


def test_row_gemm_input_guards_nonfinite_rows_and_reproducibility():
    """Rows >= R of a / residual are never operands (NaN there or zeros: the same bytes out); a NaN, a +inf and a -inf in
    three rows of a poison those rows, non-finite where float64 is, and nothing else; two launches give the same bytes."""
    K, N, R = 384, 128, 129
    c = bc.gemm_random_case(R, K, N)
    pk, _keep = _packed(c["w"], 0)
    bias = _vec(c["bias"])
    run = lambda a, res: _row_gemm(a, pk, R, K, N, bias=bias, residual=res)["y"].t
    clean = run(_rows_in(c["a"]), _rows_in(c["residual"]))
    assert _same_bits(clean, run(_rows_in(c["a"], pad="zero"), _rows_in(c["residual"], pad="zero")))
    assert _same_bits(clean, run(_rows_in(c["a"]), _rows_in(c["residual"])))
    a = c["a"].clone()
    a[3, 7], a[64, 200], a[128, 383] = float("nan"), float("inf"), float("-inf")
    dirty = _row_gemm(_rows_in(a), pk, R, K, N, bias=bias, residual=_rows_in(c["residual"]), check=False)["y"].t
    want, _ = bc.gemm_chain(a, c["w"], c["bias"], residual=c["residual"], store=False)
    hit = [3, 64, 128]
    rest = [r for r in range(R) if r not in hit]
    assert not bool(torch.isfinite(want[hit]).any())                      # (the weights have no zeros)
    assert not bool(torch.isfinite(dirty[hit].float()).any())
    assert _same_bits(dirty[rest], clean[rest])


# ---------------------------------------------------------------------------------------------- weight gradients of given operands
def _wgrad(dy, x, R, N, K, mask=None, bias=True, skinny_f32=False):
    lib = _L().load()
    dw, db = Guarded(N, K, F32), Guarded(N, 1, F32, vector=True)
    ws = torch.empty(int(lib.dg_linear_wgrad_workspace_bytes(R, N, K)), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    if skinny_f32:
        _ok(lib.dg_skinny_linear_wgrad(dy.data_ptr(), x.data_ptr(), dw.ptr(), db.ptr() if bias else None, ws.data_ptr(),
                                       ws.numel(), R, N, K, 1, _stream()), "dg_skinny_linear_wgrad")
    else:
        _ok(lib.dg_linear_wgrad(dy.data_ptr(), None if mask is None else mask.data_ptr(), x.data_ptr(), dw.ptr(),
                                db.ptr() if bias else None, ws.data_ptr(), ws.numel(), R, N, K, 1, _stream()), "dg_linear_wgrad")
    torch.cuda.synchronize()
    dw.check(what=f"dw R={R} N={N} K={K}")
    db.check(written=bias, what=f"db R={R} N={N} K={K}")
    if not bias:
        assert torch.equal(db.raw.cpu(), db.sent), "db written although it was not asked for"
    return dw.cpu(), db.cpu()


def _wgrad_rows(R, N, K):
    """``PAST``: a row count at which every workgroup of dg_linear_wgrad walks at least two of its row tiles, the tail tile
    among them: blocks x 64 + 65, with the block count from the library's workspace query (one [N, K] + [N] float partial per
    block) and 64 rows as an upper bound of the kernel's 16- or 32-row tile."""
    if R != PAST:
        return R
    lib = _L().load()
    blocks = int(lib.dg_linear_wgrad_workspace_bytes(1 << 24, N, K)) // ((N * K + N) * 4)
    assert blocks >= 1
    return blocks * 64 + 65


WGRAD_SHAPES = ([(R, 128, 128) for R in bc.ROW_COUNTS + (4133, PAST)] + [(129, 384, 128), (65, 128, 384), (257, 128, 384),
                                                                          (PAST, 384, 128), (PAST, 128, 384)]
                + [(R, N, 128) for N in (1, 5, 13) for R in (1, 65, 4133)])


@pytest.mark.parametrize("R,N,K", WGRAD_SHAPES)
def test_linear_wgrad_bf16_exact_cases_bit_for_bit(R, N, K):
    """Integer dy / x: dW and db are integer sums below 2^24 and must be exact -- with and without bias, through dy_mask, and on
    the skinny route (N <= 16) with bf16 and with float32 dy."""
    R = _wgrad_rows(R, N, K)
    c = bc.wgrad_exact_case(R, N, K)
    dy, x = _rows_in(c["dy"]), _rows_in(c["x"])
    want_w, want_b = c["dy"].t() @ c["x"], c["dy"].sum(0)
    tag = f"R={R} N={N} K={K}"
    dw, db = _wgrad(dy, x, R, N, K)
    _exact(dw, want_w, f"dw, {tag}")
    _exact(db, want_b, f"db, {tag}")
    dw, _ = _wgrad(dy, x, R, N, K, bias=False)
    _exact(dw, want_w, f"dw without bias, {tag}")
    if N > 16:
        dwm, dbm = _wgrad(dy, x, R, N, K, mask=_rows_in(c["mask"]))
        kept = c["dy"] * (c["mask"] > 0)
        _exact(dwm, kept.t() @ c["x"], f"dw through dy_mask, {tag}")
        _exact(dbm, kept.sum(0), f"db through dy_mask, {tag}")
    else:
        dw, db = _wgrad(_rows_in(c["dy"], F32), x, R, N, K, skinny_f32=True)
        _exact(dw, want_w, f"dw, float32 dy, {tag}")
        _exact(db, want_b, f"db, float32 dy, {tag}")


@pytest.mark.parametrize("R,N,K", [(65, 128, 128), (257, 384, 128), (4133, 128, 384), (PAST, 128, 128), (PAST, 384, 128)])
def test_linear_wgrad_bf16_planted_rows(R, N, K):
    """N(0,1) bf16 operands, dy zero outside the planted rows: every element within (P + 4) 2^-23 S_ij of the float64 sum
    over the planted rows; at the smallest R each planted row alone gives its outer product exactly (a product of two bf16
    numbers is a float32 number); a non-finite planted row poisons what it poisons in float64 and nothing else."""
    past = R == PAST
    R = _wgrad_rows(R, N, K)
    g = torch.Generator().manual_seed(R + N)
    dy_all = bc.bf(torch.randn(R, N, generator=g, dtype=F64))
    x = bc.bf(torch.randn(R, K, generator=g, dtype=F64))
    rows = bc.planted_rows(R, (R - 65) // 64 if past else None)
    dy = bc.plant(dy_all, rows)
    xd = _rows_in(x)
    dw, db = _wgrad(_rows_in(dy), xd, R, N, K)
    A = (len(rows) + 4) * 2.0 ** -23
    rw = bc.worst_ratio(dw, dy.t() @ x, A * (dy.abs().t() @ x.abs()))
    rb = bc.worst_ratio(db, dy.sum(0), A * dy.abs().sum(0))
    print(f"weight gradient planted rows R={R} N={N} K={K}: dw error / bar {rw:.3f}, db error / bar {rb:.3f}")
    assert rw <= 1.0 and rb <= 1.0
    if R == 65:
        for r in rows:
            one = bc.plant(dy_all, [r])
            dw1, db1 = _wgrad(_rows_in(one), xd, R, N, K)
            _exact(dw1, torch.outer(dy_all[r], x[r]), f"row {r} alone, dw")
            _exact(db1, dy_all[r], f"row {r} alone, db")
    bad = x.clone()
    bad[rows[-1], 5] = float("inf")
    dwi, _ = _wgrad(_rows_in(dy), _rows_in(bad), R, N, K)
    want = dy.t() @ bad
    assert torch.equal(torch.isfinite(dwi), torch.isfinite(want))
    assert not bool(torch.isfinite(dwi[:, 5]).any()) and _same_bits(dwi[:, 6:], dw[:, 6:]) and _same_bits(dwi[:, :5], dw[:, :5])


# ---------------------------------------------------------------------------------------------- fused feed-forward
def _ffn_pack(c):
    from druggen_amd.functional.ffn import _ffn_packed_bf16
    w1, w2 = c["w1"].to(F32).cuda(), c["w2"].to(F32).cuda()
    return _ffn_packed_bf16(w1, w2), (w1, w2)


def _ffn_fwd(c, x, packed, check=True):
    lib = _L().load()
    R = c["R"]
    Rp = int(lib.dg_ffn_bf16_padded_rows(R))
    assert R <= Rp < R + 64
    out = dict(y=Guarded(R, 128, BF, alloc=Rp), pre=Guarded(R, 128, BF, alloc=Rp), mean=Guarded(R, 1, F32, alloc=Rp, vector=True),
               rstd=Guarded(R, 1, F32, alloc=Rp, vector=True),
               bits=Guarded(int(lib.dg_ffn_bf16_mask_words(R)), 1, torch.int32, vector=True))
    par = {k: _vec(c[k]) for k in ("b1", "b2", "gamma", "beta")}
    _ok(lib.dg_ffn_ln_fwd_bf16(x.data_ptr(), packed.data_ptr(), par["b1"].data_ptr(), par["b2"].data_ptr(),
                               par["gamma"].data_ptr(), par["beta"].data_ptr(), out["y"].ptr(), out["pre"].ptr(),
                               out["mean"].ptr(), out["rstd"].ptr(), out["bits"].ptr(), R, bc.EPS, _stream()), "dg_ffn_ln_fwd_bf16")
    torch.cuda.synchronize()
    if check:      # written in [0, R); may be written up to dg_ffn_bf16_padded_rows(R); not one element further
        for k, g in out.items():
            g.check(what=f"dg_ffn_ln_fwd_bf16 {k} R={R}")
    out["par"] = par
    return out


def _ffn_bwd(c, x, packed, fwd, dy, want_x=True, want_w=True, check=True):
    lib = _L().load()
    R = c["R"]
    out = dict(dz=Guarded(R, 128, BF), dgamma=Guarded(128, 1, F32, vector=True), dbeta=Guarded(128, 1, F32, vector=True))
    if want_x:
        out["dx"] = Guarded(R, 128, BF)
    if want_w:
        out.update(dw1=Guarded(384, 128, F32), db1=Guarded(384, 1, F32, vector=True), dw2=Guarded(128, 384, F32),
                   db2=Guarded(128, 1, F32, vector=True))
    bits2 = torch.empty_like(fwd["bits"].t)
    ws = torch.empty(int(lib.dg_ffn_bf16_workspace_bytes(R)), dtype=torch.uint8, device="cuda")
    p = lambda k: out[k].ptr() if k in out else None
    _ok(lib.dg_ffn_ln_bwd_bf16(x.data_ptr(), fwd["pre"].ptr(), fwd["mean"].ptr(), fwd["rstd"].ptr(), fwd["bits"].ptr(),
                               fwd["par"]["gamma"].data_ptr(), packed.data_ptr(), fwd["par"]["b1"].data_ptr(), dy.data_ptr(),
                               p("dz"), p("dx"), p("dgamma"), p("dbeta"), p("dw1"), p("db1"), p("dw2"), p("db2"),
                               bits2.data_ptr() if want_w else None, ws.data_ptr(), ws.numel(), R, _stream()), "dg_ffn_ln_bwd_bf16")
    torch.cuda.synchronize()
    if check:
        for k, g in out.items():
            g.check(what=f"dg_ffn_ln_bwd_bf16 {k} R={R}")
    return out


@pytest.mark.parametrize("R", bc.ROW_COUNTS + (PAST,))
def test_fused_ffn_exact_forward_and_planted_row_gradients(R):
    """The integer feed-forward case.  Forward: pre and mean exact, rstd a float32 function of an exact variance, y inside
    the LayerNorm bar, outputs written in [0, R), possibly up to dg_ffn_bf16_padded_rows(R) and not one element further.
    Backward with dy planted in at most 8 rows (tile edges, the tail, a workgroup's second round): dz exactly zero outside
    them, and dw1, db1, dw2, db2, dgamma, dbeta inside the bars of tests/bf16_cases.py -- the ReLU bits of every planted row
    are in dw1 / db1."""
    grid = _ffn_grid()
    R = _rows(R, grid)
    c = bc.ffn_exact_case(R)
    rows = bc.planted_rows(R, grid)
    dy64 = bc.plant(c["dy"], rows)
    ref = bc.ffn_chain(c, F64, dy=dy64)
    x = _rows_in(c["x"])
    packed, _keep = _ffn_pack(c)
    fwd = _ffn_fwd(c, x, packed)
    _exact(fwd["pre"].t, ref["z"], f"pre R={R}")
    _exact(fwd["mean"].t, ref["mean"], f"mean R={R}")
    rel = float(((fwd["rstd"].cpu().double() - ref["rstd"]).abs() / ref["rstd"]).max())
    y64, _, _ = bc.ln_rows(ref["z"], c["gamma"], c["beta"])
    ry = bc.worst_ratio(fwd["y"].cpu(), y64, bc.ln_out_bar(ref["z"], c["gamma"], c["beta"]))
    print(f"fused feed-forward exact case R={R}: rstd rel {rel:.2e} (bar {bc.RSTD_REL:.2e}), y error / bar {ry:.3f}")
    assert rel <= bc.RSTD_REL and ry <= 1.0
    bwd = _ffn_bwd(c, x, packed, fwd, _rows_in(dy64))
    outside = [r for r in range(R) if r not in rows]
    assert not bool(bwd["dz"].cpu()[outside].float().any()) and not bool(bwd["dx"].cpu()[outside].float().any())
    bars = bc.ffn_planted_bars(c, ref, rows)
    ratios = {k: bc.worst_ratio(bwd[k].cpu(), ref[k], bar) for k, bar in bars.items()}
    print(f"fused feed-forward planted rows R={R} rows {rows}: error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    if R == 65:      # every planted row alone, and their float64 sum
        alone = {k: torch.zeros_like(ref[k]) for k in bars}
        alone_bar = {k: bar.clone() for k, bar in bars.items()}      # every single-row launch carries its own error
        for r in rows:
            one64 = bc.plant(c["dy"], [r])
            ref1 = bc.ffn_chain(c, F64, dy=one64)
            got1 = _ffn_bwd(c, x, packed, fwd, _rows_in(one64))
            for k, bar in bc.ffn_planted_bars(c, ref1, [r]).items():
                assert bc.worst_ratio(got1[k].cpu(), ref1[k], bar) <= 1.0, (k, r)
                alone[k] += got1[k].cpu().double()
                alone_bar[k] += bar
        for k in bars:
            assert bc.worst_ratio(bwd[k].cpu(), alone[k], alone_bar[k]) <= 1.0, k


_chain_pool = {}


def _chained(R):
    """Kernel and float32-restatement errors of the chained outputs on the N(0,1) case of R rows, computed once."""
    if R not in _chain_pool:
        c = bc.ffn_random_case(R)
        ref, low = bc.ffn_chain(c, F64), bc.ffn_chain(c, F32)
        x = _rows_in(c["x"])
        packed, _keep = _ffn_pack(c)
        fwd = _ffn_fwd(c, x, packed)
        bwd = _ffn_bwd(c, x, packed, fwd, _rows_in(c["dy"]))
        got = dict(y=fwd["y"].cpu(), dz=bwd["dz"].cpu(), dx=bwd["dx"].cpu())
        peak = lambda t: float((t.abs() / t.pow(2).mean(-1, keepdim=True).sqrt()).max())
        _chain_pool[R] = {k: (bc.row_scaled_errors(got[k], ref[k]), bc.row_scaled_errors(low[k], ref[k]), peak(ref[k])) for k in got}
    return _chain_pool[R]


def test_fused_ffn_chained_outputs_against_the_float32_restatement():
    """y, dz, dx on N(0,1) data at R = 1, 65 and past the grid, each element's error over the rms of its row of the float64
    reference with the kernel's storage points.  Kernel and float32 restatement both differ from it by rare one-ulp
    disagreements, so the three row counts are pooled: kernel max <= 2 x restatement max, kernel rms <= 1.5 x restatement rms."""
    pools = [_chained(_rows(R, _ffn_grid())) for R in (1, 65, PAST)]
    for name in ("y", "dz", "dx"):
        kmax, krms = bc.max_rms(torch.cat([p[name][0] for p in pools]))
        rmax, rrms = bc.max_rms(torch.cat([p[name][1] for p in pools]))
        print(f"fused feed-forward chained {name}: kernel max {kmax:.3e} rms {krms:.3e} | restatement max {rmax:.3e} rms {rrms:.3e}"
              f" | ratios max {kmax / max(rmax, 1e-300):.2f} rms {krms / max(rrms, 1e-300):.2f}")
        assert kmax <= bc.MARGIN_MAX * rmax and krms <= bc.MARGIN_RMS * rrms, name
        # each small row count on its own, so that the large one does not set their bar: the restatement's own max times the
        # margin, or -- where it has no disagreement at all -- two bf16 ulps of the row's largest element (the output's own
        # rounding next to the reference's, and one upstream disagreement carried into it)
        for p in pools[:2]:
            k1, r1 = bc.max_rms(p[name][0])[0], bc.max_rms(p[name][1])[0]
            assert k1 <= max(bc.MARGIN_MAX * r1, 2 * bc.ULP_BF16 * p[name][2]), (name, k1, r1, p[name][2])


def test_fused_ffn_input_guards_nonfinite_rows_and_reproducibility():
    """NaN rows behind x / dy or zeros: the same bytes out of forward and backward; a NaN, a +inf and a -inf in three rows of
    x make those rows of y, pre and dx non-finite and leave every other row bit-identical; two runs give the same bytes."""
    R = 129
    c = bc.ffn_random_case(R)
    packed, _keep = _ffn_pack(c)

    def run(x64, pad, check=True):
        x = _rows_in(x64, pad=pad)
        fwd = _ffn_fwd(c, x, packed, check=check)
        bwd = _ffn_bwd(c, x, packed, fwd, _rows_in(c["dy"], pad=pad), check=check)
        return {**{k: fwd[k].t for k in ("y", "pre", "mean", "rstd")}, **{k: bwd[k].t for k in bwd}}

    clean, zeros, again = run(c["x"], "nan"), run(c["x"], "zero"), run(c["x"], "nan")
    for k in clean:
        assert _same_bits(clean[k], zeros[k]), f"{k}: rows >= R were read"
        assert _same_bits(clean[k], again[k]), f"{k}: two runs differ"
    x = c["x"].clone()
    x[0, 0], x[64, 77], x[128, 127] = float("nan"), float("inf"), float("-inf")
    dirty = run(x, "nan", check=False)
    hit = [0, 64, 128]
    rest = [r for r in range(R) if r not in hit]
    for k in ("y", "dx"):
        assert not bool(torch.isfinite(dirty[k][hit].float()).any()), k
    # (the kernel's ReLU is a max with zero, which drops a NaN: a row of pre is non-finite at least where x is)
    assert not bool(torch.isfinite(dirty["pre"][hit].float()).all(-1).any())
    for k in ("y", "pre", "dx", "mean", "rstd", "dz"):
        assert _same_bits(dirty[k][rest], clean[k][rest]), k


# ---------------------------------------------------------------------------------------------- fused attention half
def _attn_operands(c):
    L = _L()
    lib = L.load()
    we, woe = c["we"].to(F32).cuda(), c["woe"].to(F32).cuda()
    packed = torch.empty(int(lib.dg_attn_half_packed_bytes(1)), dtype=torch.uint8, device="cuda")
    _ok(lib.dg_attn_half_pack(we.data_ptr(), woe.data_ptr(), packed.data_ptr(), 1, _stream()), "dg_attn_half_pack")
    rows = {n: _rows_in(c[n].reshape(-1, 128)) for n in ("y", "q", "k", "v")}
    return packed, rows, {n: _vec(c[n]) for n in ("be", "boe", "gamma", "beta")}


@pytest.mark.parametrize("B,N", [(2, 9), (3, 20), (1, 45), (5, 3)])
def test_attn_half_forward_exact_case(B, N):
    """Integer y, q, k, We, Woe with alpha = 1/4 (exact by construction): the e GEMM, the score, the out_e GEMM, residual and
    bias in one chain -- pre4 equals float64 bit for bit, mean4 too; rstd4, y2 and o inside their bars; guards intact."""
    lib = _L().load()
    c = bc.attn_exact_case(B, N)
    packed, r, par = _attn_operands(c)
    ref = bc.attn_half_chain(c, torch.zeros_like(c["dz"]), torch.zeros_like(c["dO"]))
    R = B * N * N
    out = dict(o=Guarded(B * N, 128, BF), y2=Guarded(R, 128, BF), pre=Guarded(R, 128, BF), mean=Guarded(R, 1, F32, vector=True),
               rstd=Guarded(R, 1, F32, vector=True))
    _ok(lib.dg_attn_half_fwd(r["y"].data_ptr(), r["q"].data_ptr(), r["k"].data_ptr(), r["v"].data_ptr(), packed.data_ptr(),
                             par["be"].data_ptr(), par["boe"].data_ptr(), par["gamma"].data_ptr(), par["beta"].data_ptr(),
                             out["o"].ptr(), out["y2"].ptr(), out["pre"].ptr(), out["mean"].ptr(), out["rstd"].ptr(), B, N, 128,
                             bc.ALPHA, bc.EPS, 1, _stream()), "dg_attn_half_fwd")
    torch.cuda.synchronize()
    for k, g in out.items():
        g.check(what=f"dg_attn_half_fwd {k} B={B} N={N}")
    pre = ref["pre"].reshape(R, 128)
    _exact(out["pre"].t, pre, f"pre4 B={B} N={N}")
    y64, mean, rstd = bc.ln_rows(pre, c["gamma"], c["beta"])
    _exact(out["mean"].t, mean, f"mean4 B={B} N={N}")
    rel = float(((out["rstd"].cpu().double() - rstd).abs() / rstd).max())
    ry = bc.worst_ratio(out["y2"].cpu(), y64, bc.ln_out_bar(pre, c["gamma"], c["beta"]))
    p = torch.softmax(ref["s"], dim=2)
    o_bar = bc.U_BF16 * ref["o"].abs() + 2.0 ** -15 * (p * c["v"][:, None, :, :].abs()).sum(2)
    ro = bc.worst_ratio(out["o"].cpu(), ref["o"].reshape(B * N, 128), o_bar.reshape(B * N, 128))
    print(f"attention half exact case B={B} N={N}: rstd rel {rel:.2e} (bar {bc.RSTD_REL:.2e}), y2 error / bar {ry:.3f}, o error / bar {ro:.3f}")
    assert rel <= bc.RSTD_REL and ry <= 1.0 and ro <= 1.0


@pytest.mark.parametrize("B,N", [(2, 9), (3, 20)])
def test_attn_half_backward_planted_tiles(B, N):
    """dz4 and d_o zero outside the first, a middle and the last (b, i) tile, on the exact forward case: dwe, dbe, dwoe, dboe of
    dg_attn_half_bwd inside the per-element bars of bc.attn_half_chain; each tile alone, summed, gives the same."""
    lib = _L().load()
    c = bc.attn_exact_case(B, N)
    packed, r, par = _attn_operands(c)
    tiles = bc.attn_planted_tiles(B, N)

    def run(which, dz_override=None):
        dz64, dO64 = bc.plant_tiles(c, which)
        if dz_override is not None:
            dz64 = dz_override
        out = dict(dwe=Guarded(128, 128, F32), dbe=Guarded(128, 1, F32, vector=True), dwoe=Guarded(128, 128, F32),
                   dboe=Guarded(128, 1, F32, vector=True), dy=Guarded(B * N * N, 128, BF), dq=Guarded(B * N, 128, BF),
                   dk=Guarded(B * N, 128, BF), dv=Guarded(B * N, 128, BF))
        dz, dO = _rows_in(dz64.reshape(-1, 128)), _rows_in(dO64.reshape(-1, 128))
        ws = torch.empty(int(lib.dg_attn_half_bwd_workspace_bytes(B, N)), dtype=torch.uint8, device="cuda")
        _ok(lib.dg_attn_half_bwd(r["y"].data_ptr(), dz.data_ptr(), r["q"].data_ptr(), r["k"].data_ptr(), r["v"].data_ptr(),
                                 dO.data_ptr(), packed.data_ptr(), par["be"].data_ptr(), out["dy"].ptr(), out["dq"].ptr(),
                                 out["dk"].ptr(), out["dv"].ptr(), out["dwe"].ptr(), out["dbe"].ptr(), out["dwoe"].ptr(),
                                 out["dboe"].ptr(), ws.data_ptr(), ws.numel(), B, N, 128, bc.ALPHA, 1, _stream()), "dg_attn_half_bwd")
        torch.cuda.synchronize()
        for k, g in out.items():
            g.check(written=dz_override is None, what=f"dg_attn_half_bwd {k} B={B} N={N}")
        return {k: g.cpu() for k, g in out.items()}, bc.attn_half_chain(c, dz64, dO64)

    got, ref = run(tiles)
    ratios = {k: bc.worst_ratio(got[k], ref[k], bar) for k, bar in ref["bars"].items()}
    print(f"attention half planted tiles B={B} N={N} tiles {tiles}: error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    outside = [t for t in range(B * N) if t not in tiles]
    assert not bool(got["dy"].view(B * N, N, 128)[outside].float().any())      # a zero tile of dz4 / d_o: a zero tile of dy
    alone = {k: torch.zeros_like(ref[k]) for k in ref["bars"]}
    alone_bar = {k: bar.clone() for k, bar in ref["bars"].items()}      # every single-tile launch carries its own error
    for t in tiles:
        g1, r1 = run([t])
        for k, bar in r1["bars"].items():
            assert bc.worst_ratio(g1[k], r1[k], bar) <= 1.0, (k, t)
            alone[k] += g1[k].double()
            alone_bar[k] += bar
    for k in ref["bars"]:
        assert bc.worst_ratio(got[k], alone[k], alone_bar[k]) <= 1.0, k
    # one planted row of dz4 non-finite: non-finite gradients exactly where float64 has them
    dz64, dO64 = bc.plant_tiles(c, tiles)
    dz64.view(B * N, N, 128)[tiles[-1], 0, 5] = float("inf")
    gi, ri = run(tiles, dz64)
    for k in ref["bars"]:
        assert torch.equal(torch.isfinite(gi[k]), torch.isfinite(ri[k])), k
    assert bool(torch.isfinite(ri["dwoe"]).any()) and not bool(torch.isfinite(ri["dwoe"]).all())


# ---------------------------------------------------------------------------------------------- edge embedding backward
def _embed_bwd(c, g64, want_da=True, act=0, written=True):
    lib = _L().load()
    B, N, E = c["B"], c["N"], c["E"]
    a = _rows_in(c["a"].reshape(-1, E), F32)
    g = _rows_in(g64.reshape(-1, 128))
    par = {n: c[n].to(F32).cuda().contiguous() for n in ("w1", "b1", "w2", "b2")}
    out = dict(dw1=Guarded(64, E, F32), db1=Guarded(64, 1, F32, vector=True), dw2=Guarded(128, 64, F32),
               db2=Guarded(128, 1, F32, vector=True))
    if want_da:
        out["da"] = Guarded(B * N * N, E, F32)
    ws = torch.empty(int(lib.dg_embed_sym_bwd_bf16_workspace_bytes(B, N)), dtype=torch.uint8, device="cuda")
    _ok(lib.dg_embed_sym_bwd_bf16(a.data_ptr(), par["w1"].data_ptr(), par["b1"].data_ptr(), par["w2"].data_ptr(),
                                  par["b2"].data_ptr(), g.data_ptr(), out["da"].ptr() if want_da else None, out["dw1"].ptr(),
                                  out["db1"].ptr(), out["dw2"].ptr(), out["db2"].ptr(), ws.data_ptr(), ws.numel(), B, N, E, 64, 128,
                                  act, _stream()), "dg_embed_sym_bwd_bf16")
    torch.cuda.synchronize()
    for k, gd in out.items():
        gd.check(written=written, what=f"dg_embed_sym_bwd_bf16 {k} B={B} N={N} E={E}")
    return {k: gd.cpu() for k, gd in out.items()}


@pytest.mark.parametrize("B,N,E", [(1, 1, 5), (2, 6, 5), (3, 15, 1), (2, 16, 8), (2, 17, 3), (2, 32, 5), (1, 33, 8), (3, 45, 5),
                                    (1, 48, 2), (33, 16, 8), (12, 45, 5)])
def test_embed_sym_bwd_bf16_exact_cases_bit_for_bit(B, N, E):
    """Integer a, W1, W2 and even integer g (exact by construction, relu): da and every parameter gradient of
    dg_embed_sym_bwd_bf16 equal float64, element by element -- at N around the kernel's 16-row blocks and at B N > 512 tiles,
    where a workgroup walks more than one tile (double-buffered g tiles, da one tile late).  Then g planted in the first, a
    middle and the last (b, i) row block only: the same equality, and each block alone (smallest shape) sums to the whole."""
    c = bc.embed_exact_case(B, N, E)
    ref = bc.embed_chain(c)
    got = _embed_bwd(c, c["g"])
    for k in ("da", "dw1", "db1", "dw2", "db2"):
        _exact(got[k], ref[k].reshape(got[k].shape), f"{k} B={B} N={N} E={E}")
    nd = _embed_bwd(c, c["g"], want_da=False)
    for k in ("dw1", "db1", "dw2", "db2"):
        _exact(nd[k], ref[k], f"{k} without da, B={B} N={N} E={E}")
    tiles = bc.attn_planted_tiles(B, N)

    def plant(which):
        z = torch.zeros_like(c["g"])
        z.view(B * N, N, 128)[which] = c["g"].view(B * N, N, 128)[which]
        return z

    gp = plant(tiles)
    refp, gotp = bc.embed_chain(c, gp), _embed_bwd(c, gp)
    for k in ("da", "dw1", "db1", "dw2", "db2"):
        _exact(gotp[k], refp[k].reshape(gotp[k].shape), f"{k}, planted row blocks {tiles}, B={B} N={N} E={E}")
    if (B, N) == (2, 6):
        total = {k: torch.zeros_like(refp[k]) for k in ("dw1", "db1", "dw2", "db2")}
        for t in tiles:
            g1 = plant([t])
            one, ref1 = _embed_bwd(c, g1), bc.embed_chain(c, g1)
            for k in total:
                _exact(one[k], ref1[k], f"{k}, row block {t} alone")
                total[k] += one[k].double()
        for k in total:
            _exact(gotp[k], total[k], f"{k}: the planted blocks one by one")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B,N,E", [(2, 6, 5), (3, 17, 8), (2, 45, 1), (12, 45, 5)])
def test_embed_sym_bwd_bf16_inside_the_stored_chain_bars(B, N, E, act):
    """relu and leaky on N(0,1) data (softmax a, float32 parameters that are not bf16 numbers, bf16 g): da and the four
    parameter gradients inside the per-element bars of bc.embed_stored_chain, whose float64 reference has the kernel's storage
    points (bf16 h, dpre2, W2, W1 and, for da, dpre1)."""
    slope = 0.01 if act else 0.0
    c = bc.embed_random_case(B, N, E)
    ref = bc.embed_stored_chain(c, slope)
    got = _embed_bwd(c, c["g"], act=act)
    ratios = {k: bc.worst_ratio(got[k], ref[k].reshape(got[k].shape), bar.reshape(got[k].shape)) for k, bar in ref["bars"].items()}
    print(f"embedding stored-chain bars B={B} N={N} E={E} act {act}: error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("act", [0, 1])
def test_embed_sym_bwd_bf16_nonfinite_planted_row(act):
    """g planted in three (b, i) row blocks with one +inf in one of their rows: every parameter gradient and da non-finite
    exactly where the float64 chain is (a masked ReLU element is 0, not 0 * inf, as in autograd), finite elsewhere."""
    B, N, E = 2, 6, 5
    c = bc.embed_random_case(B, N, E)
    tiles = bc.attn_planted_tiles(B, N)
    g = torch.zeros_like(c["g"])
    g.view(B * N, N, 128)[tiles] = c["g"].view(B * N, N, 128)[tiles]
    clean = _embed_bwd(c, g, act=act)
    slope = 0.01 if act else 0.0
    # the channel: one whose pre2 is positive at (b, i, j) and not at (b, j, i), so that the +inf meets act' on both sides
    b, i, j = tiles[-1] // N, tiles[-1] % N, 1
    pre1 = c["a"] @ c["w1"].t() + c["b1"]
    pre2 = torch.where(pre1 > 0, pre1, slope * pre1) @ c["w2"].t() + c["b2"]
    ch = int(((pre2[b, i, j] > 0) & (pre2[b, j, i] <= 0)).nonzero()[0])
    g[b, i, j, ch] = float("inf")
    ref = bc.embed_stored_chain(c, slope, g=g)
    got = _embed_bwd(c, g, act=act, written=False)
    for k in ("da", "dw1", "db1", "dw2", "db2"):
        assert torch.equal(torch.isfinite(got[k]), torch.isfinite(ref[k]).reshape(got[k].shape)), k
    keep = [x for x in range(128) if x != ch]
    assert not bool(torch.isfinite(got["dw2"][ch]).any()) and not bool(torch.isfinite(got["db2"][ch]))
    assert _same_bits(got["dw2"][keep], clean["dw2"][keep]) and _same_bits(got["db2"][keep], clean["db2"][keep])


def test_fused_ffn_nonfinite_planted_row():
    """dy planted in the named rows of the exact case with one +inf in the last planted row: dz, dx and all six parameter
    gradients of dg_ffn_ln_bwd_bf16 non-finite exactly where the float64 chain is; dbeta and dgamma keep the bits of the clean
    planted run in every other channel."""
    R = 129
    c = bc.ffn_exact_case(R)
    rows = bc.planted_rows(R)
    x = _rows_in(c["x"])
    packed, _keep = _ffn_pack(c)
    fwd = _ffn_fwd(c, x, packed)
    dy64 = bc.plant(c["dy"], rows)
    clean = _ffn_bwd(c, x, packed, fwd, _rows_in(dy64))
    dy64[rows[-1], 5] = float("inf")
    ref = bc.ffn_chain(c, F64, dy=dy64)
    got = _ffn_bwd(c, x, packed, fwd, _rows_in(dy64), check=False)
    for k in ("dz", "dx", "dw1", "db1", "dw2", "db2", "dgamma", "dbeta"):
        assert torch.equal(torch.isfinite(got[k].cpu().float()), torch.isfinite(ref[k])), k
    keep = [ch for ch in range(128) if ch != 5]
    for k in ("dgamma", "dbeta"):
        assert not bool(torch.isfinite(got[k].cpu()[5])) and _same_bits(got[k].cpu()[keep], clean[k].cpu()[keep]), k
    assert bool(torch.isfinite(ref["dw1"]).any()) and not bool(torch.isfinite(ref["dw1"]).all())      # rows of dw1 follow the ReLU bits


def test_attn_half_forward_nonfinite_rows():
    """A NaN, a +inf and a -inf in three rows of y, in three different (b, i) tiles of N(0,1) data: those rows of pre4 and y2
    are non-finite, and so are the node outputs o of their tiles (all of the NaN tile's, some channels of the others'); every other row of pre4, y2, mean4, rstd4 and o keeps its bits."""
    lib = _L().load()
    B, N = 2, 9
    R = B * N * N
    g = torch.Generator().manual_seed(11)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    we, woe = rn(128, 128, scale=128 ** -0.5).cuda(), rn(128, 128, scale=128 ** -0.5).cuda()
    packed = torch.empty(int(lib.dg_attn_half_packed_bytes(1)), dtype=torch.uint8, device="cuda")
    _ok(lib.dg_attn_half_pack(we.data_ptr(), woe.data_ptr(), packed.data_ptr(), 1, _stream()), "dg_attn_half_pack")
    be, boe, b4, g4 = rn(128, scale=0.1).cuda(), rn(128, scale=0.1).cuda(), rn(128, scale=0.1).cuda(), (1 + rn(128, scale=0.1)).cuda()
    y64 = rn(R, 128, scale=0.7).double()
    q, k, v = (_rows_in(rn(B * N, 128).double()) for _ in range(3))

    def run(y_rows):
        y = _rows_in(y_rows)
        out = dict(o=Guarded(B * N, 128, BF), y2=Guarded(R, 128, BF), pre=Guarded(R, 128, BF),
                   mean=Guarded(R, 1, F32, vector=True), rstd=Guarded(R, 1, F32, vector=True))
        _ok(lib.dg_attn_half_fwd(y.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), packed.data_ptr(), be.data_ptr(),
                                 boe.data_ptr(), g4.data_ptr(), b4.data_ptr(), out["o"].ptr(), out["y2"].ptr(), out["pre"].ptr(),
                                 out["mean"].ptr(), out["rstd"].ptr(), B, N, 128, bc.ALPHA, bc.EPS, 1, _stream()), "dg_attn_half_fwd")
        torch.cuda.synchronize()
        for g_ in out.values():
            g_.check(written=False)
        return {n: g_.t for n, g_ in out.items()}

    clean = run(y64)
    hit = [(0, 3), (N + 2, 0), (B * N - 1, N - 1)]          # (tile, row j)
    bad = y64.clone()
    for (t, j), val in zip(hit, (float("nan"), float("inf"), float("-inf"))):
        bad[t * N + j, 17] = val
    dirty = run(bad)
    hit_rows, hit_tiles = [t * N + j for t, j in hit], [t for t, _ in hit]
    rest_rows = [r for r in range(R) if r not in hit_rows]
    rest_tiles = [t for t in range(B * N) if t not in hit_tiles]
    for n in ("pre", "y2"):
        assert not bool(torch.isfinite(dirty[n][hit_rows].float()).all(-1).any()), n
        assert _same_bits(dirty[n][rest_rows], clean[n][rest_rows]), n
    assert not bool(torch.isfinite(dirty["y2"][hit_rows].float()).any())
    for n in ("mean", "rstd"):
        assert _same_bits(dirty[n][rest_rows], clean[n][rest_rows]), n
    # (a channel whose score is -inf at the hit row has softmax weight 0 there: o stays finite in it; NaN spares none)
    assert not bool(torch.isfinite(dirty["o"][hit_tiles[0]].float()).any())
    assert not bool(torch.isfinite(dirty["o"][hit_tiles].float()).all(-1).any())
    assert _same_bits(dirty["o"][rest_tiles], clean["o"][rest_tiles])


# ---------------------------------------------------------------------------------------------- graph replay
def test_graph_replay_on_new_contents_equals_eager():
    """dg_row_gemm (bf16), dg_linear_wgrad (bf16) and the fused feed-forward pair captured once at R = 65 and replayed on new
    contents of the same buffers: the bytes of an eager run on those contents."""
    lib = _L().load()
    R = 65
    cg, cg2 = bc.gemm_random_case(R, 128, 128), bc.gemm_random_case(R, 128, 128, seed=1)
    cf, cf2 = bc.ffn_random_case(R), bc.ffn_random_case(R, seed=1)
    pk, _keep = _packed(cg["w"], 0)
    packed, _keep2 = _ffn_pack(cf)
    a, res, bias = _rows_in(cg["a"]), _rows_in(cg["residual"]), _vec(cg["bias"])
    x, dy = _rows_in(cf["x"]), _rows_in(cf["dy"])
    par = {k: _vec(cf[k]) for k in ("b1", "b2", "gamma", "beta")}
    Rp = int(lib.dg_ffn_bf16_padded_rows(R))
    new = lambda *s, dtype=BF: torch.empty(*s, dtype=dtype, device="cuda")
    y, fy, pre, dz, dx = new(R, 128), new(Rp, 128), new(Rp, 128), new(R, 128), new(R, 128)
    mean, rstd, dgam, dbet = new(Rp, dtype=F32), new(Rp, dtype=F32), new(128, dtype=F32), new(128, dtype=F32)
    dw1, db1, dw2, db2 = new(384, 128, dtype=F32), new(384, dtype=F32), new(128, 384, dtype=F32), new(128, dtype=F32)
    gw, gb = new(128, 128, dtype=F32), new(128, dtype=F32)
    bits = new(int(lib.dg_ffn_bf16_mask_words(R)), dtype=torch.int32)
    bits2 = torch.empty_like(bits)
    ws = new(int(lib.dg_ffn_bf16_workspace_bytes(R)), dtype=torch.uint8)
    wsg = new(int(lib.dg_linear_wgrad_workspace_bytes(R, 128, 128)), dtype=torch.uint8)
    outs = dict(y=y, fy=fy[:R], pre=pre[:R], mean=mean[:R], rstd=rstd[:R], dz=dz, dx=dx, dgam=dgam, dbet=dbet, dw1=dw1, db1=db1,
                dw2=dw2, db2=db2, gw=gw, gb=gb)

    def launch():
        s = _stream()
        _ok(lib.dg_row_gemm(a.data_ptr(), pk.data_ptr(), y.data_ptr(), R, 128, 128, bias.data_ptr(), 0, None, None, res.data_ptr(),
                            None, None, None, None, None, bc.EPS, 1, s), "dg_row_gemm")
        _ok(lib.dg_linear_wgrad(res.data_ptr(), None, a.data_ptr(), gw.data_ptr(), gb.data_ptr(), wsg.data_ptr(), wsg.numel(),
                                R, 128, 128, 1, s), "dg_linear_wgrad")
        _ok(lib.dg_ffn_ln_fwd_bf16(x.data_ptr(), packed.data_ptr(), par["b1"].data_ptr(), par["b2"].data_ptr(),
                                   par["gamma"].data_ptr(), par["beta"].data_ptr(), fy.data_ptr(), pre.data_ptr(), mean.data_ptr(),
                                   rstd.data_ptr(), bits.data_ptr(), R, bc.EPS, s), "dg_ffn_ln_fwd_bf16")
        _ok(lib.dg_ffn_ln_bwd_bf16(x.data_ptr(), pre.data_ptr(), mean.data_ptr(), rstd.data_ptr(), bits.data_ptr(),
                                   par["gamma"].data_ptr(), packed.data_ptr(), par["b1"].data_ptr(), dy.data_ptr(), dz.data_ptr(),
                                   dx.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(),
                                   db2.data_ptr(), bits2.data_ptr(), ws.data_ptr(), ws.numel(), R, s), "dg_ffn_ln_bwd_bf16")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                      # warm-up outside the capture (LDS opt-in attributes are set at first use)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    warm = {k: v.clone() for k, v in outs.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    a.copy_(cg2["a"].to(BF))
    res.copy_(cg2["residual"].to(BF))
    x.copy_(cf2["x"].to(BF))
    dy.copy_(cf2["dy"].to(BF))
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in outs.items()}
    for v in outs.values():
        v.zero_()
    launch()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert _same_bits(replayed[k], v), k
        assert not _same_bits(warm[k], v), f"{k}: the new contents changed nothing"


def test_attn_half_and_embedding_graph_replay_on_new_contents_equals_eager():
    """dg_attn_half_fwd / _bwd at (B, N) = (2, 9) and dg_embed_sym_bwd_bf16 at (2, 6, 5) on N(0,1) data: two eager runs give the
    same bytes, and one captured-graph replay on new contents of the same buffers equals the eager run on them."""
    lib = _L().load()
    g = torch.Generator().manual_seed(5)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    B, N = 2, 9
    R = B * N * N
    we, woe = rn(128, 128, scale=128 ** -0.5).cuda(), rn(128, 128, scale=128 ** -0.5).cuda()
    packed = torch.empty(int(lib.dg_attn_half_packed_bytes(1)), dtype=torch.uint8, device="cuda")
    _ok(lib.dg_attn_half_pack(we.data_ptr(), woe.data_ptr(), packed.data_ptr(), 1, _stream()), "dg_attn_half_pack")
    par = [rn(128, scale=0.1).cuda() for _ in range(3)] + [(1 + rn(128, scale=0.1)).cuda()]      # be, boe, beta4, gamma4
    be, boe, b4, g4 = par
    fresh = lambda: dict(y=rn(R, 128, scale=0.7).to(BF), q=rn(B * N, 128).to(BF), k=rn(B * N, 128).to(BF), v=rn(B * N, 128).to(BF),
                         dz=rn(R, 128).to(BF), dO=rn(B * N, 128).to(BF))
    first, second = fresh(), fresh()
    inp = {n: t.cuda() for n, t in first.items()}
    new = lambda *s, dtype=BF: torch.empty(*s, dtype=dtype, device="cuda")
    out = dict(o=new(B * N, 128), y2=new(R, 128), pre=new(R, 128), mean=new(R, dtype=F32), rstd=new(R, dtype=F32), dy=new(R, 128),
               dq=new(B * N, 128), dk=new(B * N, 128), dv=new(B * N, 128), dwe=new(128, 128, dtype=F32), dbe=new(128, dtype=F32),
               dwoe=new(128, 128, dtype=F32), dboe=new(128, dtype=F32))
    ws = new(int(lib.dg_attn_half_bwd_workspace_bytes(B, N)), dtype=torch.uint8)
    # embedding
    EB, EN, EE = 2, 6, 5
    ea1, ea2 = (torch.softmax(2 * rn(EB * EN * EN, EE), -1) for _ in range(2))
    eg1, eg2 = (rn(EB * EN * EN, 128).to(BF) for _ in range(2))
    ea, eg = ea1.cuda(), eg1.cuda()
    ew1, eb1, ew2, eb2 = rn(64, EE, scale=0.5).cuda(), rn(64, scale=0.1).cuda(), rn(128, 64, scale=0.15).cuda(), rn(128, scale=0.1).cuda()
    out.update(da=new(EB * EN * EN, EE, dtype=F32), dw1=new(64, EE, dtype=F32), db1=new(64, dtype=F32), dw2=new(128, 64, dtype=F32),
               db2=new(128, dtype=F32))
    ews = new(int(lib.dg_embed_sym_bwd_bf16_workspace_bytes(EB, EN)), dtype=torch.uint8)
    P = lambda t: t.data_ptr()

    def launch():
        s = _stream()
        _ok(lib.dg_attn_half_fwd(P(inp["y"]), P(inp["q"]), P(inp["k"]), P(inp["v"]), P(packed), P(be), P(boe), P(g4), P(b4),
                                 P(out["o"]), P(out["y2"]), P(out["pre"]), P(out["mean"]), P(out["rstd"]), B, N, 128, bc.ALPHA,
                                 bc.EPS, 1, s), "dg_attn_half_fwd")
        _ok(lib.dg_attn_half_bwd(P(inp["y"]), P(inp["dz"]), P(inp["q"]), P(inp["k"]), P(inp["v"]), P(inp["dO"]), P(packed), P(be),
                                 P(out["dy"]), P(out["dq"]), P(out["dk"]), P(out["dv"]), P(out["dwe"]), P(out["dbe"]),
                                 P(out["dwoe"]), P(out["dboe"]), P(ws), ws.numel(), B, N, 128, bc.ALPHA, 1, s), "dg_attn_half_bwd")
        _ok(lib.dg_embed_sym_bwd_bf16(P(ea), P(ew1), P(eb1), P(ew2), P(eb2), P(eg), P(out["da"]), P(out["dw1"]), P(out["db1"]),
                                      P(out["dw2"]), P(out["db2"]), P(ews), ews.numel(), EB, EN, EE, 64, 128, 0, s),
            "dg_embed_sym_bwd_bf16")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    once = {k_: v_.clone() for k_, v_ in out.items()}
    launch()
    torch.cuda.synchronize()
    for k_, v_ in out.items():
        assert _same_bits(once[k_], v_), f"{k_}: two runs differ"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for n, t in second.items():
        inp[n].copy_(t)
    ea.copy_(ea2)
    eg.copy_(eg2)
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k_: v_.clone() for k_, v_ in out.items()}
    for v_ in out.values():
        v_.zero_()
    launch()
    torch.cuda.synchronize()
    for k_, v_ in out.items():
        assert _same_bits(replayed[k_], v_), k_
        assert not _same_bits(once[k_], v_), f"{k_}: the new contents changed nothing"


# ---------------------------------------------------------------------------------------------- misaligned pointers
def test_misaligned_pointers_are_refused_before_any_launch():
    """The bf16 row kernels fetch rows by 16-byte LDS-DMA: a base pointer off 16 bytes is DG_E_ARG and nothing is launched
    (the outputs keep their bytes)."""
    lib = _L().load()
    R = 65
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((1 << 18,), 7, dtype=torch.uint8, device="cuda")
    p, o, s = buf.data_ptr(), out.data_ptr(), _stream()
    E_ARG = -2
    for off in (2, 8):
        assert lib.dg_row_gemm(p + off, p, o, R, 128, 128, None, 0, None, None, None, None, None, None, None, None, 1e-5, 1, s) == E_ARG
        assert b"misaligned" in lib.dg_last_error_string()
        assert lib.dg_row_gemm(p, p + off, o, R, 128, 128, None, 0, None, None, None, None, None, None, None, None, 1e-5, 1, s) == E_ARG
        assert lib.dg_row_gemm(p, p, o + off, R, 128, 128, None, 0, None, None, None, None, None, None, None, None, 1e-5, 1, s) == E_ARG
        assert lib.dg_row_gemm(p, p, o, R, 128, 128, None, 0, None, None, p + off, None, None, None, None, None, 1e-5, 1, s) == E_ARG
        assert lib.dg_ffn_ln_fwd_bf16(p + off, p, p, p, p, p, o, o, o, o, o, R, 1e-5, s) == E_ARG
        assert lib.dg_ffn_ln_fwd_bf16(p, p, p, p, p, p, o + off, o, o, o, o, R, 1e-5, s) == E_ARG
        assert lib.dg_ffn_ln_fwd_bf16(p, p, p, p, p, p, o, o + off, o, o, o, R, 1e-5, s) == E_ARG
        big = 1 << 20
        assert lib.dg_ffn_ln_bwd_bf16(p + off, p, p, p, p, p, p, p, p, o, o, o, o, o, o, o, o, o, o, big, R, s) == E_ARG
        assert lib.dg_ffn_ln_bwd_bf16(p, p, p, p, p, p, p, p, p + off, o, o, o, o, o, o, o, o, o, o, big, R, s) == E_ARG
        assert lib.dg_ffn_ln_bwd_bf16(p, p, p, p, p, p, p, p, p, o + off, o, o, o, o, o, o, o, o, o, big, R, s) == E_ARG
        assert lib.dg_ffn_ln_bwd_bf16(p, p, p, p, p, p, p, p, p, o, o, o, o, o, o, o, o, o, o + off, big, R, s) == E_ARG
        assert lib.dg_embed_sym_bwd_bf16(p, p, p, p, p, p + off, o, o, o, o, o, o, 1 << 30, 1, 9, 5, 64, 128, 0, s) == E_ARG
        assert lib.dg_embed_sym_bwd_bf16(p, p, p, p, p, p, o, o, o, o, o, o + off, 1 << 30, 1, 9, 5, 64, 128, 0, s) == E_ARG
        assert b"misaligned" in lib.dg_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and not bool(buf.any())
